"""CPU: the equations include/playsnark_hip.h states for ps_kzg_verify and ps_kzg_verify_batch, pinned against a second
implementation -- openings computed with the oracle alone (oracle.pyref for polynomials and groups, oracle.pairing.pair for the
pairing) satisfy them, and an opening to another value does not:
    e(C - y G1 + z pi, G2) = e(pi, tau G2)                                            n = 2 and 5
    e(sum_j rho_j (C_j + z_j pi_j) - (sum_j rho_j y_j) G1, G2) e(-sum_j rho_j pi_j, tau G2) = 1     k = 2
No library code runs here."""
import re
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % (2**250)


def _open(pr, p, z):
    """(C, y, pi) as oracle points / integers: the quotient through Poly.Div, highest degree first (algebra.go:119-137)."""
    q, rem = pr.poly_div(p[::-1], [1, (-z) % pr.R])
    y = rem[0]
    assert y == pr.poly_eval(p, z)
    return pr.G1.mul(pr.poly_eval(p, TAU)), y, pr.G1.mul(pr.poly_eval(q[::-1], TAU))


def _lhs_point(pr, C, z, y, pi):
    return pr.G1.add(pr.G1.add(C, pr.G1.neg(pr.G1.mul(y))), pr.G1.mul_pt(z, pi))


def test_the_header_states_these_equations():
    h = open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()
    assert "e(commit - y G1 + z proof, G2) = e(proof, tau_g2_1)" in h
    assert re.search(r"e\(sum_j rho_j \(C_j \+ z_j pi_j\) - \(sum_j rho_j y_j\) G1, G2\) \* e\(-sum_j rho_j pi_j, tau_g2_1\) == 1", h)


def test_single_and_batch_equations_hold_for_oracle_openings(pr):
    from oracle import pairing

    rng = pr.SplitMix64(0x4B5A47)
    G2, tau_g2 = pr.G2.mul(1), pr.G2.mul(TAU)
    opened = []
    for n in (2, 5):
        p = [rng.fr() for _ in range(n)]
        z = rng.fr()
        C, y, pi = _open(pr, p, z)
        opened.append((C, z, y, pi))
        right = pairing.pair(pi, tau_g2)
        assert pairing.pair(_lhs_point(pr, C, z, y, pi), G2) == right, n
        if n == 5:  # the same opening with another value is not accepted
            assert pairing.pair(_lhs_point(pr, C, z, (y + 1) % pr.R, pi), G2) != right
    # the batch equation for k = 2, 128-bit weights; e(-B, tau G2) = 1 / e(B, tau G2)
    rhos = [((rng.next() << 64) | rng.next()) or 1 for _ in opened]
    A = B = None
    s = 0
    for rho, (C, z, y, pi) in zip(rhos, opened):
        A = pr.G1.add(A, pr.G1.mul_pt(rho, pr.G1.add(C, pr.G1.mul_pt(z, pi))))
        B = pr.G1.add(B, pr.G1.mul_pt(rho, pi))
        s = (s + rho * y) % pr.R
    A = pr.G1.add(A, pr.G1.neg(pr.G1.mul(s)))
    one = pairing.pair(None, G2)  # (the identity in a slot costs no Miller loop)
    assert pairing.gt_mul(pairing.pair(A, G2), pairing.pair(pr.G1.neg(B), tau_g2)) == one
