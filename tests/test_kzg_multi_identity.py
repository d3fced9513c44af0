"""CPU: the equation include/playsnark_hip.h states for ps_kzg_verify_multi, pinned against a second implementation -- two
polynomials (2 and 5 coefficients) opened at two points with one proof per point, everything computed with the oracle alone
(oracle.pyref for polynomials and groups, oracle.pairing.pair for the pairing), satisfy
    e(sum_i w_i C_i + sum_j rho_j z_j pi_j - s G1, G2) * e(-sum_j rho_j pi_j, tau G2) == 1,
    w_i = sum_j rho_j c_ij,  s = sum_j rho_j sum_i c_ij y_ij,
under 128-bit weights rho, and fail it with one value changed.  No library code runs here."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % (2**250)


def test_the_header_states_this_equation():
    h = open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()
    assert "e(sum_i w_i C_i + sum_j rho_j z_j pi_j - s G1, G2) * e(-sum_j rho_j pi_j, tau_g2_1) == 1" in h
    assert "w_i = sum_j rho_j c_ij and s = sum_j rho_j sum_i c_ij y_ij" in h


def _lhs(pr, commits, zs, coef, ys, proofs, rhos):
    """(A, B): the two G1 points of the equation."""
    m, t = len(commits), len(zs)
    A = B = None
    s = 0
    for i in range(m):
        w = sum(rhos[j] * coef[i][j] for j in range(t)) % pr.R
        A = pr.G1.add(A, pr.G1.mul_pt(w, commits[i]))
    for j in range(t):
        A = pr.G1.add(A, pr.G1.mul_pt(rhos[j] * zs[j] % pr.R, proofs[j]))
        B = pr.G1.add(B, pr.G1.mul_pt(rhos[j], proofs[j]))
        s = (s + rhos[j] * sum(coef[i][j] * ys[i][j] for i in range(m))) % pr.R
    return pr.G1.add(A, pr.G1.neg(pr.G1.mul(s))), B


def test_the_multi_equation_holds_for_oracle_openings_and_fails_for_a_changed_value(pr):
    from oracle import pairing

    rng = pr.SplitMix64(0x4B5A4D)
    G2, tau_g2 = pr.G2.mul(1), pr.G2.mul(TAU)
    polys = [[rng.fr() for _ in range(n)] for n in (2, 5)]
    zs = [rng.fr(), rng.fr()]
    coef = [[rng.fr(), rng.fr()], [rng.fr(), rng.fr()]]
    commits = [pr.G1.mul(pr.poly_eval(p, TAU)) for p in polys]
    ys = [[pr.poly_eval(p, z) for z in zs] for p in polys]
    proofs = []
    for j, z in enumerate(zs):
        f = [0]
        for i, p in enumerate(polys):
            f = pr.poly_add(f, [coef[i][j] * a % pr.R for a in p])
        q, rem = pr.poly_div(f[::-1], [1, (-z) % pr.R])  # Poly.Div, highest degree first (algebra.go:119-137)
        assert rem[0] == sum(coef[i][j] * ys[i][j] for i in range(2)) % pr.R
        proofs.append(pr.G1.mul(pr.poly_eval(q[::-1], TAU)))
    rhos = [((rng.next() << 64) | rng.next()) or 1 for _ in zs]
    one = pairing.pair(None, G2)  # (the identity in a slot costs no Miller loop)
    A, B = _lhs(pr, commits, zs, coef, ys, proofs, rhos)
    right = pairing.pair(pr.G1.neg(B), tau_g2)
    assert pairing.gt_mul(pairing.pair(A, G2), right) == one
    ys[1][0] = (ys[1][0] + 1) % pr.R
    A, B2 = _lhs(pr, commits, zs, coef, ys, proofs, rhos)
    assert B2 == B
    assert pairing.gt_mul(pairing.pair(A, G2), right) != one
