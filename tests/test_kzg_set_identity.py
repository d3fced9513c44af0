"""CPU, pure Python over the oracle: the identity ps_poly_div_roots and ps_kzg_open_set stand on.  For k distinct points z_j,
with w_j = 1 / prod_{l != j} (z_j - z_l) and q_j = (p - p(z_j)) / (X - z_j),
    sum_j w_j q_j  ==  the quotient of Poly.Div(p, Z_S),   Z_S = prod_j (X - z_j)
coefficient by coefficient; the top k - 1 coefficients of the weighted sum are zero; the remainder of that division is the
interpolant of (z_j, p(z_j)).  And the equation ps_kzg_verify_set checks, e(C - [r(tau)] G1, G2) e(-pi, [Z_S(tau)] G2) = 1,
holds with the oracle's pairing, fails with one value changed and with two values swapped, and is ps_kzg_verify's at k = 1."""
import pytest

from oracle import pairing
from oracle import pyref as pr

R = pr.R
TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
SHAPES = [(5, 2), (9, 3), (40, 8), (2049, 3), (300, 33)]


def _points(rng, n, k):
    zs = [rng.fr() for _ in range(k)]
    if n >= 40:  # the larger shapes hold the edge points
        zs[: min(4, k)] = [0, 1, R - 1, 2][: min(4, k)]
    assert len(set(zs)) == k
    return zs


def _linear_quotient(p, z):
    """(p - p(z)) / (X - z), lowest first, and p(z): the recurrence h_i = p_i + z h_{i+1} of the scan"""
    h, out = 0, [0] * (len(p) - 1)
    for i in range(len(p) - 1, 0, -1):
        h = (p[i] + z * h) % R
        out[i - 1] = h
    return out, (p[0] + z * h) % R


def _vanishing(zs):
    zp = [1]
    for z in zs:
        zp = pr.poly_mul(zp, [(-z) % R, 1])
    return zp


def _weights(zs):
    ws = []
    for j, zj in enumerate(zs):
        d = 1
        for l, zl in enumerate(zs):
            if l != j:
                d = d * (zj - zl) % R
        ws.append(pr.fr_inv(d))
    return ws


def _div_roots(p, zs):
    """(q, rem) of Poly.Div(p, Z_S), both lowest first (the oracle's division takes highest-first order)"""
    q, rem = pr.poly_div(p[::-1], _vanishing(zs)[::-1])
    return q[::-1], rem[::-1]


@pytest.mark.parametrize("n,k", SHAPES)
def test_the_weighted_sum_of_linear_quotients_is_the_quotient_by_the_vanishing_polynomial(n, k):
    rng = pr.SplitMix64(0x5E7 + 1000 * n + k)
    p = [rng.fr() for _ in range(n)]
    zs = _points(rng, n, k)
    ws = _weights(zs)
    acc = [0] * (n - 1)
    ys = []
    for z, w in zip(zs, ws):
        qj, y = _linear_quotient(p, z)
        assert y == pr.poly_eval(p, z)
        ys.append(y)
        acc = [(a + w * c) % R for a, c in zip(acc, qj)]
    q, rem = _div_roots(p, zs)
    assert len(q) == n - k and len(rem) == k
    assert acc[: n - k] == q  # coefficient by coefficient
    assert acc[n - k :] == [0] * (k - 1)  # the top k - 1 cancel
    assert [pr.poly_eval(rem, z) for z in zs] == ys  # the remainder is the interpolant
    # and p = q Z_S + rem
    assert pr.poly_add(pr.poly_mul(q, _vanishing(zs)), rem) == p


def _set_equation(commit, r_tau, proof, zs_tau_g2, pi_side=None):
    """e(C - [r(tau)] G1, G2) == e(pi, [Z_S(tau)] G2)"""
    lhs = pairing.pair(pr.G1.add(commit, pr.G1.neg(pr.G1.mul(r_tau))), pr.G2.mul(1))
    return lhs == (pi_side if pi_side is not None else pairing.pair(proof, zs_tau_g2))


def test_the_verification_equation_holds_and_fails_with_a_changed_and_with_swapped_values():
    rng = pr.SplitMix64(0x9E3)
    p = [rng.fr() for _ in range(9)]
    zs = [rng.fr() for _ in range(3)]
    q, rem = _div_roots(p, zs)
    ys = [pr.poly_eval(p, z) for z in zs]
    commit = pr.G1.mul(pr.poly_eval(p, TAU))
    proof = pr.G1.mul(pr.poly_eval(q, TAU))
    z_g2 = pr.G2.mul(pr.poly_eval(_vanishing(zs), TAU))
    pi_side = pairing.pair(proof, z_g2)  # the same in all three checks

    def r_tau(values):  # the interpolant of (z_j, values_j) at tau, Lagrange form
        ws = _weights(zs)
        zt = pr.poly_eval(_vanishing(zs), TAU)
        return sum(y * w % R * zt % R * pr.fr_inv((TAU - z) % R) for y, w, z in zip(values, ws, zs)) % R

    assert r_tau(ys) == pr.poly_eval(rem, TAU)
    assert _set_equation(commit, r_tau(ys), proof, z_g2, pi_side)
    assert not _set_equation(commit, r_tau([ys[0], (ys[1] + 1) % R, ys[2]]), proof, z_g2, pi_side)
    assert not _set_equation(commit, r_tau([ys[1], ys[0], ys[2]]), proof, z_g2, pi_side)


def test_at_one_point_the_equation_is_the_single_openings():
    """k = 1: r = y and Z_S = X - z, so e(C - y G1, G2) = e(pi, (tau - z) G2), which is ps_kzg_verify's
    e(C - y G1 + z pi, G2) = e(pi, tau G2) with e(pi, z G2) = e(z pi, G2) moved to the other side."""
    rng = pr.SplitMix64(0x9E4)
    p = [rng.fr() for _ in range(5)]
    z = rng.fr()
    q, y = _linear_quotient(p, z)
    assert _div_roots(p, [z]) == (q, [y])
    assert _weights([z]) == [1]
    commit, proof = pr.G1.mul(pr.poly_eval(p, TAU)), pr.G1.mul(pr.poly_eval(q, TAU))
    assert pr.G2.mul(pr.poly_eval(_vanishing([z]), TAU)) == pr.G2.add(pr.G2.mul(TAU), pr.G2.neg(pr.G2.mul(z)))
    set_lhs = pairing.pair(pr.G1.add(commit, pr.G1.neg(pr.G1.mul(y))), pr.G2.mul(1))
    set_rhs = pairing.pair(proof, pr.G2.mul((TAU - z) % R))
    single_lhs = pairing.pair(pr.G1.add(pr.G1.add(commit, pr.G1.neg(pr.G1.mul(y))), pr.G1.mul_pt(z, proof)), pr.G2.mul(1))
    single_rhs = pairing.pair(proof, pr.G2.mul(TAU))
    assert set_lhs == set_rhs and single_lhs == single_rhs
    # the two differ by the same factor e(pi, z G2) on both sides
    shift = pairing.pair(proof, pr.G2.mul(z))
    assert pairing.gt_mul(set_lhs, shift) == single_lhs and pairing.gt_mul(set_rhs, shift) == single_rhs
