"""CPU: the identity behind the value-form set opening (playsnark_amd/csrc/poly_lagrange_set.hpp), in Python integers against
the oracle, for n <= 9 (pr.interpolate is cubic).  S = {z_0 .. z_{k-1}} distinct, c_j = 1 / prod_{l != j} (z_j - z_l),
y_j = p(z_j), e_{j,i} = 1 / (z_j - i), and q = (p - r) / Z_S the oracle's Poly.Div by Z_S:
  1. at a node i that no z_j equals:  q(i) = sum_j c_j (y_j - v_i) e_{j,i};
  2. at a node m = z_j*: the term of j* is c_j* q_m, q_m = (A - v_m B) / w_m the value of the single-point quotient at its own
     node (w the barycentric weights, A and B summed over i != m, tests/test_kzg_lagrange_identity.py), every other term as in 1;
  3. k >= n: q = 0 and the formula gives zero at every node;
  4. the proof scalar: sum_i q(i) l_i(tau) = q(tau), l_i(tau) from rs.lagrange_at, since deg q <= n - 1 - k.
Sets: every point off the domain (0, r - 1 and n + 1 among them), one hit, every point a node (k = n - 1 and k = n), a mix, and
more points than nodes.  This documents the formula; it holds with or without the device entry points."""
import math

import pytest

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
SIZES = [1, 2, 3, 5, 9]


def _weights(pr, n):
    return [(-1) ** (n - i) * pr.fr_inv(math.factorial(i - 1) * math.factorial(n - i) % pr.R) % pr.R for i in range(1, n + 1)]


def _q_m(pr, v, m):
    """the value at the node m of (p - v_m) / (X - m): (A - v_m B) / w_m over the nodes but m"""
    n, R = len(v), pr.R
    w = _weights(pr, n)
    A = B = 0
    for i in range(1, n + 1):
        if i != m:
            e = pr.fr_inv((m - i) % R)
            A = (A + w[i - 1] * v[i - 1] % R * e) % R
            B = (B + w[i - 1] * e) % R
    return (A - v[m - 1] * B) % R * pr.fr_inv(w[m - 1]) % R


def _set_weights(pr, zs):
    cs = []
    for j, zj in enumerate(zs):
        d = 1
        for l, zl in enumerate(zs):
            if l != j:
                d = d * (zj - zl) % pr.R
        cs.append(pr.fr_inv(d))
    return cs


def _formula(pr, v, p, zs):
    """the n values the fold computes, term by term"""
    n, R = len(v), pr.R
    cs = _set_weights(pr, zs)
    ys = [pr.poly_eval(p, z) for z in zs]
    row = []
    for i in range(1, n + 1):
        s = 0
        for c, y, z in zip(cs, ys, zs):
            if z == i:
                assert y == v[i - 1]
                s += c * _q_m(pr, v, i)
            else:
                s += c * (y - v[i - 1]) % R * pr.fr_inv((z - i) % R)
        row.append(s % R)
    return row


def _oracle_quotient(pr, p, zs):
    if len(p) <= len(zs):
        return []
    zp = [1]
    for z in zs:
        zp = pr.poly_mul(zp, [(-z) % pr.R, 1])
    q, _ = pr.poly_div(p[::-1], zp[::-1])
    return q[::-1]


def _sets(pr, n, rng):
    off = [0, pr.R - 1, n + 1, rng.fr(), rng.fr()]
    nodes = list(range(1, n + 1))
    sets = {
        "off": off,
        "one off": off[3:4],
        "one hit": off[:2] + [n] + off[2:],
        "a hit alone": [1],
        "every node but one": nodes[:-1],
        "every node": nodes,
        "mixed": [off[3], 1, 0, n, pr.R - 1] + nodes[1:-1:2],
        "more points than nodes": nodes + off[:2],
    }
    return {name: list(dict.fromkeys(zs)) for name, zs in sets.items() if zs}


@pytest.mark.parametrize("n", SIZES)
def test_the_fold_formula_gives_the_oracle_quotients_value_at_every_node(pr, n):
    from oracle import restate as rs

    rng = pr.SplitMix64(0x2EF + n)
    v = [rng.fr() for _ in range(n)]
    p = (pr.interpolate(v) + [0] * n)[:n]
    assert [pr.poly_eval(p, i) for i in range(1, n + 1)] == v
    lag = rs.lagrange_at(n, TAU)[0]
    for name, zs in _sets(pr, n, rng).items():
        q = _oracle_quotient(pr, p, zs)
        row = _formula(pr, v, p, zs)
        assert row == [pr.poly_eval(q, i) for i in range(1, n + 1)], (n, name)
        if len(zs) >= n:
            assert row == [0] * n, (n, name)
        assert sum(a * b for a, b in zip(row, lag)) % pr.R == pr.poly_eval(q, TAU), (n, name)
