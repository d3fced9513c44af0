"""CPU: the identity behind the proofs of every node of the domain (playsnark_amd/csrc/kzg_all.hpp), in Python integers against
the oracle, with the group replaced by Fr (a point [a] G1 is the scalar a).  v_i = p(i), L_i = l_i(tau) from rs.lagrange_at,
w_i = (-1)^(n-i) / ((i-1)! (n-i)!), kappa(d) = 1 / d and kappa(0) = 0:
    pi_m = v_m K_m - U_m + g_m L_m,   U_m = sum_i kappa(m-i) v_i L_i,   K_m = sum_i kappa(m-i) L_i,
    s_m = sum_i kappa(m-i) w_i v_i,   c_m = sum_i kappa(m-i) w_i,       g_m = (s_m - v_m c_m) (-1)^(n-m) (m-1)! (n-m)!
is the oracle's Poly.Div of the interpolated polynomial by (X - m), evaluated at tau -- for every node of n = 1..9, 17 and 64.
The four sums are computed the way the device computes them: as cyclic convolutions of size S = 2^p >= 2n - 1 with the inputs
at the indices 0 .. n - 1 and kappa(d) at the index d mod S (the placement of kzg_all_plan.hpp, restated here); a literal double
loop pins the convolution.  kappa is antisymmetric, so the multiplier read backwards gives exactly the NEGATED sums: checked,
and checked that this is a different value.  1 / d is taken as (d-1)! (1/d!) as the device takes it.  This documents the formula;
it holds with or without the device entry points."""
import math

import pytest

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 64]


def _interpolate(pr, v):
    """coefficients, lowest first, of the polynomial with p(i) = v[i-1]: Newton's divided differences on 1..n (quadratic, where
    pr.interpolate is cubic; pinned against it for n <= 9 below)"""
    n, R = len(v), pr.R
    dd = list(v)
    for k in range(1, n):
        inv = pr.fr_inv(k)
        for i in range(n - 1, k - 1, -1):
            dd[i] = (dd[i] - dd[i - 1]) * inv % R
    p = [0] * n
    for k in range(n - 1, -1, -1):  # p = p (X - (k + 1)) + dd[k]
        p = [((p[i - 1] if i else 0) - (k + 1) * p[i]) % R for i in range(n)]
        p[0] = (p[0] + dd[k]) % R
    return p


def _plan(n):
    p = 0
    while (1 << p) < 2 * n - 1:
        p += 1
    return p, 1 << p


def _kappa_wrapped(pr, n, reverse=False):
    """kappa(d) at the index d mod S, |d| <= n - 1; reverse: the sequence read backwards, kappa(-d) there"""
    p, S = _plan(n)
    fact = [1] * (n + 1)
    for j in range(1, n + 1):
        fact[j] = fact[j - 1] * j % pr.R
    k = [0] * S
    for d in range(1, n):
        inv = fact[d - 1] * pr.fr_inv(fact[d]) % pr.R
        assert inv * d % pr.R == 1
        lo, hi = d % S, (-d) % S
        assert 1 <= lo <= n - 1 < hi <= S - 1  # positive and negative offsets never meet
        k[hi if reverse else lo] = inv
        k[lo if reverse else hi] = (-inv) % pr.R
    return k


def _cyclic(pr, x, k, n):
    """out[m-1] = sum_j k[(m-1-j) mod S] x[j], the first n entries of the cyclic convolution of the padded x with k"""
    S = len(k)
    xs = list(x) + [0] * (S - n)
    return [sum(k[(a - j) % S] * xs[j] for j in range(S)) % pr.R for a in range(n)]


def _all_proofs(pr, v, lag, reverse=False):
    """(pi, U, K) through the wrapped convolutions"""
    n, R = len(v), pr.R
    w = [(-1) ** (n - i) * pr.fr_inv(math.factorial(i - 1) * math.factorial(n - i) % R) % R for i in range(1, n + 1)]
    k = _kappa_wrapped(pr, n, reverse)
    U = _cyclic(pr, [a * b % R for a, b in zip(v, lag)], k, n)
    K = _cyclic(pr, lag, k, n)
    s = _cyclic(pr, [a * b % R for a, b in zip(w, v)], k, n)
    c = _cyclic(pr, w, k, n)
    pi = []
    for m in range(1, n + 1):
        inv_w = (-1) ** (n - m) * math.factorial(m - 1) * math.factorial(n - m) % R
        assert inv_w * w[m - 1] % R == 1
        g = (s[m - 1] - v[m - 1] * c[m - 1]) * inv_w % R
        pi.append((v[m - 1] * K[m - 1] - U[m - 1] + g * lag[m - 1]) % R)
    return pi, U, K


@pytest.mark.parametrize("n", SIZES)
def test_every_nodes_proof_scalar_is_the_oracle_quotient_at_tau(pr, n):
    from oracle import restate as rs

    rng = pr.SplitMix64(0xA11 + n)
    v = [rng.fr() for _ in range(n)]
    p = _interpolate(pr, v)
    if n <= 9:
        assert p == (pr.interpolate(v) + [0] * n)[:n]
    assert [pr.poly_eval(p, i) for i in range(1, n + 1)] == v
    lag = rs.lagrange_at(n, TAU)[0]
    assert sum(a * b for a, b in zip(v, lag)) % pr.R == pr.poly_eval(p, TAU)
    pi, U, K = _all_proofs(pr, v, lag)
    # the literal Toeplitz sums the convolutions stand for
    kap = lambda d: pr.fr_inv(d % pr.R) if d else 0
    assert U == [sum(kap(m - i) * v[i - 1] * lag[i - 1] for i in range(1, n + 1)) % pr.R for m in range(1, n + 1)]
    assert K == [sum(kap(m - i) * lag[i - 1] for i in range(1, n + 1)) % pr.R for m in range(1, n + 1)]
    for m in range(1, n + 1):
        if n == 1:
            want = 0
        else:
            q, rem = pr.poly_div(p[::-1], [1, (-m) % pr.R])
            assert rem == [v[m - 1]]
            want = pr.poly_eval(q[::-1], TAU)
            assert want == (pr.poly_eval(p, TAU) - v[m - 1]) * pr.fr_inv((TAU - m) % pr.R) % pr.R
        assert pi[m - 1] == want, (n, m)


@pytest.mark.parametrize("n", SIZES)
def test_the_multiplier_read_backwards_gives_the_negated_sums(pr, n):
    from oracle import restate as rs

    rng = pr.SplitMix64(0xA12 + n)
    v = [rng.fr() for _ in range(n)]
    lag = rs.lagrange_at(n, TAU)[0]
    pi, U, K = _all_proofs(pr, v, lag)
    bad, Ur, Kr = _all_proofs(pr, v, lag, reverse=True)
    assert Ur == [(-u) % pr.R for u in U] and Kr == [(-k) % pr.R for k in K]
    if n >= 2:
        assert Ur != U and Kr != K  # not an obviously wrong value: the same magnitude, the other sign
        assert bad != pi
        # with s and c negated too, g changes sign with them: every term but none survives -- the result is MINUS the proof
        assert bad == [(-x) % pr.R for x in pi]


def test_the_wrapped_placement_has_room_exactly_from_2n_minus_1_on(pr):
    for n in range(1, 70):
        p, S = _plan(n)
        assert S >= 2 * n - 1 and (p == 0 or (S >> 1) < 2 * n - 1)
        k = _kappa_wrapped(pr, n)
        assert k[0] == 0 and sum(1 for x in k if x) == 2 * (n - 1)
        assert all(k[t] == 0 for t in range(n, S - n + 1))
