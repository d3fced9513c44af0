"""CPU: the identities behind the value-form openings (playsnark_amd/csrc/poly_lagrange.hpp), in Python integers against the
oracle, for n <= 9 (pr.interpolate is cubic).  With w_i = (-1)^(n-i) / ((i-1)! (n-i)!) and e_i = 1 / (z - i):
  1. z off the domain: p(z) = P A with A = sum_i w_i v_i e_i and P = prod_i (z - i); and B = sum_i w_i e_i has B P = 1;
  2. the quotient values: q_i = (y - v_i) e_i at every node i != z are the values of (p - y) / (X - z);
  3. z = m on the domain: y = v_m and q_m = (A - v_m B) / w_m with A, B summed over i != m; 1 / w_m = +-(m-1)! (n-m)!;
  4. the proof scalar: sum_i q_i l_i(tau) = q(tau), l_i(tau) from rs.lagrange_at -- so the sum over the Lagrange-form string is
     the same group element as the coefficient route's.
Points: 0, r - 1, n + 1 and random ones off the domain; 1, n and the middle on it.  n = 1 needs no special case."""
import math

import pytest

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
SIZES = [1, 2, 5, 9]


def _weights(pr, n):
    return [(-1) ** (n - i) * pr.fr_inv(math.factorial(i - 1) * math.factorial(n - i) % pr.R) % pr.R for i in range(1, n + 1)]


def _sums(pr, v, z, skip=0):
    """(A, B, P) over the nodes but `skip`"""
    n, R = len(v), pr.R
    w = _weights(pr, n)
    A = B = 0
    P = 1
    for i in range(1, n + 1):
        if i == skip:
            continue
        e = pr.fr_inv((z - i) % R)
        A = (A + w[i - 1] * v[i - 1] % R * e) % R
        B = (B + w[i - 1] * e) % R
        P = P * (z - i) % R
    return A, B, P


def _quotient(pr, p, z):
    q, rem = pr.poly_div(p[::-1], [1, (-z) % pr.R])
    return q[::-1], rem[0]


def _case(pr, n):
    rng = pr.SplitMix64(0x1DE + n)
    v = [rng.fr() for _ in range(n)]
    p = (pr.interpolate(v) + [0] * n)[:n]
    assert [pr.poly_eval(p, i) for i in range(1, n + 1)] == v
    return rng, v, p


@pytest.mark.parametrize("n", SIZES)
def test_off_the_domain_the_value_is_P_times_A_and_B_times_P_is_one(pr, n):
    rng, v, p = _case(pr, n)
    for z in (0, pr.R - 1, n + 1, rng.fr(), rng.fr()):
        A, B, P = _sums(pr, v, z)
        assert P * A % pr.R == pr.poly_eval(p, z), (n, z)
        assert B * P % pr.R == 1, (n, z)


@pytest.mark.parametrize("n", SIZES)
def test_quotient_values_off_the_domain(pr, n):
    rng, v, p = _case(pr, n)
    for z in (0, pr.R - 1, n + 1, rng.fr()):
        q, y = _quotient(pr, p, z)
        assert y == pr.poly_eval(p, z) and len(q) == n - 1
        for i in range(1, n + 1):
            assert (y - v[i - 1]) * pr.fr_inv((z - i) % pr.R) % pr.R == pr.poly_eval(q, i), (n, z, i)


@pytest.mark.parametrize("n", SIZES)
def test_on_the_domain_the_missing_value_comes_from_the_degree_condition(pr, n):
    rng, v, p = _case(pr, n)
    w = _weights(pr, n)
    for m in sorted({1, n, (n + 1) // 2}):
        q, y = _quotient(pr, p, m)
        assert y == v[m - 1]
        for i in range(1, n + 1):
            if i != m:
                assert (y - v[i - 1]) * pr.fr_inv((m - i) % pr.R) % pr.R == pr.poly_eval(q, i), (n, m, i)
        A, B, _ = _sums(pr, v, m, skip=m)
        inv_w = (-1) ** (n - m) * math.factorial(m - 1) * math.factorial(n - m) % pr.R
        assert inv_w * w[m - 1] % pr.R == 1
        qm = (A - v[m - 1] * B) * inv_w % pr.R
        assert qm == pr.poly_eval(q, m), (n, m)
        # the condition itself: the values of a polynomial of degree <= n - 2 are orthogonal to the weights
        qs = [pr.poly_eval(q, i) for i in range(1, n + 1)]
        assert sum(wi * qi for wi, qi in zip(w, qs)) % pr.R == 0, (n, m)


def test_one_node_needs_no_special_case(pr):
    v = [0x1234567]
    for z in (0, 1, 2, pr.R - 1):
        if z == 1:
            A, B, _ = _sums(pr, v, 1, skip=1)
            assert (A, B) == (0, 0)
            y, q1 = v[0], (A - v[0] * B) % pr.R  # 1 / w_1 = 1
        else:
            A, B, P = _sums(pr, v, z)
            y = P * A % pr.R
            q1 = (y - v[0]) * pr.fr_inv((z - 1) % pr.R) % pr.R
        assert (y, q1) == (v[0], 0), z


@pytest.mark.parametrize("n", SIZES)
def test_the_proof_scalar_over_the_lagrange_basis_is_the_quotient_at_tau(pr, n):
    from oracle import restate as rs

    rng, v, p = _case(pr, n)
    basis, _ = rs.lagrange_at(n, TAU)
    assert sum(vi * li for vi, li in zip(v, basis)) % pr.R == pr.poly_eval(p, TAU)  # the commitment's scalar
    for z in (0, pr.R - 1, rng.fr(), 1, n, (n + 1) // 2):
        q, _ = _quotient(pr, p, z)
        qs = [pr.poly_eval(q, i) for i in range(1, n + 1)]
        assert sum(qi * li for qi, li in zip(qs, basis)) % pr.R == pr.poly_eval(q, TAU), (n, z)
