"""GPU: ps_poly_eval and ps_poly_div_linear (playsnark_amd/csrc/poly_scan.hpp), byte for byte against the oracle --
oracle.pyref.poly_eval, and oracle.pyref.poly_div called as the reference calls it: highest degree first, divisor [1, -z].
Sizes sit on the edges of a wave, of a workgroup's threads and of the scan's tile T = ps_poly_scan_tile() (read at run time),
once on the second chunk of the carry walk (256 T + 1); points among 0, 1, r - 1, random values and a root of p; coefficients
random, all r - 1, only the top one non-zero (tile totals of zero under a non-zero carry) and only the constant non-zero."""
import random

import pytest

pytestmark = pytest.mark.gpu


def _tile():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_tile()


def _sizes():
    T = _tile()
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]


def _oracle_div(pr, p, z):
    """(quotient lowest degree first, remainder) of p by (X - z), through Poly.Div (algebra.go:119-137)."""
    q, rem = pr.poly_div(p[::-1], [1, (-z) % pr.R])
    assert len(rem) == 1
    return q[::-1], rem[0]


def _kinds(pr, rng, n):
    top = [0] * n
    top[-1] = rng.fr() or 1
    const = [0] * n
    const[0] = rng.fr() or 1
    return {"random": [rng.fr() for _ in range(n)], "all r-1": [pr.R - 1] * n, "top only": top, "constant only": const}


def _check(ps_api, pr, ctx, coeffs, poly, zs, cache):
    """Eval and DivLinear of `poly` (the device copy of `coeffs`) at zs against the oracle; cache: z -> (q, y)."""
    n = len(coeffs)
    for z in zs:
        if z not in cache:
            cache[z] = _oracle_div(pr, coeffs, z) if n >= 2 else ([], coeffs[0])
            assert cache[z][1] == pr.poly_eval(coeffs, z)
    want_y = [cache[z][1] for z in zs]
    assert poly.Eval(zs) == want_y
    if n < 2:
        return
    q, rems = poly.DivLinear(zs)
    assert rems == want_y
    assert len(q) == len(zs) * (n - 1)
    got = q.download()
    for j, z in enumerate(zs):
        assert got[j * (n - 1) : (j + 1) * (n - 1)] == cache[z][0], (n, j)


@pytest.mark.parametrize("n", _sizes())
def test_values_and_quotients_match_the_oracle(ps_api, ctx, pr, n):
    rng = pr.SplitMix64(0xD1 + n)
    for kind, coeffs in _kinds(pr, rng, n).items():
        poly = ps_api.Poly.upload(ctx, coeffs)
        cache = {}
        for zs in ([rng.fr()], [0, pr.R - 1], [0, 1, pr.R - 1, rng.fr(), rng.fr()]):  # k = 1, 2, 5
            _check(ps_api, pr, ctx, coeffs, poly, zs, cache)


@pytest.mark.parametrize("n", [s for s in _sizes() if s >= 2])
def test_a_root_leaves_no_remainder_and_gives_back_the_cofactor(ps_api, ctx, pr, n):
    """p = (X - z) s(X), built on the device with Poly.Mul: the remainder at z is zero and the quotient is s; the other four
    points of the same call are checked against the oracle on the downloaded product."""
    rng = pr.SplitMix64(0xA7 + n)
    z = rng.fr()
    s = [rng.fr() for _ in range(n - 1)]
    poly = ps_api.Poly.upload(ctx, [(-z) % pr.R, 1]).Mul(ps_api.Poly.upload(ctx, s))
    coeffs = poly.download()
    assert coeffs == pr.poly_mul([(-z) % pr.R, 1], s) and len(coeffs) == n
    zs = [0, 1, pr.R - 1, rng.fr(), z]
    q, rems = poly.DivLinear(zs)
    assert rems[4] == 0 and poly.Eval([z]) == [0]
    assert q.download(4 * (n - 1), n - 1) == s
    _check(ps_api, pr, ctx, coeffs, poly, zs, {})


def test_the_second_chunk_of_the_carry_walk(ps_api, ctx, pr):
    """256 T + 1 coefficients are 257 tiles: the carry walk scans a chunk of one tile, then a full chunk with a carry coming in."""
    n = 256 * _tile() + 1
    raw = random.Random(20).randbytes(32 * n)
    coeffs = [int.from_bytes(raw[32 * i : 32 * i + 32], "big") % pr.R for i in range(n)]
    poly = ps_api.Poly.upload(ctx, coeffs)
    z = pr.SplitMix64(77).fr()
    want_q, want_y = _oracle_div(pr, coeffs, z)
    assert want_y == pr.poly_eval(coeffs, z)
    assert poly.Eval([z]) == [want_y]
    q, rems = poly.DivLinear([z])
    assert rems == [want_y]
    assert q.download() == want_q


def test_argument_checks_return_before_any_launch(ps_api, ctx, pr):
    poly = ps_api.Poly.upload(ctx, [3, 1, 4])
    for call in (lambda: poly.Eval([pr.R]), lambda: poly.DivLinear([1, pr.R]), lambda: poly.Eval([1, 2**256 - 1])):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            call()
        assert e.value.code == -3  # PS_ERR_ENCODING
    const = ps_api.Poly.upload(ctx, [5])
    with pytest.raises(ps_api.LengthMismatch):  # no quotient to hold
        const.DivLinear([2])
    assert const.Eval([2, 0]) == [5, 5]
    with pytest.raises(ps_api.LengthMismatch):  # an empty polynomial
        poly.slice(0, 0).Eval([1])
    assert poly.Eval([]) == []  # k = 0
    q, rems = poly.DivLinear([])
    assert len(q) == 0 and rems == []


def test_a_view_gives_the_answer_of_its_own_coefficients(ps_api, ctx, pr):
    T = _tile()
    rng = pr.SplitMix64(0x51)
    whole = [rng.fr() for _ in range(T + 40)]
    poly = ps_api.Poly.upload(ctx, whole)
    for first, n in ((3, T + 1), (T - 1, 5), (1, 1)):
        view = poly.slice(first, n)
        _check(ps_api, pr, ctx, whole[first : first + n], view, [rng.fr(), 1], {})
