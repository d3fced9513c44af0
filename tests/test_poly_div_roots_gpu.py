"""GPU: Poly.DivRoots (ps_poly_div_roots) -- quotient, values and remainder of a division by Z_S = prod (X - z_j) -- compared
word for word with the oracle's Poly.Div (pr.poly_div, highest-first order) up to 2T + 1 coefficients and, above that, with k
chained synthetic divisions written here and pinned to pr.poly_div at a small size.  T = ps_poly_scan_tile(), G =
ps_poly_scan_set_group(): the shapes sit on the edges of point groups (one group, a full one, a partial last one, the
reduce-every-32 step of the fold), on the cut of the top k - 1 coefficients (a tile's edge, a thread's edge, inside a thread's
items), on the empty quotient, and in the second chunk of the carry walk."""
import pytest

pytestmark = pytest.mark.gpu


def _tile():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_tile()


def _group():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_set_group()


T, G = _tile(), _group()


def _vanishing(pr, zs):
    zp = [1]
    for z in zs:
        zp = pr.poly_mul(zp, [(-z) % pr.R, 1])
    return zp


def _oracle(pr, p, zs):
    """(q, ys, rem), all lowest first: Poly.Div by Z_S in the reference's highest-first order, Poly.Eval"""
    k = len(zs)
    if len(p) <= k:
        return [], [pr.poly_eval(p, z) for z in zs], list(p) + [0] * (k - len(p))
    q, rem = pr.poly_div(p[::-1], _vanishing(pr, zs)[::-1])
    return q[::-1], [pr.poly_eval(p, z) for z in zs], rem[::-1]


def _chained(pr, p, zs):
    """The quotient by Z_S as k synthetic divisions by (X - z_j), one after the other, and the values p(z_j)."""
    R = pr.R
    ys = []
    for z in zs:
        h = 0
        for c in reversed(p):
            h = (c + z * h) % R
        ys.append(h)
    cur = list(p)
    for z in zs:
        h, out = 0, [0] * (len(cur) - 1)
        for i in range(len(cur) - 1, 0, -1):
            h = (cur[i] + z * h) % R
            out[i - 1] = h
        cur = out  # (the remainder of each step goes into the interpolant and is not needed for the quotient)
    return cur, ys


def _points(pr, rng, k, edge=False):
    zs = [rng.fr() for _ in range(k)]
    if edge:
        zs[: min(4, k)] = [0, 1, pr.R - 1, 2][: min(4, k)]
    assert len(set(zs)) == k
    return zs


def _check(ps_api, ctx, pr, p, zs, poly=None):
    poly = poly if poly is not None else ps_api.Poly.upload(ctx, p)
    q, ys, rem = poly.DivRoots(zs)
    wq, wys, wrem = _oracle(pr, p, zs)
    assert len(q) == len(wq) == max(len(p) - len(zs), 0)
    assert ys == wys
    assert rem == wrem
    got = q.download() if len(q) else []
    if got != wq:
        bad = [i for i, (a, b) in enumerate(zip(got, wq)) if a != b]
        raise AssertionError(f"n={len(p)} k={len(zs)}: {len(bad)} coefficients differ, first at {bad[0]}, last at {bad[-1]}")


@pytest.fixture(scope="module")
def base(ps_api, ctx, pr):
    """2T + 7 random coefficients, on the host and on the device: the tests take views of its head"""
    rng = pr.SplitMix64(0xD1F0)
    p = [rng.fr() for _ in range(2 * T + 7)]
    return p, ps_api.Poly.upload(ctx, p)


def test_the_chained_division_of_this_file_is_the_oracles(pr):
    rng = pr.SplitMix64(0xC4A1)
    p = [rng.fr() for _ in range(41)]
    zs = _points(pr, rng, 5, edge=True)
    q, ys, _ = _oracle(pr, p, zs)
    assert _chained(pr, p, zs) == (q, ys)


@pytest.mark.parametrize("k", sorted({1, 2, 3, G - 1, G, G + 1, 2 * G + 1, 33, 65} - {0}))
def test_quotient_values_and_remainder_are_the_oracles_at_two_tiles_and_one(ps_api, ctx, pr, base, k):
    p, poly = base
    n = 2 * T + 1
    rng = pr.SplitMix64(0xA000 + k)
    _check(ps_api, ctx, pr, p[:n], _points(pr, rng, k), poly.slice(0, n))


@pytest.mark.parametrize("k", sorted({3, G + 1}))
def test_the_cut_of_the_top_coefficients_on_a_tile_edge_a_thread_edge_and_inside_a_thread(ps_api, ctx, pr, base, k):
    """n - k in T - 1 .. T + 6: T - 1, T, T + 1 around the tile's edge, and every residue mod 8 of a thread's items"""
    p, poly = base
    rng = pr.SplitMix64(0xB000 + k)
    zs = _points(pr, rng, k)
    lens = list(range(T - 1, T + 7))
    assert {T - 1, T, T + 1} <= set(lens) and {v % 8 for v in lens} == set(range(8))
    for nq in lens:
        n = nq + k
        _check(ps_api, ctx, pr, p[:n], zs, poly.slice(0, n))


@pytest.mark.parametrize("k", sorted({3, G + 1}))
def test_short_polynomials_have_an_empty_quotient_and_are_their_own_remainder(ps_api, ctx, pr, base, k):
    p, poly = base
    rng = pr.SplitMix64(0xC000 + k)
    zs = _points(pr, rng, k)
    for n in (1, k - 1, k):
        q, ys, rem = poly.slice(0, n).DivRoots(zs)
        assert len(q) == 0 and rem == p[:n] + [0] * (k - n) and ys == [pr.poly_eval(p[:n], z) for z in zs]
    _check(ps_api, ctx, pr, p[: k + 1], zs, poly.slice(0, k + 1))  # one quotient coefficient: p's leading one
    q, _, _ = poly.slice(0, k + 1).DivRoots(zs)
    assert q.download() == [p[k]]


def test_the_second_chunk_of_the_carry_walk(ps_api, ctx, pr):
    """256 T + 1 coefficients, three points: scalars only, against the chained division"""
    n = 256 * T + 1
    rng = pr.SplitMix64(0xE001)
    p, v, c = [], rng.fr(), rng.fr()
    for _ in range(n):  # v -> v^2 + c: cheap, and without the structure a geometric sequence would have
        p.append(v)
        v = (v * v + c) % pr.R
    zs = _points(pr, rng, 3)
    q, ys, _ = ps_api.Poly.upload(ctx, p).DivRoots(zs)
    wq, wys = _chained(pr, p, zs)
    assert ys == wys
    assert len(q) == n - 3
    assert q.download() == wq


@pytest.mark.parametrize("k", sorted({4, G + 1, 33}))
def test_point_sets_that_hold_zero_one_minus_one_and_two(ps_api, ctx, pr, base, k):
    p, poly = base
    rng = pr.SplitMix64(0xF000 + k)
    n = T + 3
    _check(ps_api, ctx, pr, p[:n], _points(pr, rng, k, edge=True), poly.slice(0, n))


def test_thirty_three_consecutive_integers(ps_api, ctx, pr, base):
    p, poly = base
    n = T + 35
    _check(ps_api, ctx, pr, p[:n], list(range(5, 38)), poly.slice(0, n))
    _check(ps_api, ctx, pr, p[:n], [(pr.R - 16 + i) % pr.R for i in range(33)], poly.slice(0, n))  # ... across zero


def test_every_coefficient_r_minus_one_at_65_points(ps_api, ctx, pr):
    """the top of the lazy ranges: every loaded word is r - 1, and nine point groups meet in the fold"""
    n = 2 * T + 1
    rng = pr.SplitMix64(0xAB65)
    _check(ps_api, ctx, pr, [pr.R - 1] * n, _points(pr, rng, 65, edge=True))


def test_a_view_of_a_longer_vector(ps_api, ctx, pr, base):
    p, poly = base
    rng = pr.SplitMix64(0xAB66)
    zs = _points(pr, rng, G + 1)
    first, n = 5, T + 9
    _check(ps_api, ctx, pr, p[first : first + n], zs, poly.slice(first, n))
    # without the remainder (a NULL rem_be32): the same quotient and values
    q, ys, rem = poly.slice(first, n).DivRoots(zs, remainder=False)
    wq, wys, _ = _oracle(pr, p[first : first + n], zs)
    assert rem is None and ys == wys and q.download() == wq


def test_errors(ps_api, ctx, pr, base):
    p, poly = base
    small = poly.slice(0, 40)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # two equal points: both indices are named
        small.DivRoots([7, 9, 11, 9])
    assert e.value.code == -5 and "z[1]" in str(e.value) and "z[3]" in str(e.value)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # z = r is not canonical
        small.DivRoots([7, pr.R])
    assert e.value.code == -3
    with pytest.raises(ps_api.PlaysnarkError) as e:  # the empty set is not offered
        small.DivRoots([])
    assert e.value.code == -5
    with pytest.raises(ps_api.PlaysnarkError) as e:  # more than PS_KZG_SET_MAX points
        small.DivRoots(list(range(1025)))
    assert e.value.code == -5 and "1024" in str(e.value)
    q, ys, rem = small.DivRoots(list(range(1024)))  # the largest set: p is its own remainder
    assert len(q) == 0 and rem == p[:40] + [0] * (1024 - 40) and ys[:3] == [pr.poly_eval(p[:40], z) for z in range(3)]
