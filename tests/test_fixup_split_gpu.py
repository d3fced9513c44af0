"""GPU parity of the long sums' fix-up in three kernels (msm.hpp section 5: k_fixup_classify, k_fixup_pair,
k_qfixup_chain, and the heavy-bucket kernels behind them) against the oracle, bit-exact on the affine bytes.

Which kernel sums a cut bucket depends on how many slices it touches, so every case runs over several slice lengths
(ctx.set_slice) and says, from ctx.last_msm_info(), why the shape it ran at reaches the path it is meant to cover:

  * all-equal scalars put exactly n entries into each of W buckets that follow one another in the sorted list, so with
    slices of M entries every bucket is cut once for n < M < 2n (pair kernel; W >= 3), touches 3 .. 8 slices for
    2M < n <= 6M (chain kernel) and 9 or more for n >= 9M (heavy kernels) -- exact, no statistics;
  * uniform scalars fill the buckets with entries / buckets on average; a bucket with more than k M entries touches more
    than k slices, so the mean fill against M tells which class dominates (pigeonhole: mean > k M guarantees one).

Sums of fewer than 2^21 digits are "short" and keep the one-kernel fix-up or the quad fix-up; ctx.set_tail(1) plans them
like long ones, which is how the small cases here reach the three kernels.  Both tail modes must give the oracle's bytes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x66697875
HEAVY_SPAN = 8  # msm.hpp / fixup_class.hpp


def _grp(ps_api, co, name):
    return (ps_api.G1, co.G1) if name == "g1" else (ps_api.G2, co.G2)


def _uniform_be32(n, seed):
    raw = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F  # < 2^254 < r
    return raw.tobytes()


_cache = {}


def _uniform_case(ps_api, ctx, co, name, log2n):
    """Points a_i G made on the device, uniform scalars, and the oracle's sum: computed once per (group, size)."""
    key = (name, log2n)
    if key not in _cache:
        gid, og = _grp(ps_api, co, name)
        n = 1 << log2n
        pts = ps_api.Points.from_scalars(ctx, gid, ps_api.Poly.upload(ctx, _uniform_be32(n, SEED + log2n)))
        sc = _uniform_be32(n, SEED + 100 + log2n)
        want = og.to_b(og.msm_pippenger(sc, pts.download(), n, 16))
        _cache[key] = (pts, ps_api.Poly.upload(ctx, sc), want)
    return _cache[key]


def _regime(info):
    """Slices an average bucket touches at least: ceil(mean fill / M)."""
    return info["entries"] / (info["buckets"] * info["slice"])


@pytest.mark.parametrize("log2n", [10, 16, 20])
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_uniform_scalars_table_and_plain_plan(ps_api, ctx, co, name, log2n):
    pts, dsc, want = _uniform_case(ps_api, ctx, co, name, log2n)
    n = 1 << log2n
    seen = set()
    try:
        for table in (False, True):
            if table:
                pts.precompute()
            ctx.set_slice(0)
            ctx.set_tail(1)
            assert dsc.BlindEval(pts) == want
            info = ctx.last_msm_info()
            assert info["window_table"] == int(table)
            fill = info["entries"] / info["buckets"]
            # slices of about the mean fill (buckets cut once or not at all), a third of it (three to eight slices) and
            # a tenth (nine and more): pair, chain and heavy buckets by the pigeonhole argument of the module docstring
            slices = sorted({max(1, round(fill)), max(1, int(fill / 3)), max(1, int(fill / 10))}, reverse=True)
            for tail in ((1,) if log2n == 20 else (1, 0)):
                for m in [0] + slices:
                    ctx.set_tail(tail)
                    ctx.set_slice(m)
                    assert dsc.BlindEval(pts) == want, (name, log2n, table, tail, m)
                    info = ctx.last_msm_info()
                    assert info["entries"] > n
                    if m:
                        assert info["slice"] == m
                    if tail == 1:
                        r = _regime(info)
                        seen.add("heavy" if r > HEAVY_SPAN else "chain" if r > 2 else "pair" if r > 0.25 else "whole")
            pts.drop_table()
    finally:
        ctx.set_slice(0)
        ctx.set_tail(0)
        pts.drop_table()
    if log2n == 20:  # 26 entries per bucket over the table (M = 26, 8, 2), 13 x 2^20 digits: the headline's shape
        assert {"pair", "chain", "heavy"} <= seen, seen
    else:
        assert "pair" in seen or "chain" in seen, seen


def _witness_values(n, seed):
    """int64 values as a circuit's witness holds them: a tenth zeros, a tenth ones, a quarter negative, 40 bits."""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 1 << 40, size=n, dtype=np.int64)
    kind = rs.randint(0, 20, size=n)
    w[kind < 2] = 0
    w[(kind >= 2) & (kind < 4)] = 1
    w[kind >= 15] *= -1
    return w


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_skewed_witness_scalars(ps_api, ctx, co, pr, name):
    """A tenth of the values are ones: one bucket of window 0 holds ~n / 10 entries, dozens of slices (heavy), beside
    thousands of buckets of a few entries."""
    gid, og = _grp(ps_api, co, name)
    n = 1 << 11
    vals = _witness_values(n, SEED + 7).tolist()
    raw = og.gen_points(12345 + n, 6789, n)
    pts = ps_api.Points.upload(ctx, gid, raw)
    want = og.to_b(og.blind_eval_i64(vals, raw))
    dsc = ps_api.Poly.from_values(ctx, vals)
    try:
        for tail in (1, 0):
            for m in (0, 16, 5, 2):
                ctx.set_tail(tail)
                ctx.set_slice(m)
                assert dsc.BlindEval(pts) == want, (name, tail, m)
                info = ctx.last_msm_info()
                if m:
                    assert info["slice"] == m
                    ones = sum(1 for v in vals if v == 1)
                    assert ones > (HEAVY_SPAN + 1) * m  # the bucket of digit 1 in window 0 is heavy at every forced slice
    finally:
        ctx.set_slice(0)
        ctx.set_tail(0)


def _neg(pr, name, P):
    return (P[0], (pr.P - P[1]) % pr.P) if name == "g1" else (P[0], ((-P[1][0]) % pr.P, (-P[1][1]) % pr.P))


@pytest.mark.parametrize("points", ["distinct", "repeated", "p_and_minus_p"])
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_equal_scalars_reach_pair_chain_and_heavy_exactly(ps_api, ctx, co, pr, name, points):
    """n equal scalars: W buckets of exactly n entries, one behind the other.  `repeated` makes every partial sum a
    multiple of one point (equal partial sums: the doubling branch of both adders); `p_and_minus_p` makes them cancel
    (identity partial sums and the P + (-P) branch)."""
    gid, og = _grp(ps_api, co, name)
    n = 100
    rng = pr.SplitMix64(SEED + 31)
    k = rng.fr()
    base = og.unpack(og.gen_points(rng.fr(), rng.fr(), n))
    P = base[0]
    if points == "repeated":
        base = [P] * n
    elif points == "p_and_minus_p":
        base = [P if i % 3 else _neg(pr, name, P) for i in range(n)]
    raw = og.pack(base)
    want = og.to_b(og.blind_eval([k] * n, raw))
    pts = ps_api.Points.upload(ctx, gid, raw)
    dsc = ps_api.Poly.upload(ctx, [k] * n)
    try:
        for tail in (1, 0):
            ctx.set_tail(tail)
            for m, path in ((150, "pair"), (101, "pair"), (30, "chain"), (17, "chain"), (11, "heavy"), (4, "heavy")):
                ctx.set_slice(m)
                assert dsc.BlindEval(pts) == want, (name, points, tail, m)
                info = ctx.last_msm_info()
                assert info["slice"] == m
                nonzero, rem = divmod(info["entries"], n)  # windows whose digit of k is not zero: a bucket of n entries each
                assert rem == 0 and nonzero >= 3
                if path == "pair":
                    assert n < m < 2 * n  # the boundary at M lies inside the second bucket, which no other boundary cuts
                elif path == "chain":
                    assert 2 * m < n <= (HEAVY_SPAN - 2) * m  # 3 .. 8 slices whatever the bucket's phase
                else:
                    assert n >= (HEAVY_SPAN + 1) * m  # 9 slices or more
    finally:
        ctx.set_slice(0)
        ctx.set_tail(0)
