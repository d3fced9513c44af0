"""Sums over COLLINEAR points through every tail a plan can choose.

The points are m_i P with m_i uniform in {-3 .. 3} (0: the identity) and P one oracle point per group, so the array holds at
most seven distinct encodings, every bucket is an integer multiple of P, and the expected result is ONE scalar multiplication:
(sum k_i m_i mod r) P.  With distinct random points (og.gen_points, every other sum test) no two partial sums are ever equal or
opposite; here they collide at every level of every tree and chain: the fix-up of cut buckets and the bucket reduction, on
lane quads (qtail.hpp: set_tail(2)) and one lane a point (k_fixup*, k_reduce_small / k_reduce_l1 / k_reduce_pyr / k_reduce_sum
at the window sizes tests/test_msm_gpu.py::test_window_size_does_not_change_the_result lists: set_tail(1)), behind both point
passes, and the fold of a batch (k_batch_fold).  tests/test_device_tail.py checks the same kernels value by value.

A CPU test keeps the input honest: a Python model of the signed digits gives every bucket's integer multiplier, and for every
(n, c) used below some buckets of a window are equal, some opposite, and some touched buckets sum to the identity."""
import collections
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bucket_sum_cases import _grp, _neg  # noqa: E402

SEED = 0x7461696C
SIZES = (300, 4097)
WINDOWS = (4, 7, 8, 13, 16)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MAX_BITS = 255  # capi.hip: the bound on uploaded big-endian scalars, from which a plan takes W = MAX_BITS / c + 1 windows


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (seeded: the same on every run)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multipliers(n, salt=0):
    return [int(v) for v in np.random.RandomState(SEED + 7 * n + salt).randint(-3, 4, size=n)]


@functools.lru_cache(maxsize=None)
def scalars(kind, n, salt=0):
    """uniform: below r.  wire: 0 / 1 values, every fifth scalar uniform."""
    raw = np.random.RandomState(SEED + 13 * n + salt).randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F  # < 2^254 < r
    ks = [int.from_bytes(bytes(row), "big") for row in raw]
    if kind == "wire":
        bits = np.random.RandomState(SEED + 17 * n + salt).randint(0, 2, size=n)
        ks = [k if i % 5 == 0 else int(bits[i]) for i, k in enumerate(ks)]
    else:
        assert kind == "uniform"
    return ks


def be32(ks):
    return b"".join(k.to_bytes(32, "big") for k in ks)


def signed_digits(k, c):
    """The digits the sort gives scalar k (msm.hpp, scalar_plus_c / digit_from): digit w is window w of k + C minus 2^(c - 1),
    C = sum over all windows but the top one of 2^(c - 1) 2^(c w); the top window is taken raw.  sum_w d_w 2^(c w) = k."""
    W = MAX_BITS // c + 1
    kp = k + sum(1 << (c * w + c - 1) for w in range(W - 1))
    out = [((kp >> (c * w)) & ((1 << c) - 1)) - (1 << (c - 1)) for w in range(W - 1)]
    out.append(kp >> (c * (W - 1)))
    return out


def bucket_multipliers(ks, ms, c):
    """per window {bucket: integer multiplier of P} over the touched buckets (bucket |d|, the point negated where d < 0)"""
    W = MAX_BITS // c + 1
    wins = [collections.defaultdict(int) for _ in range(W)]
    for k, m in zip(ks, ms):
        for w, d in enumerate(signed_digits(k, c)):
            if d:
                wins[w][abs(d)] += m if d > 0 else -m
    return wins


@pytest.mark.parametrize("kind", ["uniform", "wire"])
@pytest.mark.parametrize("n", SIZES)
def test_collinear_inputs_make_buckets_collide(n, kind):
    """The digit model recomposes every scalar, and at every window size used below the buckets of a window do collide:
    equal non-zero multipliers (the reduction doubles), opposite ones (it cancels), touched buckets that sum to zero (it
    meets the identity in a non-trivial representation)."""
    ks, ms = scalars(kind, n), multipliers(n)
    assert max(ks) < R and set(ms) == set(range(-3, 4))
    for c in WINDOWS:
        for k in ks[:50]:
            d = signed_digits(k, c)
            assert sum(v << (c * w) for w, v in enumerate(d)) == k and all(-(1 << (c - 1)) <= v < (1 << (c - 1)) for v in d[:-1])
            assert 0 <= d[-1] <= 1 << (c - 1), "the raw top window must fit the bucket set"
        equal = opposite = zero = 0
        for win in bucket_multipliers(ks, ms, c):
            cnt = collections.Counter(win.values())
            equal += sum(v * (v - 1) // 2 for m, v in cnt.items() if m != 0)
            opposite += sum(v * cnt[-m] for m, v in cnt.items() if m > 0)
            zero += cnt[0]
        assert equal >= 1 and opposite >= 1 and zero >= 1, (n, kind, c, equal, opposite, zero)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
_made = {}


def _base(og, pr, name):
    """P and the encodings of m P, -3 <= m <= 3, made once per group"""
    if name not in _made:
        base = og.mul(0x5DEECE66D if name == "g1" else 0x2545F4914F6CDD1D)
        enc, acc = {0: og.to_b(None)}, None
        for m in (1, 2, 3):
            acc = base if acc is None else og.add(acc, base)
            enc[m], enc[-m] = og.to_b(acc), og.to_b(_neg(pr, name, acc))
        _made[name] = (base, enc)
    return _made[name]


def _points(og, pr, name, ms):
    enc = _base(og, pr, name)[1]
    raw = b"".join(enc[m] for m in ms)
    assert len(set(raw[i:i + og.nb] for i in range(0, len(raw), og.nb))) <= 7
    return raw


def _want(og, pr, name, ks, ms):
    total = sum(k * m for k, m in zip(ks, ms)) % R
    return og.to_b(og.mul(total, _base(og, pr, name)[0]) if total else None)


def _reset(ctx):
    ctx.set_accumulate(0)
    ctx.set_window(0)
    ctx.set_slice(0)
    ctx.set_tail(0)
    ctx.set_batch_chunk(0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_collinear_sums_through_every_tail(ps_api, ctx, co, pr, name, n):
    """Forced windows 4, 7, 8, 13, 16; chains and trees behind the accumulation (set_tail 1 / 2); both point passes
    (set_accumulate 1 / 2); the automatic slices and slices of 2 entries on the uniform vector, the automatic ones on the
    wire values: every sum is the one scalar multiple of P."""
    gid, og = _grp(ps_api, co, name)
    ms = multipliers(n)
    pts = ps_api.Points.upload(ctx, gid, _points(og, pr, name, ms))
    runs = []
    for kind, slices in (("uniform", (0, 2)), ("wire", (0,))):
        ks = scalars(kind, n)
        runs.append((kind, slices, ps_api.Poly.upload(ctx, be32(ks)), _want(og, pr, name, ks, ms)))
    assert og.from_b(runs[0][3]) is not None
    try:
        for c in WINDOWS:
            ctx.set_window(c)
            for tail in (1, 2):
                ctx.set_tail(tail)
                for acc in (1, 2):
                    ctx.set_accumulate(acc)
                    for kind, slices, poly, want in runs:
                        for sl in slices:
                            ctx.set_slice(sl)
                            assert poly.BlindEval(pts) == want, (name, n, kind, c, tail, acc, sl)
                            assert ctx.last_accumulate_path() == acc and ctx.last_msm_info()["window_bits"] == c
    finally:
        _reset(ctx)


@pytest.mark.gpu
def test_collinear_sum_over_a_window_table(ps_api, ctx, co, pr):
    """precompute(0) at 4 097 points: one bucket set for all windows, every bucket a multiple of P, both tails and passes."""
    n, og = 4097, co.G1
    ms, ks = multipliers(n), scalars("uniform", n)
    pts = ps_api.Points.upload(ctx, ps_api.G1, _points(og, pr, "g1", ms)).precompute(0)
    poly = ps_api.Poly.upload(ctx, be32(ks))
    want = _want(og, pr, "g1", ks, ms)
    try:
        for tail in (1, 2):
            ctx.set_tail(tail)
            for acc in (1, 2):
                ctx.set_accumulate(acc)
                assert poly.BlindEval(pts) == want, (tail, acc)
                assert ctx.last_msm_info()["window_table"] == 1
    finally:
        _reset(ctx)
        pts.drop_table()


@pytest.mark.gpu
def test_collinear_multi_sum_over_both_groups(ps_api, ctx, co, pr):
    """ps_msm_multi over [G1, G2, G1], each array with multipliers of its own, one sort: the tail plan is shared by the
    groups (the quads of a G2 bucket must fit its 32-point block)."""
    n = 300
    ks = scalars("uniform", n)
    poly = ps_api.Poly.upload(ctx, be32(ks))
    arrays = [("g1", multipliers(n)), ("g2", multipliers(n, 1)), ("g1", multipliers(n, 2))]
    pts = [ps_api.Points.upload(ctx, _grp(ps_api, co, nm)[0], _points(_grp(ps_api, co, nm)[1], pr, nm, ms)) for nm, ms in arrays]
    want = [_want(_grp(ps_api, co, nm)[1], pr, nm, ks, ms) for nm, ms in arrays]
    assert len(set(want)) == 3
    try:
        for c in (0, 7, 13):
            ctx.set_window(c)
            for tail in (1, 2):
                ctx.set_tail(tail)
                assert ps_api.msm_multi(ctx, pts, poly) == want, (c, tail)
    finally:
        _reset(ctx)


@pytest.mark.gpu
def test_collinear_batch_of_three_members(ps_api, ctx, co, pr):
    """ps_msm_batch, three scalar vectors over one collinear array: the members' window sums are folded on the device
    (k_batch_fold) from buckets that are equal, opposite or the identity."""
    n, k, og = 300, 3, co.G1
    ms = multipliers(n)
    members = [scalars("uniform", n, 10 + j) for j in range(k - 1)] + [scalars("wire", n, 12)]
    pts = ps_api.Points.upload(ctx, ps_api.G1, _points(og, pr, "g1", ms))
    flat = ps_api.Poly.upload(ctx, b"".join(be32(m) for m in members))
    want = [_want(og, pr, "g1", m, ms) for m in members]
    try:
        for tail in (0, 1, 2):
            ctx.set_tail(tail)
            assert ps_api.msm_batch(ctx, pts, flat, k) == want, tail
    finally:
        _reset(ctx)
