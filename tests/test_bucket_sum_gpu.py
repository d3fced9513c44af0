"""GPU parity of the whole-bucket point pass (msm.hpp section 4b: k_bo_count / k_bo_scan / k_bo_place, k_bucket_sum)
against the slice path and against the oracle's CPU Pippenger, bit-exact on the affine bytes.

ctx.set_accumulate(2) forces the new pass for any shape, so the cases are the smallest at which it can still go wrong:
1 .. 4 097 points (one bucket per lane: fewer buckets than a wave, a wave, one more, several workgroups and ordering
tiles), windows of 4 and 8 bits on the plain plan (several bucket sets, buckets of hundreds of entries and of none) and one
array with a window table (one shared set, the window in the entry).  Inputs: uniform scalars; all-zero scalars (every bucket
empty: the pass must still write the identities); all-equal scalars (one huge bucket per window: slow but correct); one
point repeated (P + P inside the adder); P and -P (sums that cancel to the identity, and the copy of the first entry
followed by its negative); arrays with identity points (at the first entry of a bucket and later).

The automatic choice is checked at the smallest shape the host condition admits (2^17 points over 16-bit windows: 2^19
buckets, 4 entries each): uniform scalars must take whole buckets, boolean scalars the slices.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bucket_sum_cases import BUCKETS, SEED, SIZES, SLICES, _case, _grp, _uniform_be32  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["uniform", "zero", "equal", "repeated", "p_and_minus_p", "identities"])
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_whole_buckets_give_the_slices_bytes_and_the_oracles(ps_api, ctx, co, pr, name, kind):
    gid, og = _grp(ps_api, co, name)
    try:
        for n in SIZES:
            sc, raw = _case(og, pr, name, kind, n)
            want = og.to_b(og.msm_pippenger(sc, raw, n, 4))
            pts = ps_api.Points.upload(ctx, gid, raw)
            dsc = ps_api.Poly.upload(ctx, sc)
            # the plain plan with windows of 4 and 8 bits; then, at one size, the array's window table
            plans = [(4, False), (8, False)] + ([(0, True)] if n == 300 else [])
            for window, table in plans:
                ctx.set_window(window)
                if table:
                    pts.precompute()
                got = {}
                for mode in (SLICES, BUCKETS):
                    ctx.set_accumulate(mode)
                    got[mode] = dsc.BlindEval(pts)
                    assert ctx.last_accumulate_path() == mode, (name, kind, n, window, table)
                    info = ctx.last_msm_info()
                    assert info["window_table"] == int(table)
                    if not table:
                        assert info["window_bits"] == window and info["buckets"] == info["windows"] << (window - 1)
                assert got[SLICES] == got[BUCKETS], (name, kind, n, window, table)
                assert got[BUCKETS] == want, (name, kind, n, window, table)
                if table:
                    pts.drop_table()
    finally:
        ctx.set_window(0)
        ctx.set_accumulate(0)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_automatic_choice_at_the_smallest_admitted_shape(ps_api, ctx, co, name):
    """2^17 points, 16-bit windows: 16 sets of 2^15 buckets = 2^19 >= 2^18, 2^21 digits (a long sum), 4 per bucket.  Uniform
    scalars fill the buckets evenly and the device's verdict is whole buckets; boolean scalars put every entry into one
    bucket and the same launches take the slices.  Small sums stay on the slices whatever their fill."""
    gid, og = _grp(ps_api, co, name)
    n = 1 << 17
    pts = ps_api.Points.from_scalars(ctx, gid, ps_api.Poly.upload(ctx, _uniform_be32(n, SEED + 1)))
    raw = pts.download()
    uni = _uniform_be32(n, SEED + 2)
    bits = np.zeros((n, 32), dtype=np.uint8)
    bits[:, 31] = np.random.RandomState(SEED + 3).randint(0, 2, size=n)
    try:
        ctx.set_window(16)
        ctx.set_accumulate(0)
        for sc, path in ((uni, BUCKETS), (bits.tobytes(), SLICES)):
            got = ps_api.Poly.upload(ctx, sc).BlindEval(pts)
            info = ctx.last_msm_info()
            assert info["window_bits"] == 16 and info["buckets"] == 1 << 19, info
            assert ctx.last_accumulate_path() == path, (name, path, info)
            assert got == og.to_b(og.msm_pippenger(sc, raw, n, 16)), (name, path)
        ctx.set_window(0)
        m = 1 << 10  # a short sum: not admitted by the host, no ordering kernels, slices
        got = ps_api.Poly.upload(ctx, uni[: 32 * m]).BlindEval(pts.slice(0, m))
        assert ctx.last_accumulate_path() == SLICES
        assert got == og.to_b(og.msm_pippenger(uni[: 32 * m], raw[: m * og.nb], m, 4))
    finally:
        ctx.set_window(0)
        ctx.set_accumulate(0)
