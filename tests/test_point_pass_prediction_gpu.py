"""GPU: an admitted sum is launched with only the point pass the last sum of its kind took (point_pass_predict.hpp), and a
wrong guess is summed again -- the caller sees the oracle's bytes and the device's verdict whatever was guessed.

The shape is the smallest the host condition admits, the one test_bucket_sum_gpu.py uses: 2^17 points with 16-bit windows,
2^19 buckets.  Two scalar vectors over one point array: uniform scalars (U: the device says whole buckets) and a vector of
bits (B: slices).  Both are uploaded as 32-byte rows, so they are one kind of sum to the history.  Expected bytes: the oracle's
CPU Pippenger, once per vector and group.

Every pattern runs on a context of its own, so the history starts empty and the counters at zero.  With sums in flight the
driver launches while fewer than `depth` sums are pending and finishes the oldest otherwise, so a sum is launched knowing the
verdicts of all sums but the `depth - 1` before it.  The expected counters follow from the stated rule -- first sight: both
families; a history hit: one; a change of the verdict: both for the next PP_HOLD = 4 launches, started again by every further
change:
  U x 6, four in flight           sums 1-4 see no history (both), 5-6 are predicted            both 4, one 2, redone 0
  U U U U B U U U U, four in flight   1-4 both, 5-8 launched as U of which the B is redone while 6-8 are pending behind it
                                  (they are U and stay), 9 is launched after the change was seen   both 5, one 4, redone 1
  B B B U B B, one at a time      both, B, B, then U launched as B (redone), then the hold         both 3, one 3, redone 1
  U B U B U B U B, one at a time  both, then B launched as U (redone), then every sum renews the hold   both 7, one 1, redone 1
The sums over one sort (msm_multi: a G1 and a G2 array over one scalar vector) share one verdict and count as one sum:
  U U B B B B B B U               both, U, B launched as U (both arrays redone), four of the hold, B, U launched as B (redone)
                                                                                                   both 5, one 4, redone 2
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bucket_sum_cases import BUCKETS, SEED, SLICES, _grp, _uniform_be32  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1 << 17
WINDOW = 16
PATH = {"U": BUCKETS, "B": SLICES}

_inputs = {}


def _setup(ps_api, ctx, co, name):
    """(group id, points, {U, B: scalar bytes}, {U, B: expected bytes}), made once per group."""
    if name not in _inputs:
        gid, og = _grp(ps_api, co, name)
        pts = ps_api.Points.from_scalars(ctx, gid, ps_api.Poly.upload(ctx, _uniform_be32(N, SEED + 21)))
        raw = pts.download()
        bits = np.zeros((N, 32), dtype=np.uint8)
        bits[:, 31] = np.random.RandomState(SEED + 23).randint(0, 2, size=N)
        sc = {"U": _uniform_be32(N, SEED + 22), "B": bits.tobytes()}
        want = {k: og.to_b(og.msm_pippenger(v, raw, N, WINDOW)) for k, v in sc.items()}
        _inputs[name] = (gid, pts, sc, want)
    return _inputs[name]


def _run(ps_api, c, gid, pts, polys, want, pattern, depth):
    """The sums of `pattern` with at most `depth` pending; checks every result as it is finished."""
    pending = []
    todo = list(pattern)
    done = 0
    while todo or pending:
        if todo and len(pending) < depth:
            k = todo.pop(0)
            ps_api.msm_launch(c, pts, polys[k])
            pending.append(k)
        else:
            k = pending.pop(0)
            got = ps_api.msm_finish(c, gid)
            assert c.last_accumulate_path() == PATH[k], (pattern, done, k)
            assert got == want[k], (pattern, done, k)
            done += 1


CASES = [
    ("g1", "UUUUUU", 4, (4, 2, 0)),
    ("g2", "UUUUUU", 4, (4, 2, 0)),
    ("g1", "UUUUBUUUU", 4, (5, 4, 1)),
    ("g2", "UUUUBUUUU", 4, (5, 4, 1)),
    ("g1", "BBBUBB", 0, (3, 3, 1)),  # depth 0: one at a time through BlindEval
    ("g1", "UBUBUBUB", 1, (7, 1, 1)),
]


@pytest.mark.parametrize("name,pattern,depth,counts", CASES, ids=["%s-%s-%d" % c[:3] for c in CASES])
def test_predicted_point_pass_returns_the_oracles_bytes(ps_api, ctx, co, name, pattern, depth, counts):
    gid, pts, sc, want = _setup(ps_api, ctx, co, name)
    c = ps_api.Context(0)
    try:
        c.set_window(WINDOW)
        polys = {k: ps_api.Poly.upload(c, v) for k, v in sc.items()}
        assert c.prediction_counts() == {"both": 0, "one": 0, "redone": 0}
        if depth == 0:
            for i, k in enumerate(pattern):
                got = polys[k].BlindEval(pts)
                assert c.last_accumulate_path() == PATH[k], (pattern, i, k)
                assert got == want[k], (pattern, i, k)
        else:
            _run(ps_api, c, gid, pts, polys, want, pattern, depth)
        info = c.last_msm_info()
        assert info["window_bits"] == WINDOW and info["buckets"] == 1 << 19, info
        k = c.prediction_counts()
        assert (k["both"], k["one"], k["redone"]) == counts, (pattern, k)
        assert k["both"] + k["one"] == len(pattern)
    finally:
        c.close()


def test_sums_over_one_sort_are_predicted_and_redone_together(ps_api, ctx, co):
    g1 = _setup(ps_api, ctx, co, "g1")
    g2 = _setup(ps_api, ctx, co, "g2")
    assert g1[2] == g2[2]  # the same two scalar vectors
    c = ps_api.Context(0)
    try:
        c.set_window(WINDOW)
        polys = {k: ps_api.Poly.upload(c, v) for k, v in g1[2].items()}
        pattern = "UUBBBBBBU"
        for i, k in enumerate(pattern):
            got = ps_api.msm_multi(c, [g1[1], g2[1]], polys[k])
            assert c.last_accumulate_path() == PATH[k], (i, k)
            assert got == [g1[3][k], g2[3][k]], (i, k)
        assert c.prediction_counts() == {"both": 5, "one": 4, "redone": 2}
        # one array over the same sort is another kind of sum: nothing inherited
        assert ps_api.msm_multi(c, [g1[1]], polys["U"]) == [g1[3]["U"]]
        assert c.prediction_counts() == {"both": 6, "one": 4, "redone": 2}
    finally:
        c.close()


def test_forced_modes_and_sums_not_admitted_leave_the_counters_alone(ps_api, ctx, co):
    gid, pts, sc, want = _setup(ps_api, ctx, co, "g1")
    og = co.G1
    c = ps_api.Context(0)
    try:
        c.set_window(WINDOW)
        polys = {k: ps_api.Poly.upload(c, v) for k, v in sc.items()}
        _run(ps_api, c, gid, pts, polys, want, "UU", 1)  # a history exists: the forced modes must not consult it
        before = c.prediction_counts()
        assert before == {"both": 1, "one": 1, "redone": 0}
        for mode in (SLICES, BUCKETS):
            c.set_accumulate(mode)
            for k in "UBU":
                ps_api.msm_launch(c, pts, polys[k])
                got = ps_api.msm_finish(c, gid)
                assert c.last_accumulate_path() == mode and got == want[k], (mode, k)
            assert c.prediction_counts() == before, mode
        c.set_accumulate(0)
        c.set_window(0)
        m = 1 << 10  # a short sum: the host does not admit it
        short = sc["U"][: 32 * m]
        got = ps_api.Poly.upload(c, short).BlindEval(pts.slice(0, m))
        assert c.last_accumulate_path() == SLICES
        assert got == og.to_b(og.msm_pippenger(short, pts.download()[: m * og.nb], m, 4))
        assert c.prediction_counts() == before
        # ... and the automatic mode picks its history up again where it was
        c.set_window(WINDOW)
        assert polys["U"].BlindEval(pts) == want["U"]
        assert c.prediction_counts() == {"both": 1, "one": 2, "redone": 0}
    finally:
        c.close()
