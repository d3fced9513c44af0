"""What a wrong guess of the point pass costs (csrc/point_pass_predict.hpp): the headline shape (2^20-point G1 sums over the
20-bit table, four in flight), a stream of uniform scalar vectors with ONE vector of bits in the middle.  The bits take the
slices, the history says whole buckets, so that sum's point pass runs twice.  Printed: the wall-clock interval between
consecutive finishes -- the mean over the undisturbed steps, and the intervals around the flip -- and the counters.
A library without the prediction (named by PLAYSNARK_HIP_LIB) runs the same stream with both passes enqueued every time:
the difference of the two totals is the cost of the flip less what the predicted launches save.
  python3 tools/point_pass_flip_cost.py          (GPU box; profiles/point_pass_prediction.txt)"""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bench
from playsnark_amd import api

ctx = api.Context(0)
n = 1 << 20
a = api.Poly.upload(ctx, bench.uniform_scalars_be32(n, 77).tobytes())
pts = api.Points.from_scalars(ctx, api.G1, a).precompute(0)
uni = api.Poly.upload(ctx, bench.uniform_scalars_be32(n, 78).tobytes())
bits = np.zeros((n, 32), dtype=np.uint8)
bits[:, 31] = np.random.RandomState(79).randint(0, 2, size=n)
bit = api.Poly.upload(ctx, bits.tobytes())
counts = getattr(ctx, "prediction_counts", None) if hasattr(api.lib, "ps_msm_prediction_counts") else None


def stream(pattern, depth=4):
    """finish times (ms from the start) of the sums of `pattern`, and their results"""
    todo, pending, stamps, outs = list(pattern), 0, [], []
    ctx.sync()
    t0 = time.perf_counter()
    while todo or pending:
        if todo and pending < depth:
            api.msm_launch(ctx, pts, uni if todo.pop(0) == "U" else bit)
            pending += 1
        else:
            outs.append(api.msm_finish(ctx, api.G1))
            stamps.append((time.perf_counter() - t0) * 1e3)
            pending -= 1
    return stamps, outs


stream("U" * 8)  # warm-up: workspaces, the history
for rnd in range(3):
    before = counts() if counts else None
    plain, ref = stream("U" * 33)
    flip, outs = stream("U" * 16 + "B" + "U" * 16)
    assert outs[:16] == ref[:16] and outs[17:] == ref[17:]
    d = np.diff(flip)
    step = float(np.mean(np.diff(plain)[4:]))
    print("round %d: undisturbed step %.3f ms (33 sums %.2f ms) | with one flip: 33 sums %.2f ms, intervals before the finishes of sums 15..22: %s" % (
        rnd + 1, step, plain[-1], flip[-1], " ".join("%.2f" % v for v in d[13:21])), flush=True)
    if counts:
        after = counts()
        print("         counters over both streams: " + ", ".join("%s +%d" % (k, after[k] - before[k]) for k in after), flush=True)
