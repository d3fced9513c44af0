"""Slices (1) against whole buckets (2) and the automatic mode (0) of ctx.set_accumulate, sums four in flight, over the shapes
the host thresholds of csrc/bucket_order.hpp separate and over skews the device threshold separates.  ms per step, three
interleaved rounds each; every mode must give the same bytes.
  python3 tools/accumulate_sweep.py [tag prefix ...]     (GPU box; profiles/bucket_order_ab.txt section 4)
The int64 witness row forces whole buckets onto one enormous bucket: seconds per sum -- leave it out with prefixes."""
import os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import bench
from playsnark_amd import api
from playsnark_amd.dist import ShardedMsm

ctx = api.Context(0)
only = sys.argv[1:]

def run(tag, gid, log2n, table, scal="uniform", skew=0, modes=(1, 2, 0), steps=20):
    if only and not any(tag.startswith(o) for o in only):
        return
    n = 1 << log2n
    a = api.Poly.upload(ctx, bench.uniform_scalars_be32(n, 77).tobytes())
    pts = api.Points.from_scalars(ctx, gid, a)
    if table:
        pts.precompute(0)
    if scal == "witness":
        sc = api.Poly.from_values(ctx, bench.witness_values(n, 5).tolist())
    else:
        h = bench.uniform_scalars_be32(n, 78).copy()
        if skew:
            h.reshape(n, 32)[:skew] = h.reshape(n, 32)[0]
        sc = api.Poly.upload(ctx, h.tobytes())
    m = ShardedMsm(ctx, gid, None, 1)
    res = {k: [] for k in modes}
    ref = None
    path = {}
    for rnd in range(3):
        for mode in modes:
            ctx.set_accumulate(mode)
            out = m.run_pipelined(pts, sc, 6, depth=4)
            ctx.sync()
            t0 = time.perf_counter()
            out = m.run_pipelined(pts, sc, steps, depth=4)
            res[mode].append((time.perf_counter() - t0) / steps * 1e3)
            path[mode] = ctx.last_accumulate_path()
            ref = ref or out
            assert out == ref, (tag, mode)
    info = ctx.last_msm_info()
    ctx.set_accumulate(0)
    print("%-34s G %8d mean %7.1f | " % (tag, info["buckets"], info["entries"] / info["buckets"]) +
          " | ".join("mode %d (path %d) %s" % (k, path[k], " ".join("%.3f" % v for v in res[k])) for k in modes), flush=True)
    pts.drop_table() if table else None
    pts.free(); sc.free(); a.free()

G1, G2 = api.G1, api.G2
run("g1 2^20 table (headline)", G1, 20, True)
run("g1 2^20 plain", G1, 20, False)
run("g2 2^20 table", G2, 20, True, steps=10)
run("g1 2^19 table", G1, 19, True)
run("g1 2^18 table", G1, 18, True)
run("g1 2^17 table", G1, 17, True)
run("g1 2^16 table", G1, 16, True)
run("g1 2^21 table", G1, 21, True)
run("g1 2^22 plain", G1, 22, False, steps=10)
run("g1 2^24 plain", G1, 24, False, steps=6)
run("g1 2^20 witness", G1, 20, True, scal="witness")
for s in (64, 96, 128, 192, 256, 1024, 16384):
    run("skew g1 2^20 table, bucket of +%d" % s, G1, 20, True, skew=s)
