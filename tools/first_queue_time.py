"""Wall clock of the first full queue of sums on a fresh context (it creates the worker workspaces), then of the second."""
import os, sys, time
sys.path.insert(0, os.getcwd())
import bench
from playsnark_amd import api, _lib
warm = api.Context(0)
n = 1 << 10
a = api.Poly.upload(warm, bench.uniform_scalars_be32(n, 1).tobytes())
pts = api.Points.from_scalars(warm, api.G1, a)
sc = api.Poly.upload(warm, bench.uniform_scalars_be32(n, 2).tobytes())
for _ in range(3):
    api.msm_launch(warm, pts, sc); api.msm_finish(warm, api.G1)
res = []
for rep in range(5):
    t0 = time.perf_counter()
    cx = api.Context(0)
    t1 = time.perf_counter()
    for _ in range(_lib.PS_MSM_QUEUE): api.msm_launch(cx, pts, sc)
    for _ in range(_lib.PS_MSM_QUEUE): api.msm_finish(cx, api.G1)
    t2 = time.perf_counter()
    for _ in range(_lib.PS_MSM_QUEUE): api.msm_launch(cx, pts, sc)
    for _ in range(_lib.PS_MSM_QUEUE): api.msm_finish(cx, api.G1)
    t3 = time.perf_counter()
    cx.close()
    res.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
print("fresh ctx: create / first full queue / second full queue ms:", " | ".join("%.2f %.2f %.2f" % r for r in res))
