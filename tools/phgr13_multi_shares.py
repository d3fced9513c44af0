"""PHGR13Prove at 2^20 constraints split over 8 ranks, on ONE GPU (reports only, not a gate):
  - each rank's ps_phgr13_prove_shard share alone, warmed, with its phase split (the whole key on the rank; the quotient in
    every share);
  - ps_phgr13_prove_multi over 8 contexts of the one GPU, each holding only its ranges of the key, with each context's phase
    split.  All contexts share one chip, so this is NOT an 8-GPU time: unmeasured on multiple GPUs.
Lagrange-form key (NewPHGR13TrustedSetup emits lgsi; MONOMIAL=1 drops it).  Writes profiles/phgr13_multi_2p20.txt, or the
path given as the first argument.
    python tools/phgr13_multi_shares.py [out.txt]          (LOG2N=20 WORLD=8 by default)"""
import os
import random
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from playsnark_amd import api  # noqa: E402
from playsnark_amd.dist import shard_range  # noqa: E402

FIELDS = api.PHGR13EvalKey.FIELDS
log2n = int(os.environ.get("LOG2N", "20"))
world = int(os.environ.get("WORLD", "8"))
reps = int(os.environ.get("REPS", "5"))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "phgr13_multi_2p%d.txt" % log2n)
lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


def phases(cx):
    return "  ".join("%s %.2f" % (k, v) for k, v in cx.last_prove_phase_ms().items())


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def same(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in api.PHGR13Proof.FIELDS)


n = 1 << log2n
ctx = api.Context(0)
nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
dsol = api.Poly.upload(ctx, sol)
rnd = random.Random(1)
ek, _ = api.NewPHGR13TrustedSetup(q, *[rnd.randrange(1 << 20, bench.R_MOD) for _ in range(8)])
if os.environ.get("MONOMIAL"):
    ek = ek.monomial_only()
form = "monomial key (gsi)" if ek.lgsi is None else "Lagrange-form key (lgsi)"
try:
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    head = "?"
out("# PHGR13Prove at 2^%d constraints (%d non-IO variables), %s, world %d, ONE MI355X%s" % (log2n, nvars - 3, form, world,
                                                                                            " (%s)" % head if head else ""))
out("# phases (ms, host wall clock, ps_prove_last_phase_ms): quotient = computing h -- on a device of the multi entry other than")
out("#   dev[0], waiting for h incl. the copy of its range --, prep_or_h_sum = the h(s) sum, sums = what is left of the solution")
out("#   sums after it, total")
out("# reference: ps_phgr13_prove on one GPU, 24.1-24.7 ms at 2^20 (profiles, round 4)")
out("")

for _ in range(2):
    whole = api.PHGR13Prove(ek, q, dsol)
ms = []
for _ in range(reps):
    _, t = timed(lambda: api.PHGR13Prove(ek, q, dsol))
    ms.append(t)
out("unsharded ps_phgr13_prove: median %.2f ms (min %.2f)   [%s]" % (statistics.median(ms), min(ms), phases(ctx)))
out("")

out("## ps_phgr13_prove_shard, each rank's share alone (whole key on the rank, the quotient in every share), warmed")
parts = []
for g in range(world):
    api.PHGR13ProveShard(ek, q, dsol, g, world)  # warm: view tables of this rank's ranges
    ms = []
    for _ in range(reps):
        p, t = timed(lambda: api.PHGR13ProveShard(ek, q, dsol, g, world))
        ms.append(t)
    parts.append(p)
    out("rank %d of %d: median %.2f ms (min %.2f)   [%s]" % (g, world, statistics.median(ms), min(ms), phases(ctx)))
folded = {f: api.points_sum(api.G2 if f == "wss" else api.G1, b"".join(getattr(p, f) for p in parts)) for f in api.PHGR13Proof.FIELDS}
assert all(folded[f] == getattr(whole, f) for f in api.PHGR13Proof.FIELDS), "folded shares differ from the unsharded proof"
out("folded shares == unsharded proof: yes")
out("")

raw = {f: getattr(ek, f).download() for f in FIELDS + (("lgsi",) if ek.lgsi is not None else ())}
ctxs = [ctx] + [api.Context(0) for _ in range(world - 1)]
devices = []
for d, cx in enumerate(ctxs):
    fields = {}
    for f, b in raw.items():
        nb = 192 if f == "ws" else 96
        first, cnt = shard_range(len(b) // nb, d, world)
        fields[f] = api.Points.upload(cx, api.G2 if f == "ws" else api.G1, b[first * nb:(first + cnt) * nb])
    devices.append((api.PHGR13EvalKey(**fields), api.QAP.from_csr(cx, nvars, nvars - 3, L, Rm, O), api.Poly.upload(cx, sol)))
del raw
out("## ps_phgr13_prove_multi over %d contexts of ONE GPU (rank-local keys) -- unmeasured on multiple GPUs: all contexts share one chip" % world)
for _ in range(2):
    got = api.PHGR13ProveMulti(devices)
assert same(got, whole), "multi proof differs from the unsharded proof"
ms = []
for _ in range(reps):
    got, t = timed(lambda: api.PHGR13ProveMulti(devices))
    ms.append(t)
assert same(got, whole)
out("multi, %d contexts on one GPU: median %.2f ms (min %.2f); == unsharded proof: yes" % (world, statistics.median(ms), min(ms)))
out("  (context 0's quotient phase is long here because the other contexts' solution sums run on the same chip meanwhile)")
for d, cx in enumerate(ctxs):
    out("  context %d (%s): [%s]" % (d, "quotient, then its sums" if d == 0 else "sums first, h copied in", phases(cx)))

os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", path)
