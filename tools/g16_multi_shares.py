"""Groth16Prove at 2^20 constraints split over 8 ranks, on ONE GPU (reports only, not a gate):
  (a) unsharded ps_groth16_prove, Lagrange-form key;
  (b) each rank's ps_groth16_prove_shard share alone (the whole key on the rank, the quotient in every share);
  (c) each rank's ps_groth16_prove_local share alone (only its ranges of the Lagrange-form key on the rank), with its phases;
  (d) ps_groth16_prove_multi over 8 contexts of the one GPU, once with monomial and once with Lagrange-form rank-local keys,
      for PS_G16_MULTI_HSPLIT = 1 and 0.  All contexts share one chip, so the times inside (d) are NOT what 8 GPUs would give:
      unmeasured on multiple GPUs.
The one relation to hold: (d) with Lagrange-form keys beats (d) with monomial keys.  Legs whose entry points the library or the
Python layer do not have are skipped, so the same tool runs on a commit from before ps_groth16_prove_local.  Device memory
is what hipMemGetInfo reports as used by the process's device before and after a leg's keys, QAPs and tables exist.
Writes profiles/g16_multi_2p20.txt, or the path given as the first argument.
    python tools/g16_multi_shares.py [out.txt]          (LOG2N=20 WORLD=8 REPS=7 by default)"""
import ctypes
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

log2n = int(os.environ.get("LOG2N", "20"))
world = int(os.environ.get("WORLD", "8"))
reps = int(os.environ.get("REPS", "7"))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "g16_multi_2p%d.txt" % log2n)
lines = []
HAVE_LOCAL = hasattr(api, "Groth16ProveLocal") and hasattr(api.lib, "ps_groth16_prove_local")
hip = ctypes.CDLL("libamdhip64.so")


def out(s):
    print(s, flush=True)
    lines.append(s)


def used_gb():
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    return (total.value - free.value) / 2.0**30


def phases(cx):
    return "  ".join("%.2f" % v for v in cx.last_prove_phase_ms().values())


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def stats(f):
    for _ in range(2):
        r = f()
    ms = []
    for _ in range(reps):
        r, t = timed(f)
        ms.append(t)
    return r, statistics.median(ms), min(ms)


def abc(p):
    return (p.A, p.B, p.C) if hasattr(p, "A") else tuple(p)


def fold(parts):
    return (api.points_sum(api.G1, b"".join(p[0] for p in parts)), api.points_sum(api.G2, b"".join(p[1] for p in parts)),
            api.points_sum(api.G1, b"".join(p[2] for p in parts)))


n = 1 << log2n
ctx = api.Context(0)
nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
nio = nvars - 3
q = api.QAP.from_csr(ctx, nvars, nio, L, Rm, O)
dsol = api.Poly.upload(ctx, sol)
rnd = random.Random(1)
tox = [rnd.randrange(1 << 20, bench.R_MOD) for _ in range(5)]
r, s = rnd.randrange(1 << 20, bench.R_MOD), rnd.randrange(1 << 20, bench.R_MOD)
tr, _ = api.NewGroth16TrustedSetup(q, *tox)
try:
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
except OSError:
    head = "?"
out("# Groth16Prove at 2^%d constraints (%d non-IO variables), world %d, ONE MI355X%s" % (log2n, nio, world, " (%s)" % head if head else ""))
out("# times: host wall clock, median (min) of %d warmed proofs in one process.  phases (ms, ps_prove_last_phase_ms) of a share over" % reps)
out("#   rank-local Lagrange-form keys: own rows + values route on this device + wait for h | the h sum | the other sums | total")
out("# ps_groth16_prove_local in this library: %s" % ("yes" if HAVE_LOCAL else "no (legs c and d-Lagrange skipped)"))
out("")

whole, med, mn = stats(lambda: api.Groth16Prove(tr, q, dsol, r, s))
want = abc(whole)
out("(a) unsharded ps_groth16_prove, Lagrange-form key: median %.2f ms (min %.2f)   [%s]" % (med, mn, phases(ctx)))
out("")

out("## (b) ps_groth16_prove_shard, each rank's share alone (whole key on the rank, the quotient in every share)")
from playsnark_amd.dist import ShardedGroth16  # noqa: E402

sh = ShardedGroth16(ctx, None, world, 0)
parts = []
for g in range(world):
    p, med, mn = stats(lambda: sh.partials(tr, q, dsol, r, s, rank=g))
    parts.append(p)
    out("rank %d of %d: median %.2f ms (min %.2f)" % (g, world, med, mn))
assert fold(parts) == want, "folded shares differ from the unsharded proof"
out("folded shares == unsharded proof: yes;  device memory with the whole key, its tables and one QAP: %.1f GB" % used_gb())
out("")

NAMES = ("Xi", "Xi2", "XiT", "LXi", "LXi2", "LXiT", "NioLP")
raw = {f: getattr(tr, f).download() for f in NAMES}
fixed = [tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2]
del tr, sh, parts


def local_key(cx, d, lagrange):
    def part(f):
        nb = 192 if f.endswith("Xi2") else 96
        first, cnt = shard_range(len(raw[f]) // nb, d, world)
        return api.Points.upload(cx, api.G2 if nb == 192 else api.G1, raw[f][first * nb:(first + cnt) * nb])

    if lagrange:
        return api.Groth16Setup(*fixed, None, None, part("NioLP"), None, part("LXi"), part("LXi2"), part("LXiT"))
    return api.Groth16Setup(*fixed, part("Xi"), part("Xi2"), part("NioLP"), part("XiT"))


def contexts(hsplit):
    os.environ["PS_G16_MULTI_HSPLIT"] = hsplit  # read by ps_ctx_create
    cxs = [api.Context(0) for _ in range(world)]
    del os.environ["PS_G16_MULTI_HSPLIT"]
    return cxs


results = {}
for hsplit in ("1", "0"):
    cxs = contexts(hsplit)
    qaps = [api.QAP.from_csr(cx, nvars, nio, L, Rm, O) for cx in cxs]
    sols = [api.Poly.upload(cx, sol) for cx in cxs]
    for lagrange in ((False, True) if HAVE_LOCAL else (False,)):
        if not lagrange and hsplit == "0":
            continue  # the knob does not reach the monomial route
        before = used_gb()
        devices = [(local_key(cx, d, lagrange), qaps[d], sols[d]) for d, cx in enumerate(cxs)]
        form = "Lagrange-form" if lagrange else "monomial"
        if lagrange and hsplit == "1":
            out("## (c) ps_groth16_prove_local, each rank's share alone (only its ranges of the key on the rank; the values route in every share)")
            parts = []
            for g, (k, qq, ds) in enumerate(devices):
                p, med, mn = stats(lambda: api.Groth16ProveLocal(k, qq, ds, r, s, g, world))
                parts.append(p)
                out("rank %d of %d: median %.2f ms (min %.2f)   [%s]" % (g, world, med, mn, phases(cxs[g])))
            assert fold(parts) == want, "folded local shares differ from the unsharded proof"
            out("folded shares == unsharded proof: yes;  device memory per rank (its ranges, their tables): %.2f GB" % ((used_gb() - before) / world))
            out("  critical path on 8 GPUs, from pieces measured alone: a share above is its UPPER bound -- it holds all three")
            out("  convolutions of the values route where a device of the multi entry runs one (or none) and copies 3 x 40 B per node;")
            out("  the one-convolution piece alone is not exposed by the library and is unmeasured.  Aspiration: <= 4.5 ms (VERDICT.md).")
            out("")
        got, med, mn = stats(lambda: api.Groth16ProveMulti(devices, r, s))
        assert abc(got) == want, "multi proof differs from the unsharded proof"
        results[(form, hsplit)] = med
        out("## (d) ps_groth16_prove_multi over %d contexts of ONE GPU, %s rank-local keys%s -- unmeasured on multiple GPUs" %
            (world, form, ", PS_G16_MULTI_HSPLIT=" + hsplit if lagrange else ""))
        out("multi: median %.2f ms (min %.2f); == unsharded proof: yes" % (med, mn))
        if lagrange:
            for d, cx in enumerate(cxs):
                out("  context %d: [%s]" % (d, phases(cx)))
        out("")
        del devices
    del qaps, sols
    for cx in cxs:
        cx.close()

mono = results.get(("monomial", "1"))
for hsplit in ("1", "0"):
    lag = results.get(("Lagrange-form", hsplit))
    if mono and lag:
        out("(d) monomial / Lagrange-form, PS_G16_MULTI_HSPLIT=%s: %.2f / %.2f ms = %.2f x (must be a clear win; below 1.5 x needs an explanation)" %
            (hsplit, mono, lag, mono / lag))

os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("wrote", path)
