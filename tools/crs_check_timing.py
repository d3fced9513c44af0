"""Wall time of checking a Groth16 key against its powers-of-tau string (ps_groth16_crs_check_from_srs) at 2^LOG2N constraints,
beside the parent's way of doing the same job: deriving the key again (ps_groth16_setup_from_srs) and comparing bytes.
The key is made from fixed toxic values (ps_groth16_setup) with one share folded in, the string from the same values
(ps_scalars_powers + ps_points_from_scalars).  The check is warmed once and timed REPS times, host clock around a call that
returns with its result; the derivation runs once (DERIVE=0 skips it).
  LOG2N=16 REPS=5 python3 tools/crs_check_timing.py"""
import os
import random
import sys
import time

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from playsnark_amd import api  # noqa: E402

log2n = int(os.environ.get("LOG2N", "16"))
reps = int(os.environ.get("REPS", "5"))
derive = os.environ.get("DERIVE", "1") != "0"
n = 1 << log2n
ctx = api.Context(0)
nvars, L, Rm, O, _sol = bench.synthetic_r1cs(n)
q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
rnd = random.Random(5)
fr = lambda: rnd.randrange(1 << 20, bench.R_MOD)
alpha, beta, x, d, g = fr(), fr(), fr(), fr(), fr()
pw = api.Poly.powers(ctx, x, 2 * n - 1)
srs = api.Groth16SRS(api.Points.from_scalars(ctx, api.G1, pw), api.Points.from_scalars(ctx, api.G2, pw.slice(0, n)),
                     api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, alpha)),
                     api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, beta)),
                     api.Points.from_scalars(ctx, api.G2, api.Poly.upload(ctx, [beta])).download())
k0 = api.NewGroth16TrustedSetup(q, alpha, beta, 1, x, 1)
key = api.Groth16Contribute(ctx, *k0, d, g)
rhos = [rnd.getrandbits(128) | 1 for _ in range(max(nvars, n))]
ctx.sync()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return out, time.perf_counter() - t0


tag = "n = 2^%d (%d variables)" % (log2n, nvars)
best = {}
for label, k, sub in (("Lagrange-form key, subgroup tests on", key, True), ("Lagrange-form key, subgroup tests off", key, False),
                      ("monomial-only key, subgroup tests off", (key[0].monomial_only(), key[1]), False)):
    check = lambda: api.Groth16CheckFromSRS(ctx, q, srs, k, rhos, check_subgroup=sub)
    ok, first = timed(check)
    assert ok, label
    ts = []
    for _ in range(reps):
        ok, dt = timed(check)
        assert ok
        ts.append(dt)
    best[label] = min(ts)
    print("%s  check, %s: first call %.1f ms, then min %.1f / median %.1f / max %.1f ms of %d" % (
        tag, label, 1e3 * first, 1e3 * min(ts), 1e3 * sorted(ts)[len(ts) // 2], 1e3 * max(ts), reps), flush=True)
# a rejected key costs no more: one NioLP point replaced
raw = bytearray(key[0].NioLP.download())
raw[-96:] = srs.TauG1.download(1, 1)
bad = api.Groth16Setup(key[0].Alpha, key[0].Beta, key[0].Delta, key[0].Beta2, key[0].Delta2, key[0].Xi, key[0].Xi2,
                       api.Points.upload(ctx, api.G1, bytes(raw)), key[0].XiT, key[0].LXi, key[0].LXi2, key[0].LXiT)
ok, dt = timed(lambda: api.Groth16CheckFromSRS(ctx, q, srs, (bad, key[1]), rhos))
assert not ok
print("%s  check of a key with one NioLP point replaced: rejected in %.1f ms" % (tag, 1e3 * dt), flush=True)
for mono, lagr, nodes, name in ((key[0].Xi, key[0].LXi, 0, "xi / lxi"), (key[0].Xi2, key[0].LXi2, 0, "xi2 / lxi2"),
                                (key[0].XiT, key[0].LXiT, 1, "xi_t / lxi_t")):
    mono.lagrange_check(q, lagr, rhos, nodes)
    ok, dt = timed(lambda: mono.lagrange_check(q, lagr, rhos, nodes))
    assert ok
    print("%s  ps_points_lagrange_check %s: %.1f ms" % (tag, name, 1e3 * dt), flush=True)
if derive:
    made, dt = timed(lambda: api.NewGroth16SetupFromSRS(q, srs))
    same = all(getattr(made[0], f).download() == getattr(k0[0], f).download() for f in ("NioLP", "XiT", "LXi", "LXiT"))
    assert same
    print("%s  ps_groth16_setup_from_srs (the derivation the check replaces; its byte comparison not included): %.2f s" % (tag, dt), flush=True)
    for label, t in best.items():
        print("%s  derivation / check (%s): %.0f x" % (tag, label, dt / t), flush=True)
