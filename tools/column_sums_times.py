"""Wall time of the column sums over points (ps_qap_column_sums for L, R and O), of the key from a powers-of-tau string
(ps_groth16_setup_from_srs) and of one Groth16 proof at 2^LOG2N gates, for two circuits in one process:
  * the tiled toy circuit of bench.py through the int64 entry (ps_qap_create): every coefficient is 1 or 5;
  * a MiMC-style circuit of 2^(LOG2N-1) rounds (tests/wide_circuits.py) through ps_qap_create_fr: every round constant is a
    full field element, so the `const` column holds 2^(LOG2N-1) wide entries in L and 2^LOG2N in R -- two long wide rows, each
    summed by one workgroup (csrc/ec_spmv.hpp).  Their cost alone is measured on a second QAP that keeps only that column.
Everything is warmed once and timed REPS times, host clock around a call that returns with its result; the median is quoted.
  LOG2N=16 REPS=5 python3 tools/column_sums_times.py           (MIMC=0: the int64 circuit only, for a library without the new entry)"""
import os
import random
import sys
import time

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from playsnark_amd import api  # noqa: E402

log2n = int(os.environ.get("LOG2N", "16"))
reps = int(os.environ.get("REPS", "5"))
mimc = os.environ.get("MIMC", "1") != "0"
tag = os.environ.get("TAG", "")
n = 1 << log2n
ctx = api.Context(0)
rnd = random.Random(5)
fr = lambda: rnd.randrange(1 << 20, bench.R_MOD)
alpha, beta, x = fr(), fr(), fr()
pw = api.Poly.powers(ctx, x, 2 * n - 1)
srs = api.Groth16SRS(api.Points.from_scalars(ctx, api.G1, pw), api.Points.from_scalars(ctx, api.G2, pw.slice(0, n)),
                     api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, alpha)),
                     api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, beta)),
                     api.Points.from_scalars(ctx, api.G2, api.Poly.upload(ctx, [beta])).download())
P = srs.TauG1.slice(0, n)  # any n points serve the column sums
ctx.sync()


def timed(fn):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def show(name, what, t):
    print("%s%s  n = 2^%d  %-46s median %9.2f ms  (min %.2f, max %.2f of %d)" % (tag and tag + "  ", name, log2n, what, t[0], t[1], t[2], reps), flush=True)


def measure(name, q, sol):
    out = {}
    sums = lambda: [q.column_sums(w, P) for w in range(3)]
    out["sums"] = timed(sums)
    show(name, "ps_qap_column_sums, L + R + O", out["sums"])
    for w, m in enumerate("LRO"):
        show(name, "ps_qap_column_sums, %s alone" % m, timed(lambda: q.column_sums(w, P)))
    out["setup"] = timed(lambda: api.NewGroth16SetupFromSRS(q, srs))
    show(name, "ps_groth16_setup_from_srs", out["setup"])
    print("%s%s  column sums / setup from the string: %.1f %%" % (tag and tag + "  ", name, 100 * out["sums"][0] / out["setup"][0]), flush=True)
    tr, _ = api.NewGroth16TrustedSetup(q, alpha, beta, fr(), x, fr())
    dsol = api.Poly.upload(ctx, sol)
    r, s = fr(), fr()
    api.Groth16Prove(tr, q, dsol, r, s)  # (builds the window tables)
    out["prove"] = timed(lambda: api.Groth16Prove(tr, q, dsol, r, s))
    show(name, "Groth16Prove", out["prove"])
    return out


nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
narrow = measure("int64 circuit", q, sol)
q.free()

if mimc:
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import wide_circuits as wc  # noqa: E402

    c, sol, cs = wc.mimc_circuit(n // 2)
    q = api.QAP.from_csr(ctx, c.nbVars, c.nbIO, *(wc.csr_fr(rows) for rows in (c.left, c.right, c.out)))
    print("MiMC circuit  wide entries (L, R, O):", q.wide_entries(), flush=True)
    wide = measure("MiMC circuit", q, sol)
    q.free()
    # the long wide rows alone: the same matrices with every column but `const` emptied
    only = lambda rows: [[(col, v) for col, v in row if col == 0] for row in rows]
    qc = api.QAP.from_csr(ctx, c.nbVars, c.nbIO, *(wc.csr_fr(only(rows)) for rows in (c.left, c.right, c.out)))
    long_rows = timed(lambda: [qc.column_sums(w, P) for w in (0, 1)])
    show("MiMC circuit", "the two long wide rows alone (L + R)", long_rows)
    # R's row as ONE sum of the library (ps_msm): both gates of round i multiply `const` by c_i, so the row is sum_g c_[g/2] P[g]
    sc = api.Poly.upload(ctx, [cs[g // 2] for g in range(n)])
    assert sc.BlindEval(P) == qc.column_sums(1, P).download(0, 1)
    show("MiMC circuit", "R's long wide row as one ps_msm over the gates", timed(lambda: sc.BlindEval(P)))
    rest = wide["sums"][0] - long_rows[0]
    print("MiMC circuit  long wide rows %.2f ms, all other work of the three column sums %.2f ms: %s" % (
        long_rows[0], rest, "the rows dominate" if long_rows[0] > rest else "the rows do not dominate"), flush=True)
    print("MiMC circuit / int64 circuit: column sums %.1f x, setup from the string %.2f x, proof %.2f x" % (
        wide["sums"][0] / narrow["sums"][0], wide["setup"][0] / narrow["setup"][0], wide["prove"][0] / narrow["prove"][0]), flush=True)
