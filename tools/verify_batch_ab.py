#!/usr/bin/env python3
"""A/B of the batch verifier against a loop of single verifications, on the same proofs, key and context:
    python tools/verify_batch_ab.py [--gates G] N [N ...]  >> profiles/verify_batch.txt
    PLAYSNARK_HIP_LIB=<another build> python tools/verify_batch_ab.py ...      (the same rows for a layout variant)
Baseline: ps_groth16_verify per proof (median over up to 64 of the proofs, warm context).  Candidate: one
ps_groth16_verify_batch over all N (median of 5 calls, warm), then one more call with the context's timing on for the split
by stage (the stream is drained at every stage boundary, so the split adds up to more than the untimed call):
  checks = key checks + upload + [r]P of A, B, C | scale = rho_i A_i | miller = k_miller_batch | prod = k_f12_product tree |
  sums = column sums + the two sums over points | host = download, three Miller loops, final exponentiation.
Proofs by ps_groth16_prove for a key made on the device; batches beyond 256 repeat 256 distinct proofs (the verifier's work
does not depend on whether proofs repeat).  The circuits declare const, x, out as IO, so by the reference's `diff`
convention the verifier's IO sum runs over nbVars - 3 points: at --gates 65536 the collapse of N full-length sums into one.
Bar: at N = 4096 the batch's time per proof is below a sixteenth of the baseline's."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, default=21)
    ap.add_argument("sizes", type=int, nargs="*", default=[1, 64, 1024, 4096, 65536])
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0xAB)
    c, sol = rs.synthetic_circuit(args.gates)
    diff = c.nbVars - c.nbIO
    q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    pk, vkd = api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
    dsol = api.Poly.upload(ctx, sol)
    ndist = min(256, max(args.sizes))
    distinct = [api.Groth16Prove(pk, q, dsol, rng.fr(), rng.fr()) for _ in range(ndist)]
    io1 = api.Poly.upload(ctx, sol[:diff])
    key = (pk.Alpha, pk.Beta2, vkd["Gamma"], pk.Delta2, vkd["IoLP"])
    mads = ctx.microbench_mad()
    print(f"# library {os.path.basename(_lib.library_path())}, {args.gates} gates, diff = {diff}; ps_microbench_mad {mads:.3e} lane multiply-adds/s")
    print("# N  single_us_per_proof  batch_ms  batch_us_per_proof  speedup  verdicts | timed call, ms: checks scale miller prod sums host | miller: us per loop, share of the multiply-add peak")
    io_row = b"".join(int(v).to_bytes(32, "big") for v in sol[:diff])
    for n in args.sizes:
        proofs = [distinct[i % ndist] for i in range(n)]
        ts = []
        for p in proofs[:64]:
            t = time.perf_counter()
            ok1 = api.Groth16Verify(ctx, *key, p, io1)
            ts.append(time.perf_counter() - t)
        single = statistics.median(ts)
        io = api.Poly.upload(ctx, io_row * n)
        rhos = [(rng.fr() >> 127) or 1 for _ in range(n)]
        api.Groth16VerifyBatch(ctx, *key, proofs, io, rhos)  # warm
        tb = []
        for _ in range(5):
            t = time.perf_counter()
            okb = api.Groth16VerifyBatch(ctx, *key, proofs, io, rhos)
            tb.append(time.perf_counter() - t)
        batch = statistics.median(tb)
        ctx.set_timing(True)
        api.Groth16VerifyBatch(ctx, *key, proofs, io, rhos)
        ctx.set_timing(False)
        ms = (C.c_float * 6)()
        _lib.lib.ps_debug_verify_batch_stage_ms(ctx._h, ms)
        # one loop is ~3 100 Fp2 products x 3 Fp products x 392 multiply-adds (the count of the issue, from pairing_body.inc)
        frac = n * 3100 * 3 * 392 / (ms[2] * 1e-3) / mads if ms[2] > 0 else 0.0
        print(f"{n:6d}  {single * 1e6:10.1f}  {batch * 1e3:10.2f}  {batch / n * 1e6:10.2f}  {single / (batch / n):8.1f}x  {ok1} {okb} | "
              + " ".join(f"{v:8.2f}" for v in ms) + f" | {ms[2] * 1e3 / n:9.2f} {frac:6.3f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
