#!/usr/bin/env python3
"""Times of ps_groth16_verify_batch_locate beside ps_groth16_verify_batch and the per-proof loop, on the same proofs, key
and context, in one process:
    python tools/verify_locate_times.py [--gates G] [--no-loop] [N ...]  > profiles/verify_locate.txt
For every N (default 64, 1024, 4096):
  b = 0   the plain batch call and the locating call ALTERNATED (--alternations pairs, warm): retaining the levels of the
          product tree is their only difference, so they should agree within the run-to-run spread of the plain call, which
          is printed (min .. max, and the median of both);
  b >= 1  (1 and 16, and N / 2 at N = 64) bad proofs -- the C of another proof -- at evenly spread positions: the locating
          call (median of 3), its checks and levels, the split of its descent from ps_debug_verify_locate_ms (trees: the C
          tree and the scalar tree, enqueued; device: the rounds' gathers, X_S, normalisation and download up to the
          synchronisation, which also waits for the trees; host: Miller loops and final exponentiations), the time per check
          below the root = (device + host) / (checks - 1), and ONE run of Groth16VerifyBatch(..., locate=True), which
          verifies proof by proof, for the ratio.
Proofs by ps_groth16_prove for a key made on the device; batches beyond 256 repeat 256 distinct proofs."""
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


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, default=21)
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--no-loop", action="store_true", help="skip the per-proof loop (13 s at N = 4096)")
    ap.add_argument("sizes", type=int, nargs="*", default=[64, 1024, 4096])
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x10CA7E)
    c, sol = rs.synthetic_circuit(args.gates)
    diff = c.nbVars - c.nbIO
    q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    pk, vkd = api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
    dsol = api.Poly.upload(ctx, sol)
    ndist = min(256, max(args.sizes))
    distinct = [api.Groth16Prove(pk, q, dsol, rng.fr(), rng.fr()) for _ in range(ndist)]
    key = (pk.Alpha, pk.Beta2, vkd["Gamma"], pk.Delta2, vkd["IoLP"])
    io_row = b"".join(int(v).to_bytes(32, "big") for v in sol[:diff])
    print(f"# library {os.path.basename(_lib.library_path())}, {args.gates} gates, diff = {diff}; times in ms, one process, warm context")
    ms = (C.c_float * 3)()
    for n in args.sizes:
        proofs = [distinct[i % ndist] for i in range(n)]
        io = api.Poly.upload(ctx, io_row * n)
        rhos = [(rng.fr() >> 127) or 1 for _ in range(n)]
        plain = lambda pf=proofs: api.Groth16VerifyBatch(ctx, *key, pf, io, rhos)
        locate = lambda pf=proofs: api.Groth16VerifyBatchLocate(ctx, *key, pf, io, rhos)
        plain(), locate()  # warm
        tp, tl = [], []
        for _ in range(args.alternations):
            t, ok = timed(plain)
            tp.append(t * 1e3)
            t, (bad, info) = timed(locate)
            tl.append(t * 1e3)
            assert ok is True and bad == [] and info["checks"] == 1
        print(f"N = {n:5d}  b = 0     plain  " + " ".join(f"{v:7.2f}" for v in tp) + f"   median {statistics.median(tp):7.2f}  spread {min(tp):.2f} .. {max(tp):.2f}")
        print(f"N = {n:5d}  b = 0     locate " + " ".join(f"{v:7.2f}" for v in tl) + f"   median {statistics.median(tl):7.2f}  checks 1 levels 0"
              f"   locate / plain {statistics.median(tl) / statistics.median(tp):.3f}")
        for b in [1, 16] + ([n // 2] if n == 64 else []):
            positions = sorted({(2 * k + 1) * n // (2 * b) for k in range(b)})
            assert len(positions) == b
            badp = list(proofs)
            for pos in positions:
                p, other = badp[pos], proofs[(pos + 1) % n]
                assert bytes(other.C) != bytes(p.C)
                badp[pos] = api.Groth16Proof(p.R, p.S, p.A, p.B, other.C)
            assert plain(badp) is False
            ts = []
            for _ in range(3):
                t, (bad, info) = timed(lambda: locate(badp))
                ts.append(t * 1e3)
                assert bad == positions, (bad, positions)
            _lib.lib.ps_debug_verify_locate_ms(ctx._h, ms)
            med = statistics.median(ts)
            per = (ms[1] + ms[2]) / max(1, info["checks"] - 1)
            row = (f"N = {n:5d}  b = {b:<4d}  locate {med:8.2f}  checks {info['checks']:4d} levels {info['levels']:2d}   descent: trees {ms[0]:6.2f} "
                   f"device {ms[1]:7.2f} host {ms[2]:7.2f}   per check {per:6.3f} (device {ms[1] / max(1, info['checks'] - 1):6.3f} host {ms[2] / max(1, info['checks'] - 1):6.3f})")
            if not args.no_loop:
                t, found = timed(lambda: api.Groth16VerifyBatch(ctx, *key, badp, io, rhos, locate=True))
                assert found == positions
                row += f"   loop {t * 1e3:9.1f}  loop / locate {t * 1e3 / med:6.1f}x"
            print(row, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
