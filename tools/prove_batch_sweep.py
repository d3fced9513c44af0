#!/usr/bin/env python3
"""The batch prover and the batched sum against loops of single calls, in one process, on the same key and context:
    python tools/prove_batch_sweep.py [--log2n 10 12 14 16] [--k 1 8 64 256] [--reps 5]  > profiles/prove_batch.txt
Per (n, K), warm, `reps` repetitions each, batch and loop alternating; reported: the median and (min .. max), wall clock around
calls that end in a device synchronise.
  prove   ps_groth16_prove_batch of K witnesses, ms per proof, against a loop of ps_groth16_prove over min(K, 64) of them
          (the loop is what the library offered before the batch: the single prover is untouched); then ONE more batch call
          with the context's timing on, for the device-time split of the batch (events on the context stream):
            wires = witness conversion, K-column SpMV, gate check and the scalar rows | hvals = the K runs of quotient_h_values |
            B, A, C = the three batched sums, and of the LAST pass of the sum C: sort | acc | tail (fix-up + reduction) | fold
            (k_batch_fold, k_batch_to_affine, encoding)
  msm     ps_msm_batch of K vectors of n uniform 254-bit scalars over n points, G1 and G2, ms per member, against a loop of
          ps_msm over slices (min(K, 64) members)
--modes M [M ...]: ps_msm_batch_set_table modes of the batch (0 automatic, 1 never over window tables -- the plain pass --, 2
wherever a table is usable), alternated with each other and with the loop inside every repetition; one column set per mode.
`--modes 1 0` is the A/B of the tabled pass (profiles/prove_batch_table.txt); `--tables` precomputes the automatic window
table on the points of the msm rows (the provers' keys carry theirs anyway).
Witnesses: the tiled synthetic circuit with up to 8 values of x0, repeated to K (the work does not depend on whether
witnesses repeat: every member has its own bucket sets)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402

LOOP_MAX = 64


def _timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _set_mode(ctx, mode):
    """ps_msm_batch_set_table; an older build named by PLAYSNARK_HIP_LIB has no such entry and only the plain pass (mode 1)."""
    if hasattr(_lib.lib, "ps_msm_batch_set_table"):
        ctx.set_batch_table(mode)
    elif mode != 1:
        raise SystemExit("this library build has no ps_msm_batch_set_table: --modes 1 only")


def _stat(v):
    return f"{statistics.median(v):9.4f} ({min(v):.4f} .. {max(v):.4f})"


def _ab(ctx, modes, batch, loop, reps):
    """{mode: times of the batch}, times of the loop: every repetition runs the batch once per mode, then the loop."""
    tb, tl = {m: [] for m in modes}, []
    for rep in range(reps + 1):  # the first round is the warm-up: buffers sized, code objects loaded, tables built
        for m in modes:
            _set_mode(ctx, m)
            t = _timed(batch)
            if rep:
                tb[m].append(t)
        t = _timed(loop)
        if rep:
            tl.append(t)
    return tb, tl


def prove_rows(ctx, rng, log2n, ks, reps, modes):
    n = 1 << log2n
    distinct = min(8, max(ks))
    made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(distinct)]
    c = made[0][0]
    q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, _ = api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
    rows = [b"".join(int(v).to_bytes(32, "big") for v in sol) for _, sol in made]
    singles = [api.Poly.upload(ctx, r) for r in rows]
    for k in ks:
        sols = api.Poly.upload(ctx, b"".join(rows[j % distinct] for j in range(k)))
        rr, ss = [rng.fr() for _ in range(k)], [rng.fr() for _ in range(k)]
        kl = min(k, LOOP_MAX)
        out = {}

        def batch():
            out["b"] = api.Groth16ProveBatch(tr, q, sols, rr, ss)

        def loop():
            out["l"] = [api.Groth16Prove(tr, q, singles[j % distinct], rr[j], ss[j]) for j in range(kl)]

        tb, tl = _ab(ctx, modes, batch, loop, reps)
        pl = [t / kl for t in tl]
        for mode in modes:
            _set_mode(ctx, mode)
            ctx.set_timing(True)
            batch()
            same = all((out["b"][j].A, out["b"][j].B, out["b"][j].C) == (out["l"][j].A, out["l"][j].B, out["l"][j].C) for j in range(kl))
            ms = (C.c_float * 6)()
            _lib.lib.ps_debug_batch_stage_ms(ctx._h, ms)
            st = ctx.last_stage_ms()
            ctx.set_timing(False)
            info = ctx.last_msm_info()
            pb = [t / k for t in tb[mode]]
            print(f"prove 2^{log2n:<2d} K={k:<4d} mode {mode} batch ms/proof {_stat(pb)} | loop ms/proof {_stat(pl)} | loop/batch {statistics.median(pl) / statistics.median(pb):6.2f}x"
                  f" | same bytes {same} | timed batch, ms: wires {ms[1]:.3f} hvals {ms[2]:.3f} B {ms[3]:.3f} A {ms[4]:.3f} C {ms[5]:.3f}; last pass of C:"
                  f" sort {st['digits'] + st['scan'] + st['scatter']:.3f} acc {st['accumulate']:.3f} tail {st['fixup'] + st['reduce']:.3f} fold+encode {ms[0]:.3f}"
                  f" (table {info['window_table']}, c = {info['window_bits']}, {info['buckets']} buckets, slices of {info['slice']})", flush=True)
        sols.free()
    for s in singles:
        s.free()
    q.free()


def msm_rows(ctx, rng, log2n, ks, reps, group, gname, modes, tables):
    n = 1 << log2n
    gen = np.random.default_rng(log2n)
    pts = api.Points.from_scalars(ctx, group, api.Poly.upload(ctx, [rng.fr() for _ in range(n)]))
    if tables:
        pts.precompute()
    for k in ks:
        raw = gen.integers(0, 256, size=(k * n, 32), dtype=np.uint8)
        raw[:, 0] &= 0x3F  # below r
        sc = api.Poly.upload(ctx, raw.tobytes())
        kl = min(k, LOOP_MAX)
        slices = [sc.slice(j * n, n) for j in range(kl)]
        out = {}

        def batch():
            out["b"] = api.msm_batch(ctx, pts, sc, k)

        def loop():
            out["l"] = [s.BlindEval(pts) for s in slices]

        tb, tl = _ab(ctx, modes, batch, loop, reps)
        pl = [t / kl for t in tl]
        for mode in modes:
            _set_mode(ctx, mode)
            batch()  # (the loop ran last: the plan of the batch's last pass)
            info = ctx.last_msm_info()
            pb = [t / k for t in tb[mode]]
            print(f"msm {gname} 2^{log2n:<2d} K={k:<4d} mode {mode} batch ms/member {_stat(pb)} | loop ms/member {_stat(pl)} | loop/batch {statistics.median(pl) / statistics.median(pb):6.2f}x"
                  f" | same bytes {out['b'][:kl] == out['l']} | last pass: table {info['window_table']}, c = {info['window_bits']}, {info['buckets']} buckets, slices of {info['slice']}", flush=True)
        for s in slices:
            s.free()
        sc.free()
    pts.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 12, 14, 16])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-msm", action="store_true")
    ap.add_argument("--skip-prove", action="store_true")
    ap.add_argument("--modes", type=int, nargs="+", default=[0], choices=[0, 1, 2], help="ps_msm_batch_set_table modes to alternate")
    ap.add_argument("--tables", action="store_true", help="window tables on the points of the msm rows")
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0xBA7C4)
    print(f"# library {os.path.basename(_lib.library_path())}; {args.reps} repetitions, median (min .. max); ps_msm_batch_set_table modes {args.modes}; loops over at most {LOOP_MAX} members", flush=True)
    if not args.skip_prove:
        for ln in args.log2n:
            prove_rows(ctx, rng, ln, args.k, args.reps, args.modes)
    if not args.skip_msm:
        for ln in args.log2n:
            msm_rows(ctx, rng, ln, args.k, args.reps, api.G1, "G1", args.modes, args.tables)
            msm_rows(ctx, rng, ln, args.k, args.reps, api.G2, "G2", args.modes, args.tables)
    ctx.close()


if __name__ == "__main__":
    main()
