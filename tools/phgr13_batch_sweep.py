#!/usr/bin/env python3
"""The PHGR13 batch prover and the batched multi-array sum against what the library offered before them, in one process, on
the same key and context:
    python tools/phgr13_batch_sweep.py [--log2n 10 12 14 16] [--k 1 8 64 256] [--reps 5]  > profiles/phgr13_prove_batch.txt
Per (n, K), warm, `reps` repetitions each, batch and loop alternating; reported: the median and (min .. max), wall clock around
calls that end in a device synchronise.
  prove   ps_phgr13_prove_batch of K witnesses, ms per proof, against a loop of ps_phgr13_prove over min(K, 64) of them (the
          single prover is untouched: the loop is the parent's behaviour), with the host-clock stage split of the last batch
          call (ps_prove_last_phase_ms): wires = witness conversion, K-column SpMV, gate check and the K runs of
          quotient_h_values | hs = the batched h sum | sums = the seven solution sums as ONE ps_msm_batch_multi
  multi   at one (n, K): ps_msm_batch_multi over the key's seven arrays (six G1, one G2; stride m, first diff) against seven
          ps_msm_batch calls over the same members packed back to back -- what the shared sort and the side-by-side folds are
          worth -- and against one ps_msm_multi per member (the single prover's sum)
--modes M [M ...]: ps_msm_batch_set_table modes of the batch prover (0 automatic, 1 never over window tables, 2 wherever a
table is usable), alternated with each other and with the loop inside every repetition; `--modes 1 0` is the A/B of the tabled
pass (profiles/phgr13_prove_batch_table.txt).
Witnesses: the tiled synthetic circuit with up to 8 values of x0, repeated to K (the work does not depend on whether
witnesses repeat: every member has its own bucket sets)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402

LOOP_MAX = 64
ARRAYS = ("vs", "ws", "ys", "vas", "was", "yas", "vbs")  # vbs stands in for the pointwise beta sum: a G1 array of the same length


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


def _ab_modes(ctx, modes, batch, loop, reps):
    """{mode: times of the batch}, times of the loop: every repetition runs the batch once per mode, then the loop."""
    tb, tl = {m: [] for m in modes}, []
    for rep in range(reps + 1):  # the first round is the warm-up
        for m in modes:
            _set_mode(ctx, m)
            t = _timed(batch)
            if rep:
                tb[m].append(t)
        t = _timed(loop)
        if rep:
            tl.append(t)
    return tb, tl


def _ab(batch, loop, reps):
    batch(); loop()  # warm: buffers sized, code objects loaded, window tables of the single prover built
    tb, tl = [], []
    for _ in range(reps):
        tb.append(_timed(batch))
        tl.append(_timed(loop))
    return tb, tl


def _fields(p):
    return tuple(getattr(p, f) for f in api.PHGR13Proof.FIELDS)


def rows_for(ctx, rng, log2n, ks, reps, multi_k, modes):
    n = 1 << log2n
    distinct = min(8, max(ks))
    made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(distinct)]
    c = made[0][0]
    q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    ek, _ = api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    rows = [b"".join(int(v).to_bytes(32, "big") for v in sol) for _, sol in made]
    singles = [api.Poly.upload(ctx, r) for r in rows]
    m, diff = c.nbVars, c.nbVars - c.nbIO
    for k in ks:
        sols = api.Poly.upload(ctx, b"".join(rows[j % distinct] for j in range(k)))
        kl = min(k, LOOP_MAX)
        out = {}

        def batch():
            out["b"] = api.PHGR13ProveBatch(ek, q, sols, k)

        def loop():
            out["l"] = [api.PHGR13Prove(ek, q, singles[j % distinct]) for j in range(kl)]

        tb, tl = _ab_modes(ctx, modes, batch, loop, reps)
        pl = [t / kl for t in tl]
        for mode in modes:
            _set_mode(ctx, mode)
            batch()
            same = all(_fields(out["b"][j]) == _fields(out["l"][j]) for j in range(kl))
            ph = ctx.last_prove_phase_ms()
            info = ctx.last_msm_info()
            pb = [t / k for t in tb[mode]]
            wins = all(b < min(pl) for b in pb)
            print(f"prove 2^{log2n:<2d} K={k:<4d} mode {mode} batch ms/proof {_stat(pb)} | loop ms/proof {_stat(pl)} | loop/batch {statistics.median(pl) / statistics.median(pb):6.2f}x"
                  f" | every batch rep below every loop rep {wins} | same bytes {same} | last batch, host ms: wires+hvals {ph['quotient']:.3f}"
                  f" hs {ph['prep_or_h_sum']:.3f} sums {ph['sums']:.3f} total {ph['total']:.3f}"
                  f" (sums: table {info['window_table']}, c = {info['window_bits']}, {info['buckets']} buckets in the last pass, slices of {info['slice']};"
                  f" lgsi table window {ek.lgsi.table_window})", flush=True)
        _set_mode(ctx, modes[-1])
        if k == multi_k:
            arrays = [getattr(ek, f) for f in ARRAYS]
            nn = len(arrays[0])
            packed = api.Poly.upload(ctx, b"".join(rows[j % distinct][32 * diff : 32 * (diff + nn)] for j in range(k)))
            views = [singles[j % distinct].slice(diff, nn) for j in range(kl)]

            def one_call():
                out["m"] = api.msm_batch_multi(ctx, arrays, sols, k, m, diff)

            def seven_calls():
                out["s"] = [api.msm_batch(ctx, a, packed, k) for a in arrays]

            def per_member():
                out["p"] = [api.msm_multi(ctx, arrays, v) for v in views]

            tm, ts = _ab(one_call, seven_calls, reps)
            tm2, tp = _ab(one_call, per_member, reps)
            same = out["m"] == out["s"] and all(out["m"][i][j] == out["p"][j][i] for i in range(7) for j in range(kl))
            print(f"multi 2^{log2n:<2d} K={k:<4d} n={nn}: ps_msm_batch_multi over 7 arrays, ms/member {_stat([t / k for t in tm + tm2])} | seven ps_msm_batch calls"
                  f" {_stat([t / k for t in ts])} | one ps_msm_multi per member {_stat([t / kl for t in tp])} | seven calls / one call"
                  f" {statistics.median(ts) / statistics.median(tm):5.2f}x | same bytes {same}", flush=True)
            for v in views:
                v.free()
            packed.free()
        sols.free()
    for s in singles:
        s.free()
    q.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 12, 14, 16])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, nargs="+", default=[0], choices=[0, 1, 2], help="ps_msm_batch_set_table modes to alternate")
    ap.add_argument("--multi-at", type=int, nargs=2, default=[10, 64], metavar=("LOG2N", "K"), help="where the sum alone is compared")
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x9468713)
    print(f"# library {os.path.basename(_lib.library_path())}; {args.reps} repetitions, median (min .. max); ps_msm_batch_set_table modes {args.modes}; loops over at most {LOOP_MAX} members", flush=True)
    for ln in args.log2n:
        rows_for(ctx, rng, ln, args.k, args.reps, args.multi_at[1] if ln == args.multi_at[0] else -1, args.modes)
    ctx.close()


if __name__ == "__main__":
    main()
