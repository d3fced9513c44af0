#!/usr/bin/env python3
"""ps_kzg_open_multi and ps_scalars_lincomb against existing entry points, in one process, on one context:
    python tools/kzg_multi_sweep.py [--log2n 16 20] [--reps 5] [--out profiles/kzg_multi.txt]
Warm, `reps` repetitions each, the two sides of every comparison alternating; reported: the median and (min .. max) in ms,
wall clock around calls that end in a device synchronise (the method of tools/kzg_sweep.py).  Rows, per n = 2^log2n coefficients:
  open    (m, t) = (8, 2), six polynomials opened at the first point and two at the second, and (1, 1): ps_kzg_open_multi against
          the route a caller had before -- a loop of ps_kzg_open, one per polynomial over its points (eight proofs in the first
          case where the new call makes two)
  rows    ps_scalars_lincomb alone for the same two shapes, next to ps_poly_div_linear of one polynomial at t points: where the
          new kernel stands against the scan it feeds
Strings in the clear (tau known): what a measurement may do and a ceremony must not."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyref as pr  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402


def _timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _stat(v):
    return f"{statistics.median(v):10.4f} ({min(v):.4f} .. {max(v):.4f})"


def _alternate(fns, reps):
    """times[i] of fns[i]: every repetition runs each once, in turn; the first round is the warm-up."""
    times = [[] for _ in fns]
    for rep in range(reps + 1):
        for i, fn in enumerate(fns):
            t = _timed(fn)
            if rep:
                times[i].append(t)
    return times


def _random_poly(ctx, n, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F  # below r
    return api.Poly.upload(ctx, raw.tobytes())


def shape_rows(ctx, emit, rng, tau_g1, log2n, polys, first, reps):
    """polys[:first] are opened at the first point, the rest at the second (first == len(polys): one point)."""
    n, m = 1 << log2n, len(polys)
    t = 1 if first == m else 2
    zs = [rng.fr() for _ in range(t)]
    weight = lambda: 1 if m == 1 else (rng.fr() or 1)  # (1, 1) with weight 1 is ps_kzg_open: the same proof bytes
    coef = [[weight() if (j == 0) == (i < first) else 0 for j in range(t)] for i in range(m)]
    out = {}

    def multi():
        out["ys"], out["proofs"] = api.KZGOpenMulti(tau_g1, polys, zs, coef)

    def loop():
        out["loop"] = [api.KZGOpen(tau_g1, p, [zs[0 if i < first else 1]]) for i, p in enumerate(polys)]

    def rows():
        if "f" in out:
            out["f"].free()
        out["f"] = api.Poly.LinComb(polys, coef)

    def div():
        if "q" in out:
            out["q"].free()
        out["q"], _ = polys[0].DivLinear(zs)

    tm, tl = _alternate([multi, loop], reps)
    same = all(out["ys"][i][0 if i < first else 1] == out["loop"][i][0][0] for i in range(m))
    if m == 1:
        same = same and out["proofs"] == out["loop"][0][1]
    emit(f"open   2^{log2n:<2d} m={m} t={t} ps_kzg_open_multi ({t} proofs) {_stat(tm)} | loop of ps_kzg_open ({m} proofs) {_stat(tl)}"
         f" | loop / multi {statistics.median(tl) / statistics.median(tm):7.3f}x | same values {same}")
    tr, td = _alternate([rows, div], reps)
    emit(f"rows   2^{log2n:<2d} m={m} t={t} ps_scalars_lincomb {_stat(tr)} | ps_poly_div_linear of one polynomial at {t} points {_stat(td)}"
         f" | lincomb / div_linear {statistics.median(tr) / statistics.median(td):7.3f}")
    out["f"].free()
    out["q"].free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg_multi.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x4B5A4D)
    tau = rng.fr()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit(f"# library {os.path.basename(_lib.library_path())}; tile {_lib.lib.ps_poly_scan_tile()}; {args.reps} repetitions, median (min .. max), ms; the sides of a comparison alternate")
    for ln in args.log2n:
        n = 1 << ln
        tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
        polys = [_random_poly(ctx, n, 100 * ln + i) for i in range(8)]
        shape_rows(ctx, emit, rng, tau_g1, ln, polys, 6, args.reps)
        shape_rows(ctx, emit, rng, tau_g1, ln, polys[:1], 1, args.reps)
        for p in polys:
            p.free()
        tau_g1.free()
    ctx.close()


if __name__ == "__main__":
    main()
