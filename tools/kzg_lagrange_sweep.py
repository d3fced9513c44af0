#!/usr/bin/env python3
"""The value-form (Lagrange-form) KZG entries against the coefficient route, in one process, on one context:
    python tools/kzg_lagrange_sweep.py [--log2n 16 20] [--k 1 16] [--reps 5] [--rows a b] [--out profiles/kzg_lagrange.txt] [--append]
Warm, `reps` repetitions each, the two sides of every comparison alternating; reported: the median and (min .. max) in ms,
wall clock around calls that end in a device synchronise -- the method of tools/kzg_sweep.py.  Rows, per n = 2^log2n gates of
the tiled toy circuit (bench.synthetic_r1cs) and k random points, for k > 1 the last of them replaced by a node of the domain:
  (a)  ps_qap_gate_values + ps_kzg_open_lagrange against the only route to the same bytes without them:
       ps_qap_interpolate + ps_kzg_open; "same bytes" compares values and proofs of the two
  (b)  ps_poly_div_linear_lagrange alone against ps_poly_div_linear on ready coefficients (informational: the two return
       different representations of the same quotients)
Row (b) under PLAYSNARK_HIP_LIB=<a build with -DPS_LAGR_LOG_ITEMS=2 or 4> is the A/B of the nodes per thread; such runs append to
profiles/kzg_lagrange_items_ab.txt (--rows b --append --out ...).
The string is held in the clear (tau known): what a measurement may do and a ceremony must not."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
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


def rows(ctx, emit, rng, tau, log2n, ks, reps, which_rows):
    n = 1 << log2n
    nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
    qap = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    w = api.Poly.upload(ctx, sol)
    out = {}
    if "a" in which_rows:
        tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
        lag_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.upload(ctx, rs.lagrange_at(n, tau)[0]))
    values, coeffs = qap.gate_values(w, 0), qap.interpolate(w, 0)
    for k in ks:
        zs = [rng.fr() for _ in range(k)]
        if k > 1:
            zs[-1] = n // 2

        def value_route():
            v = qap.gate_values(w, 0)
            out["lag"] = api.KZGOpenLagrange(qap, lag_g1, v, zs)
            v.free()

        def coefficient_route():
            p = qap.interpolate(w, 0)
            out["mono"] = api.KZGOpen(tau_g1, p, zs)
            p.free()

        def div_values():
            if "qv" in out:
                out["qv"].free()
            out["qv"], out["yv"] = values.DivLinearLagrange(qap, zs)

        def div_coeffs():
            if "q" in out:
                out["q"].free()
            out["q"], out["yc"] = coeffs.DivLinear(zs)

        if "a" in which_rows:
            tv, tc = _alternate([value_route, coefficient_route], reps)
            emit(f"(a)    2^{log2n:<2d} k={k:<3d} gate_values + open_lagrange {_stat(tv)} | interpolate + ps_kzg_open {_stat(tc)}"
                 f" | coefficient / value {statistics.median(tc) / statistics.median(tv):6.2f}x | same bytes {out['lag'] == out['mono']}")
        if "b" in which_rows:
            tv, tc = _alternate([div_values, div_coeffs], reps)
            emit(f"(b)    2^{log2n:<2d} k={k:<3d} ps_poly_div_linear_lagrange {_stat(tv)} | ps_poly_div_linear {_stat(tc)}"
                 f" | value / coefficient {statistics.median(tv) / statistics.median(tc):6.2f}x | same values {out['yv'] == out['yc']}")
            out.pop("qv").free()
            out.pop("q").free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", nargs="*", default=["a", "b"])
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg_lagrange.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x4C4147)
    tau = rng.fr()
    lines = []
    before = open(args.out).read() if args.append and os.path.exists(args.out) else ""

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write(before + "\n".join(lines) + "\n")

    tile = _lib.lib.ps_poly_lagrange_tile()
    emit(f"# library {os.path.basename(_lib.library_path())}; T_L {tile} (I = {tile // 256}); {args.reps} repetitions, median (min .. max), ms;"
         " the sides of a comparison alternate")
    for ln in args.log2n:
        rows(ctx, emit, rng, tau, ln, args.k, args.reps, args.rows)
    ctx.close()


if __name__ == "__main__":
    main()
