#!/usr/bin/env python3
"""One proof for a set of points of a polynomial held as its VALUES against the routes a caller had before, in one process, on
one context:
    python tools/kzg_set_lagrange_sweep.py [--log2n 16 20] [--k 1 16 64] [--reps 5] [--rows a b] [--out profiles/kzg_set_lagrange.txt] [--append]
The method of tools/kzg_lagrange_sweep.py: warm, `reps` repetitions each, the sides of every comparison alternating, one box;
reported: the median and (min .. max) in ms, wall clock around calls that end in a device synchronise.  Rows, per n = 2^log2n
gates of the tiled toy circuit (bench.synthetic_r1cs) and k random points, for k > 1 the last of them replaced by a node:
  (a)  ps_qap_gate_values + ps_kzg_open_set_lagrange (ONE proof) against
         ps_qap_interpolate + ps_kzg_open_set                       (the same bytes, by way of the coefficients),
         ps_qap_gate_values + ps_kzg_open_lagrange                  (k proofs), and
         the hand composition ps_qap_gate_values + ps_poly_div_linear_lagrange + ps_scalars_lincomb + ps_msm (the same bytes; the
         weights c_j = 1 / prod_{l != j} (z_j - z_l) computed beforehand, outside the timed part)
  (b)  ps_poly_div_roots_lagrange alone (no remainder: host work the opening does not do) against the hand composition without its
       sum, with the peak device memory of both as tools/kzg_set_sweep.py samples it
Row (b) under PLAYSNARK_HIP_LIB=<a build with -DPS_LAGR_SET_GROUP=1> is the fold with ONE INVERSION PER POINT, the A/B of the
shared inversion (row (c) of DESIGN.md section 11); such a run is a process of its own and appends (--rows b --append).
The string is held in the clear (tau known): what a measurement may do and a ceremony must not."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from kzg_set_sweep import PeakMemory, _alternate, _mib, _stat, _weights  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402


def rows(ctx, emit, rng, tau, log2n, ks, reps, which_rows, mem):
    n = 1 << log2n
    nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
    qap = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    w = api.Poly.upload(ctx, sol)
    if "a" in which_rows:
        tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
        lag_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.upload(ctx, rs.lagrange_at(n, tau)[0]))
    values = qap.gate_values(w, 0)
    for k in ks:
        zs = [rng.fr() for _ in range(k)]
        if k > 1:
            zs[-1] = n // 2
        ws = _weights(zs)
        out = {}

        def composed_row(v):
            rows_, ys = v.DivLinearLagrange(qap, zs)
            views = [rows_.slice(j * n, n) for j in range(k)]
            q = api.Poly.LinComb(views, [[c] for c in ws])
            for view in views:
                view.free()
            rows_.free()
            return q, ys

        def set_value_route():
            v = qap.gate_values(w, 0)
            out["set"] = api.KZGOpenSetLagrange(qap, lag_g1, v, zs)
            v.free()

        def set_coefficient_route():
            p = qap.interpolate(w, 0)
            out["mono"] = api.KZGOpenSet(tau_g1, p, zs)
            p.free()

        def k_proofs():
            v = qap.gate_values(w, 0)
            out["k"] = api.KZGOpenLagrange(qap, lag_g1, v, zs)
            v.free()

        def by_hand():
            v = qap.gate_values(w, 0)
            q, ys = composed_row(v)
            out["hand"] = (ys, q.BlindEval(lag_g1))
            q.free()
            v.free()

        def div_roots():
            if "q" in out:
                out["q"].free()
            out["q"], out["yq"], _ = values.DivRootsLagrange(qap, zs, remainder=False)

        def composed():
            if "qc" in out:
                out["qc"].free()
            out["qc"], out["yc"] = composed_row(values)

        if "a" in which_rows:
            ts, tm, tk, th = _alternate([set_value_route, set_coefficient_route, k_proofs, by_hand], reps)
            med = statistics.median
            emit(f"(a) open    2^{log2n:<2d} k={k:<3d} gate_values + open_set_lagrange (1 proof) {_stat(ts)} | interpolate + ps_kzg_open_set {_stat(tm)}"
                 f" | gate_values + open_lagrange ({k} proofs) {_stat(tk)} | by hand {_stat(th)}"
                 f" | over set_lagrange: coefficients {med(tm) / med(ts):6.2f}x, k proofs {med(tk) / med(ts):6.2f}x, by hand {med(th) / med(ts):6.2f}x"
                 f" | same bytes {out['set'] == out['mono'] == out['hand']}, same values {out['set'][0] == out['k'][0]}")
        if "b" in which_rows:
            td, tc = _alternate([div_roots, composed], reps)
            same = out["yq"] == out["yc"] and out["q"].download_bytes() == out["qc"].download_bytes()
            out.pop("q").free()
            out.pop("qc").free()
            md, mc = mem.of(div_roots), mem.of(composed)
            out.pop("q").free()
            out.pop("qc").free()
            emit(f"(b) rows    2^{log2n:<2d} k={k:<3d} ps_poly_div_roots_lagrange {_stat(td)} peak {_mib(md)} | div_linear_lagrange + lincomb {_stat(tc)}"
                 f" peak {_mib(mc)} | composed / fused {statistics.median(tc) / statistics.median(td):8.3f}x | same words {same}")
    values.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", nargs="*", default=["a", "b"])
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg_set_lagrange.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    mem = PeakMemory()
    rng = pr.SplitMix64(0x534C47)
    tau = rng.fr()
    lines = []
    before = open(args.out).read() if args.append and os.path.exists(args.out) else ""

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write(before + "\n".join(lines) + "\n")

    tile = _lib.lib.ps_poly_lagrange_tile()
    emit(f"# library {os.path.basename(_lib.library_path())}; T_L {tile} (I = {tile // 256}), group G = {_lib.lib.ps_poly_lagrange_set_group()};"
         f" one box, warm, {args.reps} repetitions, median (min .. max), ms; the sides of a comparison alternate")
    for ln in args.log2n:
        rows(ctx, emit, rng, tau, ln, args.k, args.reps, args.rows, mem)
    ctx.close()


if __name__ == "__main__":
    main()
