#!/usr/bin/env python3
"""The KZG entries against existing entry points, in one process, on one context:
    python tools/kzg_sweep.py [--log2n 16 20] [--k 1 16] [--verify-k 64 4096] [--reps 5] [--out profiles/kzg.txt]
Warm, `reps` repetitions each, the two sides of every comparison alternating; reported: the median and (min .. max) in ms,
wall clock around calls that end in a device synchronise.  Rows, per n = 2^log2n coefficients and k points:
  scan    ps_poly_eval and ps_poly_div_linear alone (the latter with the allocation of its k (n - 1) result scalars)
  (a)     k = 1: ps_poly_eval + ps_poly_div_linear against ps_msm over the same n - 1 points and scalars -- the scan must be
          the smaller by far (about 3 n Fr products against n W mixed additions)
  open    ps_kzg_open, and its stages: ps_poly_div_linear, then ps_msm_batch of the quotient rows
  (b)     the largest k: ps_kzg_open against the route a caller had before, existing entries only: ps_scalars_download, synthetic
          division on the host (Python integers: faster here than numpy object arrays, and the C oracle has no division by a
          linear factor), ps_scalars_upload and k ps_msm calls
  verify  ps_kzg_verify_batch of K openings (subgroup tests on) against a loop of ps_kzg_verify over min(K, 64) of them,
          ms per opening
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

LOOP_MAX = 64
R = pr.R


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


def _host_division(coeffs, z):
    """(p - p(z)) / (X - z), lowest degree first, and p(z): Horner from the top"""
    q = [0] * (len(coeffs) - 1)
    h = 0
    for i in range(len(coeffs) - 1, 0, -1):
        h = (coeffs[i] + z * h) % R
        q[i - 1] = h
    return q, (coeffs[0] + z * h) % R


def scan_rows(ctx, emit, rng, tau, log2n, ks, reps):
    n = 1 << log2n
    tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
    head = tau_g1.slice(0, n - 1)
    p = _random_poly(ctx, n, log2n)
    for k in ks:
        zs = [rng.fr() for _ in range(k)]
        out = {}

        def ev():
            out["y"] = p.Eval(zs)

        def div():
            if "q" in out:
                out["q"].free()
            out["q"], out["rem"] = p.DivLinear(zs)

        def both():
            ev()
            div()

        def msm_one():
            out["m"] = out["row0"].BlindEval(head)

        def sum_rows():
            out["pb"] = api.msm_batch(ctx, head, out["q"], k)

        def opened():
            out["ys"], out["proofs"] = api.KZGOpen(tau_g1, p, zs)

        div()
        out["row0"] = out["q"].slice(0, n - 1)
        row0 = out["row0"]
        te, td = _alternate([ev, div], reps)
        emit(f"scan   2^{log2n:<2d} k={k:<3d} ps_poly_eval {_stat(te)} | ps_poly_div_linear {_stat(td)}")
        if k == 1:
            tb, tm = _alternate([both, msm_one], reps)
            emit(f"(a)    2^{log2n:<2d} k=1   eval + div_linear {_stat(tb)} | ps_msm over the same {n - 1} points {_stat(tm)} | scan / sum"
                 f" {statistics.median(tb) / statistics.median(tm):7.4f}")
        to, td2, ts = _alternate([opened, div, sum_rows], reps)
        same = out["proofs"] == out["pb"] and out["ys"] == out["rem"] == out["y"]
        emit(f"open   2^{log2n:<2d} k={k:<3d} ps_kzg_open {_stat(to)} | stages: div_linear {_stat(td2)} + ps_msm_batch {_stat(ts)} | same bytes {same}")
        if k == max(ks) and k > 1:
            got = {}

            def composed():
                raw = p.download_bytes()
                coeffs = [int.from_bytes(raw[32 * i : 32 * i + 32], "big") for i in range(n)]
                ys, proofs = [], []
                for z in zs:
                    q, y = _host_division(coeffs, z)
                    qd = api.Poly.upload(ctx, b"".join(v.to_bytes(32, "big") for v in q))
                    proofs.append(qd.BlindEval(head))
                    qd.free()
                    ys.append(y)
                got["ys"], got["proofs"] = ys, proofs

            tc, to2 = _alternate([composed, opened], reps)
            same = got["proofs"] == out["proofs"] and got["ys"] == out["ys"]
            emit(f"(b)    2^{log2n:<2d} k={k:<3d} composed (download, host division, upload, {k} ps_msm) {_stat(tc)} | ps_kzg_open {_stat(to2)}"
                 f" | composed / open {statistics.median(tc) / statistics.median(to2):8.2f}x | same bytes {same}")
        row0.free()
        out["q"].free()
    p.free()
    head.free()
    tau_g1.free()


def verify_rows(ctx, emit, rng, tau, ks, reps):
    n = 1 << 10
    tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
    t2 = api.Points.from_scalars(ctx, api.G2, api.Poly.upload(ctx, [tau])).download()
    p = _random_poly(ctx, n, 99)
    commit = api.KZGCommit(tau_g1, p)
    for k in ks:
        zs = [rng.fr() for _ in range(k)]
        ys, proofs = api.KZGOpen(tau_g1, p, zs)
        rhos = [((rng.next() << 64) | rng.next()) or 1 for _ in range(k)]
        kl = min(k, LOOP_MAX)
        out = {}

        def batch():
            out["b"] = api.KZGVerifyBatch(ctx, t2, [commit] * k, zs, ys, proofs, rhos, True)

        def loop():
            out["l"] = all(api.KZGVerify(t2, commit, zs[j], ys[j], proofs[j]) for j in range(kl))

        tb, tl = _alternate([batch, loop], reps)
        pb, pl = [t / k for t in tb], [t / kl for t in tl]
        emit(f"verify 2^10 K={k:<5d} ps_kzg_verify_batch ms/opening {_stat(pb)} (call {statistics.median(tb):.2f} ms) | loop of ps_kzg_verify over {kl} ms/opening {_stat(pl)}"
             f" | loop / batch {statistics.median(pl) / statistics.median(pb):8.2f}x | accepted {out['b']} {out['l']}")
    p.free()
    tau_g1.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--verify-k", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x4B5A47)
    tau = rng.fr()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit(f"# library {os.path.basename(_lib.library_path())}; tile {_lib.lib.ps_poly_scan_tile()}; {args.reps} repetitions, median (min .. max), ms; the sides of a comparison alternate")
    for ln in args.log2n:
        scan_rows(ctx, emit, rng, tau, ln, args.k, args.reps)
    verify_rows(ctx, emit, rng, tau, args.verify_k, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
