#!/usr/bin/env python3
"""One proof for a set of points of one polynomial against the routes a caller had before, in one process, on one context:
    python tools/kzg_set_sweep.py [--log2n 16 20] [--k 1 2 16 64] [--reps 5] [--rows a b c] [--out profiles/kzg_set.txt]
The method of tools/kzg_sweep.py: warm, `reps` repetitions each, the sides of every comparison alternating, one box; reported:
the median and (min .. max) in ms, wall clock around calls that end in a device synchronise.  Rows, per n = 2^log2n
coefficients and k points:
  (a)     ps_kzg_open_set (ONE proof) against ps_kzg_open at the same points (k proofs): the route a caller had
  (b)     the part in front of the sum: ps_poly_div_roots (quotient and values; the remainder, host work the opening does not
          do, is not asked for) against the composed route over earlier entries only -- ps_poly_div_linear, then
          ps_scalars_lincomb of its k row slices with the weights w_j = 1 / prod_{l != j} (z_j - z_l) (computed beforehand,
          outside the timed part, where ps_poly_div_roots computes them inside) -- with the peak device memory of both: the
          drop of hipMemGetInfo's free figure below its value before the call, sampled by a second thread while the call runs
  (c)     ps_kzg_verify_set against k calls of ps_kzg_verify
Strings in the clear (tau known): what a measurement may do and a ceremony must not.  PLAYSNARK_HIP_LIB selects another build of
the library (another group size G of the set apply pass): --rows b is the row that depends on it."""
import argparse
import ctypes
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyref as pr  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402

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


class PeakMemory:
    """Peak device memory of a call: a second thread reads hipMemGetInfo while the call runs (ctypes releases the interpreter
    lock around both) and keeps the lowest free figure; the peak is its drop below the figure before the call."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def free(self):
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if self.hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) != 0:
            raise RuntimeError("hipMemGetInfo failed")
        return f.value

    def of(self, fn):
        before = self.free()
        low = [before]
        stop = threading.Event()

        def sample():
            while not stop.is_set():
                low[0] = min(low[0], self.free())

        th = threading.Thread(target=sample)
        th.start()
        try:
            fn()
        finally:
            stop.set()
            th.join()
        return max(before - low[0], 0)


def _random_poly(ctx, n, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F  # below r
    return api.Poly.upload(ctx, raw.tobytes())


def _weights(zs):
    ws = []
    for j, zj in enumerate(zs):
        d = 1
        for l, zl in enumerate(zs):
            if l != j:
                d = d * (zj - zl) % R
        ws.append(pow(d, R - 2, R))
    return ws


def _mib(b):
    return f"{b / 2**20:9.1f} MiB"


def rows_for(ctx, emit, rng, tau, log2n, ks, reps, which, mem):
    n = 1 << log2n
    tau_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, tau, n))
    tau_g2 = api.Points.from_scalars(ctx, api.G2, api.Poly.powers(ctx, tau, max(ks) + 1))
    t2 = tau_g2.download(1, 1)
    p = _random_poly(ctx, n, log2n)
    commit = api.KZGCommit(tau_g1, p) if "c" in which else None
    for k in ks:
        zs = [rng.fr() for _ in range(k)]
        ws = _weights(zs)
        out = {}

        def open_set():
            out["ys"], out["proof"] = api.KZGOpenSet(tau_g1, p, zs)

        def open_k():
            out["ys_k"], out["proofs"] = api.KZGOpen(tau_g1, p, zs)

        def div_roots():
            if "q" in out:
                out["q"].free()
            out["q"], out["yq"], _ = p.DivRoots(zs, remainder=False)

        def composed():
            if "qc" in out:
                out["qc"].free()
            rows, out["yc"] = p.DivLinear(zs)
            views = [rows.slice(j * (n - 1), n - 1) for j in range(k)]
            out["qc"] = api.Poly.LinComb(views, [[w] for w in ws])
            for v in views:
                v.free()
            rows.free()

        if "a" in which:
            ts, tk = _alternate([open_set, open_k], reps)
            same = out["ys"] == out["ys_k"] and api.points_lincomb(api.G1, b"".join(out["proofs"]), ws) == out["proof"]
            emit(f"(a) open    2^{log2n:<2d} k={k:<3d} ps_kzg_open_set (1 proof) {_stat(ts)} | ps_kzg_open ({k} proofs) {_stat(tk)}"
                 f" | open / set {statistics.median(tk) / statistics.median(ts):8.3f}x | proof = sum w_j proofs_j {same}")
        if "b" in which:
            td, tc = _alternate([div_roots, composed], reps)
            same = out["yq"] == out["yc"] and out["q"].download_bytes() == out["qc"].download_bytes(0, n - k)
            top = out["qc"].download(n - k, k - 1) if k > 1 else []
            out.pop("q").free()
            out.pop("qc").free()
            md, mc = mem.of(div_roots), mem.of(composed)
            out.pop("q").free()
            out.pop("qc").free()
            emit(f"(b) divide  2^{log2n:<2d} k={k:<3d} ps_poly_div_roots {_stat(td)} peak {_mib(md)} | div_linear + lincomb {_stat(tc)} peak {_mib(mc)}"
                 f" | composed / fused {statistics.median(tc) / statistics.median(td):8.3f}x | same words {same}, zero top {not any(top)}")
        if "c" in which:
            ys, proof = api.KZGOpenSet(tau_g1, p, zs)
            _, proofs = api.KZGOpen(tau_g1, p, zs)

            def verify_set():
                out["vs"] = api.KZGVerifySet(ctx, tau_g1, tau_g2, commit, zs, ys, proof)

            def verify_k():
                out["vk"] = all(api.KZGVerify(t2, commit, zs[j], ys[j], proofs[j]) for j in range(k))

            tv, tl = _alternate([verify_set, verify_k], reps)
            emit(f"(c) verify  2^{log2n:<2d} k={k:<3d} ps_kzg_verify_set {_stat(tv)} | {k} x ps_kzg_verify {_stat(tl)}"
                 f" | loop / set {statistics.median(tl) / statistics.median(tv):8.3f}x | accepted {out['vs']} {out['vk']}")
    p.free()
    tau_g1.free()
    tau_g2.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--k", type=int, nargs="*", default=[1, 2, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg_set.txt"))
    args = ap.parse_args()
    ctx = api.Context(0)
    mem = PeakMemory()
    rng = pr.SplitMix64(0x4B5A48)
    tau = rng.fr()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit(f"# library {os.path.basename(_lib.library_path())}; tile {_lib.lib.ps_poly_scan_tile()}, group G = {_lib.lib.ps_poly_scan_set_group()};"
         f" one box, warm, {args.reps} repetitions, median (min .. max), ms; the sides of a comparison alternate")
    for ln in args.log2n:
        rows_for(ctx, emit, rng, tau, ln, args.k, args.reps, args.rows, mem)
    ctx.close()


if __name__ == "__main__":
    main()
