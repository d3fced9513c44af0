#!/usr/bin/env python3
"""The KZG proofs of EVERY node of the domain in one call against the loop a caller had before, in one process, on one context:
    python tools/kzg_all_sweep.py [--log2n 4 6 8 10 12 14 16] [--reps 5] [--chunk 256] [--sample 8] [--out profiles/kzg_all.txt]
The method of tools/kzg_set_lagrange_sweep.py: warm, `reps` repetitions each, the sides of every comparison alternating, one box;
reported: the median and (min .. max) in ms, wall clock around calls that end in a device synchronise.  Rows, per n = 2^log2n
gates of the tiled toy circuit (bench.synthetic_r1cs) and n random values:
  (a)  ps_kzg_open_all_lagrange with the key table | with all_key = NULL | ps_kzg_all_key_lagrange alone | the baseline:
       ps_kzg_open_lagrange over all nodes in chunks of `chunk` nodes (k * n < 2^32 and k * n * 32 bytes of quotient rows).  Where
       the baseline has more than 4 * `sample` chunks only `sample` chunks, spread evenly, are timed and the time is scaled to
       n nodes: the row says "scaled".  The proofs of the timed chunks are compared with the call's for equal bytes.
  (b)  the peak device memory of the tabled call and of one baseline chunk (tools/kzg_set_sweep.py's sampler)
  (c)  the stage split of a tabled call from events between the stages (ps_debug_kzg_all_stage_ms): the scalar side, load,
       forward, pointwise, inverse, combine, normalise
and at the end the largest swept n at which the loop is faster than the tabled call, if any.
The string is held in the clear (tau known): what a measurement may do and a ceremony must not."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from kzg_set_sweep import PeakMemory, _alternate, _mib, _stat  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402
from playsnark_amd import _lib, api  # noqa: E402

STAGES = ("scalar side", "load", "forward", "pointwise", "inverse", "combine", "normalise")


def rows(ctx, emit, rng, tau, log2n, reps, chunk, sample, mem):
    n = 1 << log2n
    nvars, L, Rm, O, _ = bench.synthetic_r1cs(n)
    qap = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    values = api.Poly.upload(ctx, [rng.fr() for _ in range(n)])
    lag_g1 = api.Points.from_scalars(ctx, api.G1, api.Poly.upload(ctx, rs.lagrange_at(n, tau)[0]))
    key = api.KZGAllKeyLagrange(qap, lag_g1)
    chunk = min(chunk, n)
    starts = list(range(1, n + 1, chunk))
    scaled = len(starts) > 4 * sample
    if scaled:
        starts = [starts[(i * len(starts)) // sample] for i in range(sample)]
    factor = (n / chunk) / len(starts)
    out = {}

    def tabled():
        out["all"] = api.KZGOpenAllLagrange(qap, lag_g1, values, key).download()

    def untabled():
        out["nokey"] = api.KZGOpenAllLagrange(qap, lag_g1, values).download()

    def key_alone():
        api.KZGAllKeyLagrange(qap, lag_g1)

    def one_chunk(first):
        return api.KZGOpenLagrange(qap, lag_g1, values, list(range(first, min(first + chunk, n + 1))))[1]

    def loop():
        out["loop"] = [one_chunk(first) for first in starts]

    tt, tu, tk, tl = _alternate([tabled, untabled, key_alone, loop], reps)
    tl = [t * factor for t in tl]
    same = out["all"] == out["nokey"] and all(
        out["all"][96 * (first - 1) : 96 * (first - 1 + len(proofs))] == b"".join(proofs) for first, proofs in zip(starts, out["loop"]))
    med = statistics.median
    emit(f"(a) open    2^{log2n:<2d} open_all with the table {_stat(tt)} | all_key = NULL {_stat(tu)} | all_key alone {_stat(tk)}"
         f" | open_lagrange over all nodes, chunks of {chunk}{f', {len(starts)} chunks timed and scaled x{factor:.0f}' if scaled else ''} {_stat(tl)}"
         f" | loop / tabled {med(tl) / med(tt):8.2f}x, loop / untabled {med(tl) / med(tu):8.2f}x | same bytes {same}")
    m_all, m_loop = mem.of(tabled), mem.of(lambda: one_chunk(starts[0]))
    emit(f"(b) memory  2^{log2n:<2d} open_all with the table peak {_mib(m_all)} | one chunk of {chunk} nodes of the loop peak {_mib(m_loop)}")
    ms = (C.c_float * len(STAGES))()
    split = []
    for rep in range(reps + 1):
        h = C.c_void_p()
        api._check(_lib.lib.ps_debug_kzg_all_stage_ms(ctx._h, qap._h, lag_g1._h, key._h, values._h, C.byref(h), ms))
        _lib.lib.ps_points_free(h)
        if rep:
            split.append(list(ms))
    emit(f"(c) stages  2^{log2n:<2d} " + " | ".join(f"{name} {med([s[i] for s in split]):9.4f}" for i, name in enumerate(STAGES))
         + f" | sum {med([sum(s) for s in split]):9.4f}")
    return med(tt), med(tl), max(tt) - min(tt), max(tl) - min(tl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[4, 6, 8, 10, 12, 14, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kzg_all.txt"))
    args = ap.parse_args()
    _lib.lib.ps_debug_kzg_all_stage_ms.argtypes = [C.c_void_p] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_float)]
    _lib.lib.ps_debug_kzg_all_stage_ms.restype = C.c_int
    ctx = api.Context(0)
    mem = PeakMemory()
    rng = pr.SplitMix64(0x414C4C)
    tau = rng.fr()
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        with open(args.out, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    emit(f"# library {os.path.basename(_lib.library_path())}; one box, warm, {args.reps} repetitions, median (min .. max), ms; the sides of a"
         f" comparison alternate; stages from events")
    loop_wins = []
    for ln in args.log2n:
        t_all, t_loop, spread_all, spread_loop = rows(ctx, emit, rng, tau, ln, args.reps, args.chunk, args.sample, mem)
        if t_loop < t_all:
            loop_wins.append(ln)
        emit(f"(d) verdict 2^{ln:<2d} tabled {'faster' if t_all < t_loop else 'SLOWER'} than the loop by {abs(t_loop - t_all):.4f} ms;"
             f" spreads {spread_all:.4f} and {spread_loop:.4f} ms")
    emit("# the loop wins " + (f"up to n = 2^{max(loop_wins)} of the sizes swept" if loop_wins else "at none of the sizes swept"))
    ctx.close()


if __name__ == "__main__":
    main()
