#!/usr/bin/env python3
"""The PHGR13 batch verifier against what the library offered before it -- a loop of ps_phgr13_verify over the same proofs --
in one process, on the same key and context:
    python tools/phgr13_verify_batch_sweep.py [--gates 7 64] [--n 1 16 64 256 1024 4096] [--reps 5]  > profiles/phgr13_verify_batch.txt
Per (gates, N), warm: the median and (min .. max) of `reps` ps_phgr13_verify_batch calls (wall clock; the call ends with the
stream idle), the stage split of ONE more call on a timed context (ps_ctx_set_timing: the stream is drained at every stage
boundary, so the stages add up to a little more than the untimed call; ps_debug_phgr13_verify_batch_stage_ms), and the
loop: N calls of ps_phgr13_verify, structs and input vectors prepared beforehand, `loop reps` times (one repetition from 1 024
proofs on: the loop takes seconds there).  The single verifier is untouched by the batch entry, so the loop is the parent's
behaviour.
Proofs: ps_phgr13_prove_batch over 8 values of x0 of the tiled synthetic circuit (diff = gates - 1 public inputs), repeated
to N (the work does not depend on whether proofs repeat); weights of 128 bits.  Both verdicts are checked (all valid)."""
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

STAGES = ("upload+subgroup", "rho*gv", "sums", "miller", "host")
DISTINCT = 8


def _timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _stat(v):
    return f"{statistics.median(v):10.3f} ({min(v):.3f} .. {max(v):.3f})"


def rows_for(ctx, rng, gates, ns, reps):
    made = [rs.synthetic_circuit(gates, x0=3 + 2 * j) for j in range(DISTINCT)]
    c = made[0][0]
    diff = c.nbVars - c.nbIO
    q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    ek, key = api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    distinct = api.PHGR13ProveBatch(ek, q, api.Poly.upload(ctx, [v for _, s in made for v in s]), DISTINCT)
    vk = _lib.Phgr13Vk()
    for name in api.PHGR13VerifKey.FIXED:
        C.memmove(getattr(vk, name), getattr(key, name), len(getattr(key, name)))
    arrays = (key.vs.slice(0, diff), key.ws.slice(0, diff), key.ys.slice(0, diff))
    vk.vs_io, vk.ws_io, vk.ys_io = (a._h for a in arrays)
    lib = _lib.lib
    crossover = None
    for n in ns:
        raw = (_lib.Phgr13Proof * n)()
        for i in range(n):
            for f in api.PHGR13Proof.FIELDS:
                C.memmove(getattr(raw[i], f), getattr(distinct[i % DISTINCT], f), len(getattr(distinct[i % DISTINCT], f)))
        io = api.Poly.upload(ctx, [v for i in range(n) for v in made[i % DISTINCT][1][:diff]])
        ios = [io.slice(i * diff, diff) for i in range(n)]
        rho = b"".join(((rng.fr() >> 127) or 1).to_bytes(32, "big") for _ in range(n))
        ok = C.c_int(0)
        verdicts = {}

        def batch():
            rc = lib.ps_phgr13_verify_batch(ctx._h, C.byref(vk), io._h, raw, n, rho, C.byref(ok))
            assert rc == 0, lib.ps_last_error()
            verdicts["batch"] = ok.value

        def loop():
            good = 0
            for i in range(n):
                rc = lib.ps_phgr13_verify(ctx._h, C.byref(vk), ios[i]._h, C.byref(raw[i]), C.byref(ok))
                assert rc == 0, lib.ps_last_error()
                good += ok.value
            verdicts["loop"] = good

        batch()  # warm: buffers sized, code objects loaded
        tb = [_timed(batch) for _ in range(reps)]
        ctx.set_timing(True)
        batch()
        ctx.set_timing(False)
        ms = (C.c_float * len(STAGES))()
        assert lib.ps_debug_phgr13_verify_batch_stage_ms(ctx._h, ms) == 0
        info = api.PHGR13VerifyBatchInfo(ctx)
        loop_reps = 1 if n >= 1024 else min(reps, 3)
        if n < 1024:
            loop()
        tl = [_timed(loop) for _ in range(loop_reps)]
        assert verdicts == {"batch": 1, "loop": n}, verdicts
        mb, ml = statistics.median(tb), statistics.median(tl)
        if crossover is None and mb < ml:
            crossover = n
        split = " ".join(f"{name} {v:.2f}" for name, v in zip(STAGES, ms))
        print(f"gates {gates:<3d} diff {diff:<3d} N={n:<5d} batch ms {_stat(tb)} = {mb / n * 1e3:10.1f} us/proof | loop ms {_stat(tl)} = {ml / n * 1e3:8.1f} us/proof"
              f" ({loop_reps} rep) | loop/batch {ml / mb:7.2f}x | device loops {info['device_loops']} | timed call, ms: {split} (sum {sum(ms):.2f})", flush=True)
        for s in ios:
            s.free()
        io.free()
    print(f"gates {gates}: the batch is faster than the loop from N = {crossover} on (of the sizes measured)", flush=True)
    q.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, nargs="*", default=[7, 64])
    ap.add_argument("--n", type=int, nargs="*", default=[1, 16, 64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x70766273)
    print(f"# library {os.path.basename(_lib.library_path())}; batch: {args.reps} repetitions, median (min .. max); stages of one timed call: "
          + ", ".join(STAGES), flush=True)
    for g in args.gates:
        rows_for(ctx, rng, g, args.n, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
