#!/usr/bin/env python3
"""ps_phgr13_verify_batch_locate against what a caller could do before it, in one process, on the same key and context:
    python tools/phgr13_verify_locate_sweep.py [--gates 7 64] [--n 256 1024 4096] [--bad 0 1 16] [--reps 5]  > profiles/phgr13_verify_locate.txt
  (a) loop     ps_phgr13_verify on every proof (structs and input vectors prepared beforehand); once per (gates, N), it
               does not depend on which proofs are bad; one repetition from 1 024 proofs on (it takes seconds there)
  (b) halving  caller-side bisection with ps_phgr13_verify_batch: the batch, then both halves of every rejected set down to
               single proofs (slices of the same proof array, input vector and weights: no copy on the caller's side)
  locate       ps_phgr13_verify_batch_locate
Per (gates, N, b, element): b proofs, evenly spread, get the `element` (vass: one equation; vss: three) of another proof -- a
valid subgroup point in the wrong place.  The three are run INTERLEAVED, repetition by repetition (halving once for b = 16,
where it takes seconds), the stream idle before every timed call (ps_ctx_sync), after one untimed warm-up of each; wall clock
around calls that end with the stream idle; median (min .. max).  For b = 0 the plain ps_phgr13_verify_batch and the locating
call alternate, and the difference of the medians is printed next to the spread of the plain call.
Every answer is checked: the located indices are the tampered ones, the masks are the element's, halving finds the same set.
Proofs: ps_phgr13_prove_batch over 8 values of x0 of the tiled synthetic circuit (diff = gates - 1 public inputs), repeated
to N; weights of 128 bits."""
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

DISTINCT = 8
MASK = {"vass": 0b00010, "vss": 0b10011}
PROOF_BYTES = C.sizeof(_lib.Phgr13Proof)


def _stat(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


class World:
    def __init__(self, ctx, rng, gates):
        self.ctx = ctx
        self.made = [rs.synthetic_circuit(gates, x0=3 + 2 * j) for j in range(DISTINCT)]
        c = self.made[0][0]
        self.diff = c.nbVars - c.nbIO
        self.q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
        ek, key = api.NewPHGR13TrustedSetup(self.q, *[rng.fr() for _ in range(8)])
        self.distinct = api.PHGR13ProveBatch(ek, self.q, api.Poly.upload(ctx, [v for _, s in self.made for v in s]), DISTINCT)
        self.vk = _lib.Phgr13Vk()
        for name in api.PHGR13VerifKey.FIXED:
            C.memmove(getattr(self.vk, name), getattr(key, name), len(getattr(key, name)))
        self.arrays = (key.vs.slice(0, self.diff), key.ws.slice(0, self.diff), key.ys.slice(0, self.diff))
        self.vk.vs_io, self.vk.ws_io, self.vk.ys_io = (a._h for a in self.arrays)
        self.keep = (ek, key)


class Batch:
    """N proofs, `positions` of them with `element` taken from the next distinct proof"""

    def __init__(self, w, rng, n, positions, element):
        self.w, self.n, self.positions = w, n, sorted(positions)
        self.raw = (_lib.Phgr13Proof * n)()
        for i in range(n):
            for f in api.PHGR13Proof.FIELDS:
                C.memmove(getattr(self.raw[i], f), getattr(w.distinct[i % DISTINCT], f), len(getattr(w.distinct[i % DISTINCT], f)))
        for i in positions:
            other = getattr(w.distinct[(i + 1) % DISTINCT], element)
            assert bytes(other) != bytes(getattr(w.distinct[i % DISTINCT], element))
            C.memmove(getattr(self.raw[i], element), other, len(other))
        self.io = api.Poly.upload(w.ctx, [v for i in range(n) for v in w.made[i % DISTINCT][1][:w.diff]])
        self.rho = b"".join(((rng.fr() >> 127) or 1).to_bytes(32, "big") for _ in range(n))
        self.valid, self.failed = C.create_string_buffer(n), C.create_string_buffer(n)
        self.slices = {}

    def proofs_at(self, lo):
        return C.cast(C.addressof(self.raw) + lo * PROOF_BYTES, C.POINTER(_lib.Phgr13Proof))

    def io_slice(self, lo, hi):
        if (lo, hi) not in self.slices:
            self.slices[lo, hi] = self.io.slice(lo * self.w.diff, (hi - lo) * self.w.diff)
        return self.slices[lo, hi]

    def plain(self, lo=0, hi=None):
        hi = self.n if hi is None else hi
        ok = C.c_int(0)
        rc = _lib.lib.ps_phgr13_verify_batch(self.w.ctx._h, C.byref(self.w.vk), self.io_slice(lo, hi)._h, self.proofs_at(lo), hi - lo, self.rho[32 * lo:32 * hi],
                                             C.byref(ok))
        assert rc == 0, _lib.lib.ps_last_error()
        return bool(ok.value)

    def locate(self):
        ninvalid = C.c_size_t(0)
        rc = _lib.lib.ps_phgr13_verify_batch_locate(self.w.ctx._h, C.byref(self.w.vk), self.io_slice(0, self.n)._h, self.raw, self.n, self.rho, self.valid,
                                                    self.failed, C.byref(ninvalid))
        assert rc == 0, _lib.lib.ps_last_error()
        flags = self.valid.raw
        return [i for i in range(self.n) if flags[i] == 0]

    def halving(self):
        """(bad indices, calls of ps_phgr13_verify_batch)"""
        calls, bad, level = 1, [], []
        if not self.plain():
            level = [(0, self.n)]
        while level:
            nxt = []
            for lo, hi in level:
                if hi - lo == 1:
                    bad.append(lo)
                    continue
                mid = lo + (hi - lo + 1) // 2
                for a, b in ((lo, mid), (mid, hi)):
                    calls += 1
                    if not self.plain(a, b):
                        nxt.append((a, b))
            level = nxt
        return sorted(bad), calls

    def loop(self):
        ok = C.c_int(0)
        bad = []
        for i in range(self.n):
            rc = _lib.lib.ps_phgr13_verify(self.w.ctx._h, C.byref(self.w.vk), self.io_slice(i, i + 1)._h, C.byref(self.raw[i]), C.byref(ok))
            assert rc == 0, _lib.lib.ps_last_error()
            if not ok.value:
                bad.append(i)
        return bad

    def free(self):
        for s in self.slices.values():
            s.free()
        self.io.free()


def timed(ctx, fn):
    ctx.sync()  # the stream is idle before the timed call
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def rows_for(ctx, rng, gates, ns, bads, reps):
    w = World(ctx, rng, gates)
    for n in ns:
        loop_ms = None
        for b in bads:
            for element in (("-",) if b == 0 else tuple(MASK)):
                positions = [] if b == 0 else [(2 * k + 1) * n // (2 * b) for k in range(b)]
                batch = Batch(w, rng, n, positions, "vass" if b == 0 else element)
                batch.plain(), batch.locate()  # warm: buffers sized, code objects loaded
                head = f"gates {gates:<3d} diff {w.diff:<3d} N={n:<5d} b={b:<3d} {element:<5s}"
                if b == 0:
                    tp, tl = [], []
                    for _ in range(reps):  # alternating
                        ms, ok = timed(ctx, batch.plain)
                        assert ok is True
                        tp.append(ms)
                        ms, bad = timed(ctx, batch.locate)
                        assert bad == []
                        tl.append(ms)
                    info = api.PHGR13VerifyBatchInfo(ctx)
                    assert info["failed"] == 0
                    d = statistics.median(tl) - statistics.median(tp)
                    print(f"{head} plain ms {_stat(tp)} | locate ms {_stat(tl)} | locate - plain {d:+.2f} ms, spread of the plain call {max(tp) - min(tp):.2f} ms",
                          flush=True)
                    if loop_ms is None:  # (a), once per (gates, N)
                        loop_reps = 1 if n >= 1024 else min(reps, 3)
                        loop_ms = []
                        for _ in range(loop_reps):
                            ms, bad = timed(ctx, batch.loop)
                            assert bad == []
                            loop_ms.append(ms)
                        print(f"gates {gates:<3d} diff {w.diff:<3d} N={n:<5d} (a) loop of ps_phgr13_verify ms {_stat(loop_ms)} ({loop_reps} rep) = "
                              f"{statistics.median(loop_ms) / n * 1e3:.1f} us/proof", flush=True)
                else:
                    tl, th, calls = [], [], 0
                    hreps = 1 if b > 1 else min(reps, 3)
                    for r in range(reps):  # interleaved
                        ms, bad = timed(ctx, batch.locate)
                        assert bad == batch.positions, (bad, batch.positions)
                        assert all(batch.failed.raw[i] == MASK[element] for i in bad)
                        tl.append(ms)
                        if r < hreps:
                            ms, (hbad, calls) = timed(ctx, batch.halving)
                            assert hbad == batch.positions
                            th.append(ms)
                    raw_info = _lib.Phgr13LocateInfo()
                    assert _lib.lib.ps_phgr13_verify_batch_locate_info(ctx._h, C.byref(raw_info)) == 0
                    stage = (C.c_float * 3)()
                    assert _lib.lib.ps_debug_phgr13_verify_locate_ms(ctx._h, stage) == 0
                    ml, mh, ma = statistics.median(tl), statistics.median(th), statistics.median(loop_ms) if loop_ms else float("nan")
                    print(f"{head} locate ms {_stat(tl)} checks {raw_info.checks} products {raw_info.products} (descent: trees {stage[0]:.2f} device {stage[1]:.2f} "
                          f"host {stage[2]:.2f}) | (b) halving ms {_stat(th)} ({hreps} rep, {calls} calls) = {mh / ml:6.1f}x | (a) loop {ma:.0f} ms = {ma / ml:6.1f}x",
                          flush=True)
                batch.free()
    w.q.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, nargs="*", default=[7, 64])
    ap.add_argument("--n", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--bad", type=int, nargs="*", default=[0, 1, 16])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.bad and args.bad[0] == 0, "b = 0 comes first: it measures the loop (a) the other rows compare against"
    ctx = api.Context(0)
    rng = pr.SplitMix64(0x70766c63)
    print(f"# library {os.path.basename(_lib.library_path())}; {args.reps} repetitions, median (min .. max), ms; x = times the locating call", flush=True)
    for g in args.gates:
        rows_for(ctx, rng, g, args.n, args.bad, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
