#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X prover hot path.

Metric (BASELINE.json): G1 scalar-muls/s of the Pippenger MSM on 2^20 synthetic BLS12-381 points.
A "step" is one complete MSM (digits -> sort -> bucket accumulation -> reduction -> host fold to
one affine point) over inputs already resident in HBM.  With N > 1 ranks (one process per GPU)
every rank owns an index-range shard, runs the full local MSM, and the ranks exchange their 96-byte
partial sums with one RCCL all_gather followed by a local N-way point addition:
    weak scaling   (default)            2^log2n points per rank
    strong scaling (--total-log2n T)    2^T points in total, 2^T / N per rank (BASELINE config #4: T = 24)

`python3 bench.py --gpus N` is self-sufficient: without WORLD_SIZE in the environment it starts the N
ranks itself (fresh child processes of torch.distributed.run, before this process has touched the GPU)
and relays rank 0's JSON line; under torch.distributed.run it is one of the ranks.

Prints ONE JSON line on rank 0.  A plain run does only what the headline needs: it sets up, warms up, times
--steps pipelined sums and prints `value` and `ms_per_step` (`verified` stays null); --dump-outputs DIR also
writes the sum of the last timed step to DIR/result_affine.npy.  --full adds, outside the timed region,
`ms_per_step_one_at_a_time`, `stage_ms` and `roofline` (dominant kernel = k_accumulate, HBM bound by the
benchmark's convention; the kernel is integer-ALU bound), the verification by discrete
logarithm, `cpu_baseline` (the oracle's CPU Pippenger timed on the host cores ON THE SAME INPUTS, which also
yields `verified`), `ms_per_step_with_h2d` and, at N = 1, `extras`: the secondary workloads
(2^16, 2^24, G2, the witness regime, both provers at 2^20 with the quotient's own roofline).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SEED = 0x706C6179736E61726B & 0xFFFFFFFFFFFFFFFF  # "playsnark"
MAD_PEAK_ROUND1 = 2.82e13  # v_mad_u64_u32 lane-ops/s as measured in round 1 (profiles/r01_microbench_valu.txt); the line carries the
                           # value ps_microbench_mad measures in THIS run and keeps this one beside it
MADS_PER_MIXED_ADD = {"g1": 3542, "g2": 2 * 5292}  # 8M+2S: 6*392 + 588 + 2*301; G2 per lane of a pair: 6*588 + 980 + 2*392
HBM_PEAK_GBS = 8000.0                             # MI355X_MICROARCH.md: 8 TB/s spec
BYTES_PER_SCALAR_MUL = {"g1": 96 + 32, "g2": 192 + 32}  # one affine point + one scalar
ACC_KERNEL = {"g1": "k_accumulate<Fp>", "g2": "k_accumulate<Fp2s>"}
PMC_FILE = {"g1": "pmc_accumulate.json", "g2": "pmc_accumulate_g2.json"}  # rocprofv3 --pmc passes of the accumulation kernels (tools/collect_profiles.sh)
FR_MADS_PER_BUTTERFLY = 200                        # one 10-limb Montgomery product (field.hpp fr_mul)
FR_BYTES = 40                                      # device layout of one Fr element (10 x 28-bit limbs)
SINGLE_REPS = 10  # sums of the one-at-a-time and seam-S1 legs (means; outside the timed region)
FR_ALGO_BYTES = 32                                 # algorithmic bytes per element and transform = 2 * K * 32 B


def uniform_scalars_be32(n: int, seed: int):
    """n scalars uniform in [0, r) as big-endian 32-byte rows (rejection sampling, numpy)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    r_rows = np.frombuffer(R_MOD.to_bytes(32, "big"), dtype=np.uint8)
    out = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    while True:
        # lexicographic compare against r
        diff = out.astype(np.int16) - r_rows.astype(np.int16)
        nz = diff != 0
        first = nz.argmax(axis=1)
        lead = diff[np.arange(n), first]
        bad = (lead > 0) | (~nz.any(axis=1))
        nbad = int(bad.sum())
        if nbad == 0:
            return out
        out[bad] = rng.integers(0, 256, size=(nbad, 32), dtype=np.uint8)


def witness_values(n: int, seed: int):
    """int64 values as the reference's Vector holds them (regime ii)."""
    import numpy as np

    rs = np.random.RandomState(seed % (1 << 32))
    w = rs.randint(0, 1 << 40, size=n, dtype=np.int64)
    kind = rs.randint(0, 20, size=n)
    w[kind < 2] = 0
    w[(kind >= 2) & (kind < 4)] = 1
    w[kind >= 15] *= -1
    return w


# ---------------------------------------------------------------------------------------------------------
# Verification that needs neither the oracle nor a second GPU pass: the synthetic points are P_i = a_i * G with the
# a_i known on the host, so  sum_i k_i P_i = (sum_i a_i k_i mod r) * G  -- the reference's own test method
# (groth16_test.go:41-106 recomputes discrete logs from the retained toxic waste).  One fixed-base multiplication in
# plain Python integers (affine chord-and-tangent over Fp / Fp2, public BLS12-381 constants), independent of both the
# product and oracle/.  Works for any rank count: every rank checks its own partial sum, rank 0 the folded one.
# ---------------------------------------------------------------------------------------------------------
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G1_GEN = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
          0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2_GEN = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
           0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
          (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
           0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


class _Fp:
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % P_MOD)
    sub = staticmethod(lambda a, b: (a - b) % P_MOD)
    mul = staticmethod(lambda a, b: a * b % P_MOD)
    inv = staticmethod(lambda a: pow(a, -1, P_MOD))
    to_b = staticmethod(lambda a: a.to_bytes(48, "big"))


class _Fp2:  # Fp[u] / (u^2 + 1), elements (c0, c1); wire order c1 || c0 (the ZCash / kyber serialisation)
    zero, one = (0, 0), (1, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % P_MOD, (a[1] + b[1]) % P_MOD))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % P_MOD, (a[1] - b[1]) % P_MOD))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P_MOD, (a[0] * b[1] + a[1] * b[0]) % P_MOD))
    to_b = staticmethod(lambda a: a[1].to_bytes(48, "big") + a[0].to_bytes(48, "big"))

    @staticmethod
    def inv(a):
        d = pow(a[0] * a[0] + a[1] * a[1], -1, P_MOD)
        return (a[0] * d % P_MOD, -a[1] * d % P_MOD)


def fixed_base_mul_bytes(group: str, s: int) -> bytes:
    """s * G as the library serialises a point (affine big-endian x || y; the identity is 0x40 followed by zeros)."""
    F, gen = (_Fp, G1_GEN) if group == "g1" else (_Fp2, G2_GEN)
    size = 96 if group == "g1" else 192

    def add(p, q):
        if p is None:
            return q
        if q is None:
            return p
        (x1, y1), (x2, y2) = p, q
        if x1 == x2:
            if F.add(y1, y2) == F.zero:
                return None
            three = F.add(F.add(F.one, F.one), F.one)
            lam = F.mul(F.mul(three, F.mul(x1, x1)), F.inv(F.add(y1, y1)))
        else:
            lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
        x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
        return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))

    acc, base = None, gen
    s %= R_MOD
    while s:
        if s & 1:
            acc = add(acc, base)
        base = add(base, base)
        s >>= 1
    if acc is None:
        return bytes([0x40]) + bytes(size - 1)
    return F.to_b(acc[0]) + F.to_b(acc[1])


def dlog_of_sum(a_be32: bytes, scalars) -> int:
    """sum_i a_i k_i mod r; `scalars` is the big-endian byte string the GPU got, or the list of int64 witness values."""
    n = len(a_be32) // 32
    fb = int.from_bytes
    if isinstance(scalars, (bytes, bytearray)):
        ks = (fb(scalars[32 * i:32 * i + 32], "big") for i in range(n))
    else:
        ks = iter(scalars)
    acc = 0
    for i, k in zip(range(n), ks):
        acc += fb(a_be32[32 * i:32 * i + 32], "big") * k  # (a negative witness value v stands for r - |v|: the same residue)
    return acc % R_MOD


def cpu_baseline(group: str, points_raw: bytes, scalars_be32: bytes, n: int, gpu_result: bytes):
    """Oracle CPU Pippenger (plain-C port, pthreads over windows) on the SAME points and scalars the GPU
    summed (a bounded sample of them when the workload is larger than 2^20).  Returns (block, verified)."""
    from oracle import coracle as co

    og = co.G1 if group == "g1" else co.G2
    cores = os.cpu_count() or 1
    threads = min(cores, 16)
    t0 = time.perf_counter()
    want = og.to_b(og.msm_pippenger(scalars_be32, points_raw, n, threads))
    dt = time.perf_counter() - t0
    verified = None if gpu_result is None else (want == gpu_result)
    return {
        "value": n / dt,
        "unit": "%s scalar-muls/s" % group.upper(),
        "cores": threads,
        "kind": "port",
        "sample": f"one {n}-point {group.upper()} MSM on the same points and scalars as the GPU run (downloaded), oracle C "
                  f"Pippenger (unsigned 16-bit windows, Jacobian, one window per thread), {dt:.2f} s wall = "
                  f"{dt * threads:.0f} core-seconds",
    }, verified


# ---------------------------------------------------------------------------------------------------------
# synthetic R1CS for the prover extras: the toy's gate pattern (Mul, Mul, Add, AddConst; r1cs.go:178-198)
# tiled, each block's result feeding the next block's x.  Variables: const, x, out, then the
# intermediates in creation order; CSR arrays built with numpy, the witness in Python integers mod r.
# ---------------------------------------------------------------------------------------------------------
def synthetic_r1cs(n_gates: int, x0: int = 3):
    import numpy as np

    assert n_gates % 4 == 0 and n_gates >= 4
    nb = n_gates // 4
    nvars = 3 + n_gates - 1  # every gate but the last creates a variable; the last writes `out`
    g = np.arange(n_gates, dtype=np.int64)
    o = np.where(g == n_gates - 1, 2, 3 + g)          # output variable of gate g
    blk = g // 4
    cur = np.where(blk == 0, 1, 3 + 4 * blk - 1)      # x of the block: the input, then the previous block's gate 3
    prev = 3 + g - 1                                   # output of the previous gate (u, v, w inside a block)
    kind = g % 4
    # left rows: kind 0 [cur], 1 [u], 2 [v, cur], 3 [5 const, w]
    l_cnt = np.where(kind >= 2, 2, 1)
    l_ptr = np.concatenate([[0], np.cumsum(l_cnt)]).astype(np.uint32)
    l_col = np.zeros(int(l_ptr[-1]), dtype=np.uint32)
    l_val = np.ones(int(l_ptr[-1]), dtype=np.int64)
    first = l_ptr[:-1].astype(np.int64)
    l_col[first] = np.select([kind == 0, kind == 1, kind == 2], [cur, prev, prev], 0)
    l_val[first[kind == 3]] = 5
    second = first[kind >= 2] + 1
    l_col[second] = np.where(kind[kind >= 2] == 2, cur[kind >= 2], prev[kind >= 2])
    r_ptr = np.arange(n_gates + 1, dtype=np.uint32)
    r_col = np.where(kind <= 1, cur, 0).astype(np.uint32)
    r_val = np.ones(n_gates, dtype=np.int64)
    o_ptr = np.arange(n_gates + 1, dtype=np.uint32)
    o_col = o.astype(np.uint32)
    o_val = np.ones(n_gates, dtype=np.int64)
    sol = [0] * nvars
    sol[0], sol[1] = 1, x0 % R_MOD
    x = sol[1]
    for b in range(nb):
        u = x * x % R_MOD
        v = u * x % R_MOD
        w = (v + x) % R_MOD
        nx = (w + 5) % R_MOD
        base = 3 + 4 * b
        sol[base], sol[base + 1], sol[base + 2] = u, v, w
        if b == nb - 1:
            sol[2] = nx
        else:
            sol[base + 3] = nx
        x = nx
    return nvars, (l_ptr, l_col, l_val), (r_ptr, r_col, r_val), (o_ptr, o_col, o_val), sol


def mul_chain_r1cs(n_gates: int, x0: int = 3):
    """n multiplication gates w_{k+1} = w_k * w_{k-1} (w_0 = w_{-1} = x): BOTH wires of every gate carry full-width
    values, unlike the tiled toy above whose right wire is the constant 1 in half of the gates (which halves the work
    of the G2 sum when the key is in Lagrange form -- the scalars of that sum are the right-wire values).
    Variables: const, x, out, then the products in creation order; the last gate writes `out`."""
    import numpy as np

    nvars = 3 + n_gates - 1
    g = np.arange(n_gates, dtype=np.int64)
    prod = np.where(g == n_gates - 1, 2, 3 + g)               # output variable of gate g
    left = np.where(g == 0, 1, 3 + g - 1)                      # w_k
    right = np.where(g <= 1, 1, 3 + g - 2)                     # w_{k-1}
    ptr = np.arange(n_gates + 1, dtype=np.uint32)
    ones = np.ones(n_gates, dtype=np.int64)
    sol = [0] * nvars
    sol[0], sol[1] = 1, x0 % R_MOD
    a = b = sol[1]
    for k in range(n_gates):
        a, b = a * b % R_MOD, a
        sol[2 if k == n_gates - 1 else 3 + k] = a
    return nvars, (ptr, left.astype(np.uint32), ones), (ptr, right.astype(np.uint32), ones), (ptr, prod.astype(np.uint32), ones), sol


def reference_algorithm_baseline(points_raw: bytes, scalars_be32: bytes):
    """B0 of BASELINE.md section 3: the REFERENCE'S OWN algorithms restated in C (the oracle), one thread, bounded samples.
      B0-msm  Poly.BlindEval's serial loop `acc += Mul(p[i], blindedPoint[i])` (algebra.go:355-357) on 2^12 of the GPU's
              points and scalars: us per term (linear in N) and the scalar-muls/s that extrapolates to;
      B0-h    QAP.Quotient's Mul -> Sub -> Div2 (qap.go:151-162, algebra.go:92-159: schoolbook product, O(n^3) long
              division) on the aggregate polynomials of the tiled toy circuit at n = 2^8 gates.
    The reference is Go with absent dependencies: this is the stand-in, and a conservative one
    (native 64-bit limbs against the Go original's big.Int-backed arithmetic)."""
    from oracle import coracle as co
    from oracle import restate as rs

    n = 1 << 12
    sc = [int.from_bytes(scalars_be32[32 * i:32 * i + 32], "big") for i in range(n)]
    t0 = time.perf_counter()
    co.G1.blind_eval(sc, points_raw[: 96 * n])
    dt = time.perf_counter() - t0
    nq = 1 << 8
    c, sol = rs.synthetic_circuit(nq)
    yA, yB, yC = c.values(sol)
    A, B, Cc, _h = co.fast_quotient(yA, yB, yC)
    z = [1]
    for i in range(1, nq + 1):  # z = prod (x - i), qap.go:57-63
        z = [(( z[k - 1] if k else 0) - i * (z[k] if k < len(z) else 0)) % R_MOD for k in range(len(z) + 1)]
    t0 = time.perf_counter()
    co.quotient_from_aggregates(A, B, Cc, z)
    dq = time.perf_counter() - t0
    return {
        "kind": "port", "cores": 1,
        "msm": {"value": n / dt, "unit": "G1 scalar-muls/s", "us_per_term": dt / n * 1e6,
                "sample": "%d-term serial Mul + Add loop (algebra.go:355-357), %.2f s" % (n, dt)},
        "quotient": {"n_gates": nq, "seconds": dq,
                     "sample": "Mul -> Sub -> Div2 (qap.go:151-162) at n = 2^8 gates; the division is O(n^3): x 2^36 at n = 2^20"},
        "note": "the reference's algorithms (serial MSM, schoolbook product, cubic long division) restated in C, one "
                "thread; the reference itself is Go with absent dependencies and cannot run here (BASELINE.md section 2)",
    }


def quotient_work(n: int):
    """Algorithmic traffic and butterflies of the Groth16-route quotient at n gates:
    per interpolation one convolution of 2^(p+1) and levels 7..p of batched transforms over 2^p elements;
    then five transforms of 2^(p+1) for the product and the division.  One read + one write of 32 B per element and
    transform (SURVEY 8d's figure; the device layout is 40 B)."""
    p = max(6, (n - 1).bit_length())
    np_ = 1 << p
    elems = 2 * (2 * 2 * np_ + sum(2 * np_ for _ in range(7, p + 1))) + 5 * 2 * np_
    bfly = 2 * (2 * np_ * (p + 1) + sum(np_ * logs for logs in range(7, p + 1))) + 5 * np_ * (p + 1)
    return elems * 2 * FR_ALGO_BYTES, bfly


def launch_ranks(args) -> int:
    """No WORLD_SIZE and --gpus N > 1: start N fresh ranks and relay rank 0's JSON line.  This process has
    made no torch.cuda / HIP call, and the ranks are children, not a re-exec."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line:
        print(line)
    elif proc.returncode == 0:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        return 1
    return proc.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2n", type=int, default=20, help="weak scaling: points per GPU = 2^log2n")
    ap.add_argument("--total-log2n", type=int, default=0,
                    help="strong scaling: 2^T points in total, sharded by index range over the GPUs (config #4: 24)")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--slice", type=int, default=0)
    ap.add_argument("--group", choices=["g1", "g2"], default="g1", help="g2 is a side measurement, not the headline metric")
    ap.add_argument("--in-flight", type=int, choices=[1, 2, 3, 4], default=4,
                    help="sums kept in flight per GPU (k: step i+k-1 is enqueued before step i is folded)")
    ap.add_argument("--scalars", choices=["uniform", "witness"], default="uniform",
                    help="uniform: 255-bit scalars (the headline); witness: int64 values as the reference's Vector holds "
                         "them -- small, a tenth zeros, a tenth ones, a quarter negative (SURVEY 8d, regime ii)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for --gpus > 1 (gloo + PS_BENCH_DEVICE=0 rehearses the multi-rank "
                         "path on a one-GPU box; the driver's runs use nccl = RCCL)")
    ap.add_argument("--table-window", type=int, default=0, help="window bits of the table (0 = the library's choice)")
    ap.add_argument("--no-table", action="store_true",
                    help="do not build the window table 2^(c w) P of the resident points (ps_points_precompute): the plain plan")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, measure and check what it does not need: the one-at-a-time and host-upload legs, "
                         "per-stage times and rooflines, verification by discrete logarithm, the CPU baselines and the secondary "
                         "workloads (the last two can be left out with --no-cpu-baseline / --no-extras)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary workloads (N = 1 only)")
    ap.add_argument("--cpu-sample-log2", type=int, default=20, help="CPU baseline: at most 2^k of the GPU's points (default: the full 2^20 workload)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the sum the last one computed to DIR/result_affine.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={env_world} but --gpus {args.gpus}: launch with matching values")
    if "PS_BENCH_DEVICE" in os.environ:  # rehearsal on a one-GPU box: every rank on the same device
        local_rank = int(os.environ["PS_BENCH_DEVICE"])
    dist = None
    world = 1
    devices = [local_rank]
    backend_used = None
    # torch carries the exchange between ranks only: one rank leaves it unloaded (the library has its own HIP runtime)
    if env_world > 1:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
        torch.cuda.set_device(local_rank)
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend_used = args.backend
        if args.backend == "nccl":
            try:
                import datetime

                dist.init_process_group("nccl", rank=rank, world_size=env_world, device_id=torch.device("cuda", local_rank),
                                        timeout=datetime.timedelta(seconds=180))
                probe = torch.zeros(1, dtype=torch.uint8, device=torch.device("cuda", local_rank))
                dist.all_reduce(probe)  # the communicator is built here, not at init: fail now, on every rank alike
            except Exception as e:  # RCCL unavailable between these devices: the exchange is 96 bytes per sum, gloo carries it
                print(f"bench.py rank {rank}: RCCL init failed ({type(e).__name__}: {e}); falling back to gloo", file=sys.stderr)
                if dist.is_initialized():
                    dist.destroy_process_group()
                os.environ["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + 1)
                dist.init_process_group("gloo", rank=rank, world_size=env_world)
                backend_used = "gloo (RCCL init failed)"
        else:
            dist.init_process_group("gloo", rank=rank, world_size=env_world)
        world = dist.get_world_size()
        assert world == args.gpus, (world, args.gpus)
        devices = [None] * world
        dist.all_gather_object(devices, local_rank)

    from playsnark_amd import api
    from playsnark_amd.dist import ShardedMsm, shard_range

    if api.device_count() == 0:
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    ctx = api.Context(local_rank)
    if args.window:
        ctx.set_window(args.window)
    if args.slice:
        ctx.set_slice(args.slice)
    strong = args.total_log2n > 0
    if strong:
        n_total = 1 << args.total_log2n
        _first, n = shard_range(n_total, rank, world)  # this rank's index range of the global vector
    else:
        n = 1 << args.log2n
        n_total = n * world
    g = args.group
    # synthetic inputs, resident in HBM before the timed region:
    #   points  P_i = a_i * G from the device fixed-base kernel (a_i uniform, seeded per rank)
    #   scalars uniform in [0, r)
    host_a = uniform_scalars_be32(n, SEED + 1000 + rank).tobytes()
    a = api.Poly.upload(ctx, host_a)
    gid = api.G1 if g == "g1" else api.G2
    points = api.Points.from_scalars(ctx, gid, a)
    if not args.no_table and not args.window:  # the CRS is fixed across proofs: its window table is built once, like the upload
        points.precompute(args.table_window)
    if args.scalars == "uniform":
        host_scalars = uniform_scalars_be32(n, SEED + 2000 + rank).tobytes()
        scalars = api.Poly.upload(ctx, host_scalars)
    else:
        host_values = witness_values(n, SEED + 3000 + rank).tolist()
        host_scalars = None
        scalars = api.Poly.from_values(ctx, host_values)
    ctx.sync()
    msm = ShardedMsm(ctx, gid, dist, world)

    def barrier():
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        ctx.sync()

    result = None
    if args.warmup:
        result = msm.run_pipelined(points, scalars, max(args.warmup, args.in_flight), depth=args.in_flight)
    if args.full:
        # one-at-a-time latency and kernel time, outside the timed region (reported beside the pipelined figures)
        ctx.set_timing(True)
        for _ in range(2):  # (the first timed sum creates the context's stage events: not part of a steady-state latency)
            msm.run(points, scalars)
        barrier()
        t0 = time.perf_counter()
        single_acc_ms = 0.0
        for _ in range(SINGLE_REPS):
            local_result = msm.run(points, scalars)
            single_acc_ms += ctx.last_stage_ms()["accumulate"] / SINGLE_REPS
        single_ms = (time.perf_counter() - t0) / SINGLE_REPS * 1e3  # (every run returns its result: nothing is left to wait for)
        barrier()
        # the same with the scalars coming from host memory inside the step (pageable memory, PCIe): seam S1 itself,
        # ps_msm_be32 / ps_msm_i64 as the shim's BlindEvalHIP calls it
        import numpy as np

        host_arg = host_scalars if host_scalars is not None else np.asarray(host_values, dtype=np.int64)
        h2d_result = api.blind_eval_host(ctx, points, host_arg)  # (first call: sizes the context's upload vector)
        barrier()
        t0 = time.perf_counter()
        for _ in range(SINGLE_REPS):
            h2d_result = api.blind_eval_host(ctx, points, host_arg)
        h2d_ms = (time.perf_counter() - t0) / SINGLE_REPS * 1e3
        barrier()
    stage_ms = {k: 0.0 for k in api.Context.STAGES}

    def add_stage_times():
        for k, v in ctx.last_stage_ms().items():
            stage_ms[k] += v

    barrier()
    t0 = time.perf_counter()
    # per-stage event timing (--full) stays on through the timed steps, as the roofline reads it from them
    result = msm.run_pipelined(points, scalars, args.steps, add_stage_times if args.full else None, depth=args.in_flight)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend_used == "nccl" else "cpu")  # (after a fallback the group is gloo whatever --backend said)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, result)
    info = ctx.last_msm_info()

    if args.full:
        stage_ms = {k: v / args.steps for k, v in stage_ms.items()}
        ctx.set_timing(False)
        # ---- verification by discrete logarithm, for ANY rank count (outside the timed region): every rank checks the partial
        # sum of its own shard, rank 0 the folded result of the timed run ----
        s_rank = dlog_of_sum(host_a, host_scalars if host_scalars is not None else host_values)
        api.msm_launch(ctx, points, scalars)
        my_partial = api.msm_finish(ctx, gid)  # this rank's sum before any exchange
        want_rank = fixed_base_mul_bytes(g, s_rank)
        mine = (s_rank, bool(my_partial == want_rank and h2d_result == want_rank))  # (the seam-S1 call above summed the same inputs)
        per_rank = [mine]
        if dist is not None:
            per_rank = [None] * world
            dist.all_gather_object(per_rank, mine)

    if rank == 0:
        total_muls = float(n_total) * args.steps
        value = total_muls / elapsed
        W, c = info["windows"], info["window_bits"]
        adds = info["entries"] + 2 * info["buckets"] + c * (W - 1) + W
        shape = ("2^%d points in total over %d GPU(s)" % (args.total_log2n, world)) if strong else ("2^%d points per GPU" % args.log2n)
        exchange = ""
        if world > 1 and backend_used != "nccl":  # a number whose exchange did NOT run over RCCL must say so where it is read
            exchange = " (gloo exchange%s)" % (": RCCL init failed" if "failed" in str(backend_used) else "")
        line = {
            "metric": "%s scalar-muls/s (Pippenger MSM, %s)%s" % (
                g.upper(), ("2^%d pts total" % args.total_log2n) if strong else ("2^%d pts per GPU" % args.log2n), exchange),
            "value": value,
            "unit": "%s scalar-muls/s" % g.upper(),
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "i32x14 (381-bit Fp, 28-bit unsaturated limbs, Montgomery)",
            "data": "synthetic",
            "config": {
                "workload": "BLS12-381 %s MSM, %s, %s" % (
                    g.upper(), shape,
                    "uniform 255-bit scalars" if args.scalars == "uniform" else "int64 witness scalars (zeros, ones, negatives)"),
                "points_per_gpu": n,
                "window_bits": c,
                "windows": W,
                "window_table": bool(points.table_window) and not args.window,
                "window_table_bytes": (255 // points.table_window + 1) * n * (128 if g == "g1" else 256) if points.table_window else 0,
                "slice": info["slice"],
                "in_flight": args.in_flight,
                "sharding": "index range per rank, all_gather of %d-B partial sums" % (96 if g == "g1" else 192) if world > 1 else "single GPU",
                "devices": devices,
                "backend": (backend_used if world > 1 else None),
            },
            "%s_adds_per_s" % g: adds * world * args.steps / elapsed,
            "result_affine_hex": result.hex()[:32] + "...",
            "verified": None,
        }
        if args.full:
            acc_ms = stage_ms["accumulate"]
            bytes_per_mul = BYTES_PER_SCALAR_MUL[g]
            achieved = n * bytes_per_mul / (acc_ms * 1e-3) / 1e9 if acc_ms > 0 else 0.0
            traffic, traffic_source = None, None
            pmc_name = PMC_FILE.get(g)
            pmc_path = os.path.join(ROOT, "profiles", pmc_name) if pmc_name else ""
            if pmc_name and os.path.exists(pmc_path) and not strong and args.log2n == 20 and args.scalars == "uniform":
                try:
                    pmc = json.load(open(pmc_path))
                    traffic = pmc.get("hbm_bytes_per_launch")
                    traffic_source = "rocprofv3 --pmc passes recorded in profiles/%s (%s); not re-measured by this run" % (
                        pmc_name, pmc.get("measured_at", "round 1"))
                except Exception:
                    traffic = None
            # ~1 ms, outside the timed region, on the printing rank only: the integer roofline measured in this run.  A failed or
            # empty measurement must not cost the line its headline number: fall back to round 1's figure and say so.
            mad_peak_source = "ps_microbench_mad in this run (v_mad_u64_u32, 8 chains per lane, 2 waves per SIMD, all CUs)"
            try:
                mad_peak = float(ctx.microbench_mad())
            except Exception as e:  # noqa: BLE001
                mad_peak = 0.0
                mad_peak_source = "round-1 microbenchmark (ps_microbench_mad failed in this run: %s)" % type(e).__name__
            if not mad_peak > 0.0:
                mad_peak = MAD_PEAK_ROUND1
                if "failed" not in mad_peak_source:
                    mad_peak_source = "round-1 microbenchmark (ps_microbench_mad measured no interval in this run)"
            line.update({
                "ms_per_step_one_at_a_time": single_ms,
                "scalar_muls_per_s_one_at_a_time": float(n_total) / (single_ms * 1e-3),  # N / t for ONE MSM
                "ms_per_step_with_h2d": h2d_ms,
                "h2d_note": "seam S1 (ps_msm_be32 / ps_msm_i64, what the shim's BlindEvalHIP calls): one sum at a time with its scalars "
                            "uploaded from pageable host memory inside the call (%d B each, ~0.6 ms of PCIe per 2^20 that nothing can "
                            "hide: the sort needs every digit; points stay resident); `value` never includes it.  Like ms_per_step_one_at_a_time: the "
                            "mean of %d calls in a row, each returning its result" % (8 if args.scalars == "witness" else 32, SINGLE_REPS),
                "stage_ms": stage_ms,
                "stage_note": "per-sum stage times; with in_flight > 1 the stages of neighbouring sums overlap, so they add up to more than ms_per_step",
                "roofline": {
                    "kernel": ACC_KERNEL[g],
                    "kernel_ms": acc_ms,
                    "bound": "hbm",
                    "achieved": achieved,
                    "peak": HBM_PEAK_GBS,
                    "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS,
                    "kernel_ms_one_at_a_time": single_acc_ms,
                    "frac_one_at_a_time": (n * bytes_per_mul / (single_acc_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if single_acc_ms > 0 else 0.0,
                    "traffic": traffic,
                    "traffic_source": traffic_source,
                    # the roofline that actually binds: v_mad_u64_u32 issue rate, measured on
                    # this chip by tools/microbench_valu.hip; one mixed addition = 3 542 multiply-adds (G1)
                    "int_alu": {
                        "mads_per_launch": info["entries"] * MADS_PER_MIXED_ADD[g],
                        "peak_mads_per_s": mad_peak,
                        "peak_source": mad_peak_source,
                        "peak_mads_per_s_round1": MAD_PEAK_ROUND1,
                        "frac": info["entries"] * MADS_PER_MIXED_ADD[g] / (acc_ms * 1e-3) / mad_peak if acc_ms > 0 else 0.0,
                        "frac_one_at_a_time": info["entries"] * MADS_PER_MIXED_ADD[g] / (single_acc_ms * 1e-3) / mad_peak
                        if single_acc_ms > 0 else 0.0,
                        "note": "mads counts this formulation (14 x 28-bit limbs, 392 per product; 3 542 per mixed addition): "
                                "utilisation of the multiplier by THIS representation, not a distance to an algorithmic floor",
                    },
                    "note": "integer-ALU bound by construction (SURVEY 8d): `frac` is the HBM convention of the contract, the binding "
                            "roofline is `int_alu`.  `traffic` / algorithmic bytes = 9.8 is the gather of 13 table rows of 128 B per "
                            "scalar (one per window; the windows share one bucket set) -- inherent to the plan, 0.6-1.1 TB/s, not binding",
                },
            })
            ranks_ok = [bool(ok) for _s, ok in per_rank]
            folded_ok = bool(result == fixed_base_mul_bytes(g, sum(sr for sr, _ok in per_rank) % R_MOD))
            line["verified_dlog"] = {
                "ranks": ranks_ok, "folded": folded_ok,
                "note": "P_i = a_i G with the a_i known on the host: each rank's partial sum == (sum a_i k_i mod r) G over its shard, and the "
                        "folded result of the timed run == (sum over all ranks) G; plain-integer fixed-base multiplication in bench.py "
                        "(groth16_test.go:41-106's method), no oracle, no second GPU pass",
            }
            line["verified"] = all(ranks_ok) and folded_ok
            if not args.no_cpu_baseline and world == 1:  # the CPU leg is timed on rank 0 of the one-GPU run only
                ns = min(n, 1 << args.cpu_sample_log2)
                sample_pts, sample_sc = points.slice(0, ns), scalars.slice(0, ns)
                gpu_sample = local_result if ns == n else sample_sc.BlindEval(sample_pts)
                block, verified = cpu_baseline(g, sample_pts.download(), sample_sc.download_bytes(), ns, gpu_sample)
                line["cpu_baseline"] = block
                line["cpu_baseline_reference_algorithm"] = reference_algorithm_baseline(sample_pts.download(0, 1 << 12),
                                                                                       sample_sc.download_bytes(0, 1 << 12)) if ns >= 1 << 12 and g == "g1" else None
                line["verified"] = bool(verified) and line["verified"]
                line["verified_note"] = "GPU sum == oracle CPU Pippenger on the same %d points and scalars (affine bytes), and verified_dlog" % ns
            if not args.no_extras and world == 1 and not strong:
                line["extras"] = extras(api, ctx, args, mad_peak)
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


def dump_outputs(out_dir: str, result: bytes):
    """What the timed path hands its caller, for comparing two builds output for output: the affine sum of the last timed
    step as the library serialises it (x || y big-endian, 96 B for G1, 192 B for G2), one float64 per byte (exact)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "result_affine.npy"), np.frombuffer(result, dtype=np.uint8).astype(np.float64))


def extras(api, ctx, args, mad_peak):
    """Secondary workloads, each a few steps, one GPU: the sizes and regimes BASELINE.json lists beside the
    headline (configs #2, #4, the G2 sum, the witness regime) and both provers at 2^20 constraints (configs
    #3, #5) with the quotient's own roofline.  Not part of `value`."""
    out = {}

    def msm_ms(gid, n, seed, steps, witness=False, in_flight=4):
        a = api.Poly.upload(ctx, uniform_scalars_be32(n, seed).tobytes())
        pts = api.Points.from_scalars(ctx, gid, a)
        if not args.no_table and not args.window:
            pts.precompute(args.table_window)
        a.free()
        sc = (api.Poly.from_values(ctx, witness_values(n, seed + 1).tolist()) if witness
              else api.Poly.upload(ctx, uniform_scalars_be32(n, seed + 1).tobytes()))
        ctx.sync()
        from playsnark_amd.dist import ShardedMsm

        m = ShardedMsm(ctx, gid, None, 1)
        m.run_pipelined(pts, sc, in_flight, depth=in_flight)
        ctx.sync()
        t0 = time.perf_counter()
        m.run_pipelined(pts, sc, steps, depth=in_flight)
        ctx.sync()
        ms = (time.perf_counter() - t0) / steps * 1e3
        one = 1e9
        for _ in range(3 if n > 1 << 20 else 8):  # a lone sum, best of a few (the first call after the pipelined leg re-plans)
            t0 = time.perf_counter()
            m.run(pts, sc)
            one = min(one, (time.perf_counter() - t0) * 1e3)
        info = ctx.last_msm_info()
        pts.free()
        sc.free()
        return {"ms_per_step": ms, "ms_one_at_a_time": one, "scalar_muls_per_s": n / (ms * 1e-3),
                "scalar_muls_per_s_one_at_a_time": n / (one * 1e-3), "window_bits": info["window_bits"],
                "windows": info["windows"], "slice": info["slice"], "window_table": bool(info["window_table"]), "steps": steps}

    out["g1_msm_2p16"] = msm_ms(api.G1, 1 << 16, SEED + 11, 20)   # BASELINE config #2
    out["g1_msm_2p10"] = msm_ms(api.G1, 1 << 10, SEED + 15, 30)
    out["g2_msm_2p10"] = msm_ms(api.G2, 1 << 10, SEED + 16, 30)
    # the plain plan: what a caller gets who passes a fresh point array (no ps_points_precompute, no 1.7 GB table)
    saved, args.no_table = args.no_table, True
    out["g1_msm_2p20_plain_plan"] = msm_ms(api.G1, 1 << 20, SEED + 17, 10)
    out["g1_msm_2p16_plain_plan"] = msm_ms(api.G1, 1 << 16, SEED + 18, 20)
    args.no_table = saved
    out["g1_msm_2p24"] = msm_ms(api.G1, 1 << 24, SEED + 12, 4)
    out["g2_msm_2p20"] = msm_ms(api.G2, 1 << 20, SEED + 13, 6)
    out["g1_msm_2p20_witness_int64"] = msm_ms(api.G1, 1 << 20, SEED + 14, 20, witness=True)

    # ---- both provers at 2^20 constraints: CRS made on the device, three public values ----
    import random

    n = 1 << 20
    nvars, L, Rm, O, sol = synthetic_r1cs(n)
    q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    rnd = random.Random(SEED)
    fr = lambda: rnd.randrange(1 << 20, R_MOD)
    dsol = api.Poly.upload(ctx, sol)
    tr, vk = api.NewGroth16TrustedSetup(q, fr(), fr(), fr(), fr(), fr())
    r, s = fr(), fr()
    def timed_g16(key):
        api.Groth16Prove(key, q, dsol, r, s)  # warm-up (workspaces, cached concatenations, window tables)
        ph = []
        t0 = time.perf_counter()
        for _ in range(3):
            pf = api.Groth16Prove(key, q, dsol, r, s)
            ph.append(ctx.last_prove_phase_ms())
        return (time.perf_counter() - t0) / 3 * 1e3, ph, pf

    # the key as the reference's NewGroth16TrustedSetup makes it (monomial arrays: the prover interpolates and divides) ...
    mono_ms, mono_phases, mono_proof = timed_g16(tr.monomial_only())
    # ... and with the Lagrange-form arrays the device setup also emits (values on the nodes are the scalars)
    g16_ms, phases, proof = timed_g16(tr)
    assert (proof.A, proof.B, proof.C) == (mono_proof.A, mono_proof.B, mono_proof.C)
    io = api.Poly.upload(ctx, sol[:3])
    ok = api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], proof, io)
    t0 = time.perf_counter()
    api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], proof, io)
    g16_verify_ms = (time.perf_counter() - t0) * 1e3
    # the quotient alone (Groth16 route: A, B coefficient vectors and h), device-synchronous call
    q.computeAB(dsol)
    t0 = time.perf_counter()
    for _ in range(3):
        q.computeAB(dsol)
    quot_ms = (time.perf_counter() - t0) / 3 * 1e3
    qbytes, bfly = quotient_work(n)
    out["groth16_prove_2p20"] = {
        "ms": g16_ms, "phase_ms": {k: sum(p[k] for p in phases) / 3 for k in phases[0]}, "verified_by_pairing": bool(ok),
        "verify_ms": g16_verify_ms,
        "key": "Lagrange-form CRS arrays from the device setup (ps_groth16_pk.lxi / lxi2 / lxi_t): no interpolation, no division",
        "circuit_note": "the tiled toy circuit: half of its right-wire values are the constant 1, which with this key halves the G2 sum's "
                        "work; see groth16_prove_2p20_mul_gates for a circuit whose wires are all full-width",
        "monomial_key": {"ms": mono_ms, "phase_ms": {k: sum(p[k] for p in mono_phases) / 3 for k in mono_phases[0]},
                         "note": "the key as the reference's setup makes it; same proof bytes"},
        "quotient": {
            "ms": quot_ms,
            "algorithmic_bytes": qbytes, "achieved_GBps": qbytes / (quot_ms * 1e-3) / 1e9,
            "frac_hbm": qbytes / (quot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "butterflies": bfly, "frac_mad_peak": bfly * FR_MADS_PER_BUTTERFLY / (quot_ms * 1e-3) / mad_peak,
            "device_bytes": qbytes * FR_BYTES // FR_ALGO_BYTES,
            "note": "algorithmic bytes at SURVEY 8d's 32 B per element and transform (one read + one write; the device layout is 40 B: "
                    "device_bytes); the passes are bound by instruction issue (DESIGN.md section 6)",
        },
    }
    del tr, vk, proof
    ek, pvk = api.NewPHGR13TrustedSetup(q, *[fr() for _ in range(8)])
    def timed_phgr(key):
        api.PHGR13Prove(key, q, dsol)
        t0 = time.perf_counter()
        for _ in range(3):
            pf = api.PHGR13Prove(key, q, dsol)
        return (time.perf_counter() - t0) / 3 * 1e3, pf

    ph_mono_ms, _ = timed_phgr(ek.monomial_only())
    ph_ms, pp = timed_phgr(ek)
    io_arrays = (pvk.vs.slice(0, 3), pvk.ws.slice(0, 3), pvk.ys.slice(0, 3))
    ok = api.PHGR13Verify(ctx, pvk.fixed_points(), *io_arrays, pp, io)
    ph_phase = ctx.last_prove_phase_ms()
    t0 = time.perf_counter()
    api.PHGR13Verify(ctx, pvk.fixed_points(), *io_arrays, pp, io)
    ph_verify_ms = (time.perf_counter() - t0) * 1e3
    out["phgr13_prove_2p20"] = {"ms": ph_ms, "phase_ms": ph_phase, "verified_by_pairing": bool(ok), "verify_ms": ph_verify_ms,
                                "key": "gsi also in Lagrange form (ps_phgr13_ek.lgsi)", "monomial_key": {"ms": ph_mono_ms}}
    del ek, pvk, pp, q, dsol

    # ---- a second 2^20 circuit whose right-wire values are full-width (multiplication gates only): with a Lagrange-form key
    # the scalars of the G2 sum ARE the right-wire values, and the tiled toy above has the constant 1 there in half of its
    # gates, which flatters that route ----
    nvars, L, Rm, O, sol = mul_chain_r1cs(n)
    q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    dsol = api.Poly.upload(ctx, sol)
    tr, vk = api.NewGroth16TrustedSetup(q, fr(), fr(), fr(), fr(), fr())
    mc_mono_ms, mc_mono_ph, _ = timed_g16_on(api, ctx, tr.monomial_only(), q, dsol, r, s)
    mc_ms, mc_ph, mc_proof = timed_g16_on(api, ctx, tr, q, dsol, r, s)
    ok = api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], mc_proof, api.Poly.upload(ctx, sol[:3]))
    avg = lambda ph: {k: sum(p[k] for p in ph) / len(ph) for k in ph[0]}
    out["groth16_prove_2p20_mul_gates"] = {"ms": mc_ms, "phase_ms": avg(mc_ph), "verified_by_pairing": bool(ok),
                                           "monomial_key": {"ms": mc_mono_ms, "phase_ms": avg(mc_mono_ph)},
                                           "note": "2^20 multiplication gates w_{k+1} = w_k w_{k-1}: every left- and right-wire value is full-width"}
    del tr, vk, mc_proof, q, dsol

    # ---- a small circuit: 2^10 constraints of the tiled toy (the short-sum regime: launch- and latency-bound) ----
    ns = 1 << 10
    nvars, L, Rm, O, sol = synthetic_r1cs(ns)
    q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    dsol = api.Poly.upload(ctx, sol)
    tr, vk = api.NewGroth16TrustedSetup(q, fr(), fr(), fr(), fr(), fr())
    sm_mono_ms, _, _ = timed_g16_on(api, ctx, tr.monomial_only(), q, dsol, r, s, reps=10)
    sm_ms, sm_ph, _ = timed_g16_on(api, ctx, tr, q, dsol, r, s, reps=10)
    ek, pvk = api.NewPHGR13TrustedSetup(q, *[fr() for _ in range(8)])
    for _ in range(2):  # tables on the first call, the workers' workspaces on the second
        api.PHGR13Prove(ek, q, dsol)
    laps = []
    for _ in range(10):
        t0 = time.perf_counter()
        api.PHGR13Prove(ek, q, dsol)
        laps.append((time.perf_counter() - t0) * 1e3)
    sm_p_ms = sorted(laps)[len(laps) // 2]
    out["provers_2p10"] = {"groth16_ms": sm_ms, "groth16_phase_ms": avg(sm_ph), "groth16_monomial_key_ms": sm_mono_ms, "phgr13_ms": sm_p_ms,
                           "note": "Groth16: mean of 10 proofs after one warm-up; PHGR13: median of 10 after two"}
    del tr, vk, ek, pvk, q, dsol

    # ---- a reference-made key onto the fast route without the toxic waste: the one-time monomial -> Lagrange conversion of
    # Xi, Xi2, XiT over the group elements (ps_points_monomial_to_lagrange), timed at 2^16 constraints (2^20: ~100 s,
    # profiles/r04_key_to_lagrange.txt), each array compared with the one the setup computed from the toxic waste ----
    nk = 1 << 16
    nvars, L, Rm, O, sol = synthetic_r1cs(nk)
    q = api.QAP.from_csr(ctx, nvars, nvars - 3, L, Rm, O)
    tr, vk = api.NewGroth16TrustedSetup(q, fr(), fr(), fr(), fr(), fr())
    ctx.sync()
    t0 = time.perf_counter()
    conv = tr.monomial_only().with_lagrange(q)
    ctx.sync()
    conv_s = time.perf_counter() - t0
    same = (conv.LXi.download() == tr.LXi.download() and conv.LXi2.download() == tr.LXi2.download()
            and conv.LXiT.download() == tr.LXiT.download())
    out["groth16_key_to_lagrange_2p16"] = {"seconds": conv_s, "byte_identical_to_setup_arrays": bool(same),
                                           "note": "Xi (G1), Xi2 (G2), XiT (G1) of a 2^16-constraint key; once per key"}
    del tr, vk, conv, q

    # ---- the regime the reference itself lives in (Vector = []int, algebra.go:13): 2^20 booleanity gates b*b = b, a witness
    # of random bits uploaded as int64 -- short scalars, and wire values that are all 0 or 1 ----
    import numpy as np

    ptr = np.arange(n + 1, dtype=np.uint32)
    col = np.arange(1, n + 1, dtype=np.uint32)
    val = np.ones(n, dtype=np.int64)
    q = api.QAP.from_csr(ctx, n + 1, n, (ptr, col, val), (ptr, col, val), (ptr, col, val))
    bits = [1] + np.random.RandomState(7).randint(0, 2, size=n).tolist()
    dsol = api.Poly.from_values(ctx, bits)
    tr, vk = api.NewGroth16TrustedSetup(q, fr(), fr(), fr(), fr(), fr())
    g_ms, _, proof = timed_g16_on(api, ctx, tr, q, dsol, r, s)
    ok = api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], proof, api.Poly.from_values(ctx, bits[:1]))
    del tr, vk
    ek, pvk = api.NewPHGR13TrustedSetup(q, *[fr() for _ in range(8)])
    api.PHGR13Prove(ek, q, dsol)
    t0 = time.perf_counter()
    for _ in range(3):
        api.PHGR13Prove(ek, q, dsol)
    p_ms = (time.perf_counter() - t0) / 3 * 1e3
    out["boolean_circuit_2p20_int64_witness"] = {"groth16_ms": g_ms, "phgr13_ms": p_ms, "groth16_verified_by_pairing": bool(ok)}
    return out


def timed_g16_on(api, ctx, key, q, dsol, r, s, reps=3):
    api.Groth16Prove(key, q, dsol, r, s)
    ph = []
    t0 = time.perf_counter()
    for _ in range(reps):
        pf = api.Groth16Prove(key, q, dsol, r, s)
        ph.append(ctx.last_prove_phase_ms())
    return (time.perf_counter() - t0) / reps * 1e3, ph, pf


if __name__ == "__main__":
    main()
