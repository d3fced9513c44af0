"""The field arithmetic as the GPU runs it, against big integers, at the edges of the lazy-limb contract.

tests/host_limb_check.cpp drives field.hpp's products with worst-case limbs ON THE HOST, where every product compiles to its
C++ form.  The device runs other code: the generated multiply-add chains (fp_chain.inc, fr_chain.inc -- the Fr one a different
algorithm, in the negated domain), the lane-pair Fp2s with its DPP moves, the noinline products.  Here:
  * CPU: the generated files are what their generators print; both builds of tests/device_field_check.hip cross-compile and
    the chain build really contains the chains; the Python emulation (tests/field_model.py) equals the host-compiled C++
    forms bit for bit, and no column accumulator of any product form leaves 64 bits anywhere inside the contract;
  * GPU: every operation on worst-case, edge and random lazy operands -- the residue is the big-integer answer, the output
    lands in its stated range, and the limbs equal the emulation (and the other build) bit for bit; the bucket chain of the
    group law over Fp and over Fp2s; the NTT butterflies as the shipped pass kernel sequences them, 32 stages deep.
The device program runs as a subprocess with a time limit, so a fault in a test kernel fails one test."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_model as fm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "playsnark_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "device_field_check.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/lib/llvm/bin"
# the product's flags (playsnark_amd/csrc/Makefile), without -fPIC -shared: an executable
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function"]
NO_CHAIN = ["-DPS_FP_MUL_NO_CHAIN", "-DPS_FR_MUL_NO_CHAIN"]
NRAND = 1 << 14
P, R = fm.P, fm.R


# ---------------------------------------------------------------------------------------------------------------------------
# builds and runs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_field")
    procs = {}
    for name, extra in (("chain", []), ("nochain", NO_CHAIN)):
        procs[name] = subprocess.Popen([HIPCC, *FLAGS, *extra, SRC, "-o", str(d / name)], stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT, text=True)
    for name, p in procs.items():
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, f"{name} build failed:\n{out[-4000:]}"
    return {k: str(d / k) for k in procs}


def run(exe, op, arr, timeout=300):
    """One run of the device program: a failed run is reported, never retried."""
    arr = np.asarray(arr, dtype=np.int64)
    assert arr.min() >= -(1 << 31) and arr.max() < (1 << 31)
    n = arr.shape[0]
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        arr.astype(np.int32).tofile(fin)
        res = subprocess.run([exe, op, str(n), fin, fout], capture_output=True, text=True, timeout=timeout)
        assert res.returncode == 0, f"{op}: exit status {res.returncode}\n{res.stdout[-1000:]}{res.stderr[-2000:]}"
        return np.fromfile(fout, dtype=np.int32).astype(np.int64).reshape(n, -1)


def ints(a):
    """Row values of limb arrays (exact Python ints)."""
    a = np.asarray(a, dtype=np.int64)
    w = np.array([1 << (fm.B * i) for i in range(a.shape[-1])], dtype=object)
    return list((a.astype(object) * w).sum(axis=-1))


def assert_rows(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} cases differ, first {bad[0]}: got {list(got[bad[0]])} want {list(want[bad[0]])}"


def cat(*xs):
    return np.concatenate([np.asarray(x, dtype=np.int64) for x in xs], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# operand sets (seeded: every run checks the same cases)
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


def fp_worst_set(classes, rng, patterns=16):
    """Every class tuple x 16 sign patterns: operand j gets pattern (p >> 2j) & 3 rotated, the host check's scheme."""
    rows = []
    for cl in classes:
        for p in range(patterns):
            rows.append(sum((fm.worst(c, ((p >> (2 * (j % 2))) + j) & 3, rng) for j, c in enumerate(cl)), []))
    return np.array(rows, dtype=np.int64)


def fp_random_set(classes, n, rng, L=fm.FP_L, top=fm.TOP_SPAN):
    per = -(-n // len(classes))
    blocks = [cat(*[fm.random_lazy(c, per, rng, L, top) for c in cl]) for cl in classes]
    return np.concatenate(blocks)[:n]


def mul_classes(limit, nops=2, maxc=8):
    """Class tuples (c_a1, c_b1, c_a2, c_b2, ...) whose class products add up to <= limit."""
    out = []

    def rec(prefix, budget):
        if len(prefix) == 2 * nops:
            out.append(tuple(prefix))
            return
        for ca in range(1, maxc + 1):
            for cb in range(1, maxc + 1):
                rest = nops - len(prefix) // 2 - 1
                if ca * cb + rest <= budget:
                    rec(prefix + [ca, cb], budget - ca * cb)

    rec([], limit)
    return out


def fp_edges():
    e = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, -1, -P, -P + 1, 16 * P - 1, -16 * P + 1, (P - 1) // 2, 1 << 380, (1 << 364) - 1]
    return np.array([fm.from_int(v, fm.FP_L) for v in e], dtype=np.int64)


def edge_pairs(edges):
    n = len(edges)
    return cat(np.repeat(edges, n, axis=0), np.tile(edges, (n, 1)))


def product_sets(nops, limit, square=False):
    """Worst-case, edge and random operand sets of a product of nops operand pairs (class products adding up to limit)."""
    rng = _rng(f"prod{nops}{limit}{square}")
    if square:
        cls = [(c,) for c in range(1, 9) if c * c <= limit]
        worst = fp_worst_set(cls, rng)
        rand = fp_random_set(cls, NRAND, rng)
        edges = fp_edges()
        return np.concatenate([worst, edges, rand])
    cls = mul_classes(limit, nops)
    if nops == 4:
        cls = [c for c in cls if sum(c[2 * j] * c[2 * j + 1] for j in range(4)) == limit or c == (1,) * 8][:160]
    worst = fp_worst_set(cls, rng)
    edges = fp_edges()
    ep = edge_pairs(edges)
    if nops > 1:
        ep = np.concatenate([ep] * nops, axis=1)
    rand = fp_random_set(cls, NRAND, rng)
    return np.concatenate([worst, ep, rand])


def split(x, L=fm.FP_L):
    return [x[:, L * j:L * (j + 1)] for j in range(x.shape[1] // L)]


MONT_INV_P = pow(fm.FP_RM, -1, P)
MONT_INV_R = pow(fm.FR_RM, -1, R)


def check_fp_product_output(out, sums, what, single=True):
    """sums: the exact integer S = sum (+/-) a b of every case.  The result must be the Montgomery reduction of S itself:
    V = (S + M p) / R with 0 <= M < R (so V = S R^-1 mod p, and V lies in (S/R, S/R + p)); limbs 0..12 in [0, 2^28); for a
    single product (|A|, |B| <= 16 p) the value in (-p/8, 9p/8), field.hpp's documented output."""
    vals = ints(out)
    for i, (v, s) in enumerate(zip(vals, sums)):
        m, rem = divmod(v * fm.FP_RM - s, P)
        assert rem == 0, f"{what}: wrong residue in case {i}"
        assert 0 <= m < fm.FP_RM, f"{what}: case {i} is not one Montgomery reduction of its column sums (M = {m})"
    assert (out[:, :-1] >= 0).all() and (out[:, :-1] <= fm.MASK).all(), f"{what}: a limb 0..12 outside [0, 2^28)"
    lo, hi = min(vals), max(vals)
    if single:
        assert -P // 8 < lo and hi < 9 * P // 8, f"{what}: value outside (-p/8, 9p/8): [{lo / P:.4f} p, {hi / P:.4f} p]"


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen,inc", [("gen_fp_chain.py", "fp_chain.inc"), ("gen_fr_chain.py", "fr_chain.inc")])
def test_generated_chains_match_their_generators(gen, inc):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen)], capture_output=True, timeout=120, check=True).stdout
    with open(os.path.join(CSRC, inc), "rb") as f:
        assert out == f.read(), f"{inc} is not what tools/{gen} prints: regenerate it (python3 tools/{gen} > playsnark_amd/csrc/{inc})"


def _kernel_mads(exe, tmp):
    shutil.copy(exe, os.path.join(tmp, "x"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "x"], cwd=tmp, check=True, capture_output=True)
    co = [f for f in os.listdir(tmp) if f.endswith("gfx950")]
    assert len(co) == 1, os.listdir(tmp)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co[0]], cwd=tmp, check=True,
                         capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.strip():
            funcs[cur].append(line.split("//")[0].strip())
    return funcs


def test_both_builds_compile_and_the_chain_build_uses_the_chains(binaries, tmp_path):
    """A build-flag slip would otherwise test the C++ form twice."""
    (tmp_path / "c").mkdir()
    (tmp_path / "n").mkdir()
    chain, nochain = _kernel_mads(binaries["chain"], str(tmp_path / "c")), _kernel_mads(binaries["nochain"], str(tmp_path / "n"))

    def mads(funcs, name):
        return sum("v_mad_i64_i32" in ins for ins in funcs[name])

    k_mul, k_call, k_fr = "_Z6k_caseI7OpFpMulEvPKiPii", "_Z6k_caseI11OpFpMulCallEvPKiPii", "_Z6k_caseI7OpFrMulEvPKiPii"
    fn_call = "_ZN2ps11fp_mul_callENS_2FpES0_"
    for f in (chain, nochain):
        assert all(k in f for k in (k_mul, k_call, k_fr, fn_call)), sorted(f)[:20]
    # the chains: Fp 196 operand + 196 modulus multiply-adds, Fr 100 + 90 (no r_0 term); the launch's own index arithmetic
    # is what the (out-of-line) fp_mul_call case kernel holds
    base = mads(chain, k_call)
    assert mads(chain, fn_call) == 392
    assert mads(chain, k_mul) - base == 392
    assert mads(chain, k_fr) - base == 190
    assert chain[k_mul] != nochain[k_mul] and chain[fn_call] != nochain[fn_call] and chain[k_fr] != nochain[k_fr]
    assert mads(nochain, k_mul) != mads(chain, k_mul) and mads(nochain, k_fr) != mads(chain, k_fr)


@pytest.fixture(scope="module")
def host_eval(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_eval") / "host_field_eval")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host_field_eval.cpp"), "-o", exe], check=True, capture_output=True, timeout=600)
    return exe


def _fp_emul(op, x, dtype=np.int64, track=False):
    s = split(x)
    if op in ("fp_mul", "fp_mul_ilp"):
        f = fm.fp_mulsum_ilp if op.endswith("ilp") else fm.fp_mulsum
        return f([(s[0], s[1], False)], track, dtype)
    if op == "fp_sqr":
        return fm.fp_sqr(s[0], track, dtype)
    if op in ("fp_mul2sub", "fp_mul2add", "fp_mul2sub_ilp"):
        f = fm.fp_mulsum_ilp if op.endswith("ilp") else fm.fp_mulsum
        return f([(s[0], s[1], False), (s[2], s[3], op != "fp_mul2add")], track, dtype)
    if op in ("fp_mul2add2sub", "fp_mulsum_ilp4"):
        f = fm.fp_mulsum_ilp if op.endswith("ilp4") else fm.fp_mulsum
        return f([(s[0], s[1], False), (s[2], s[3], False), (s[4], s[5], True), (s[6], s[7], True)], track, dtype)
    raise KeyError(op)


def _fp_want(op, x):
    v = [ints(y) for y in split(x)]
    k = len(v) // 2
    sg = {"fp_mul2sub": [1, -1], "fp_mul2sub_ilp": [1, -1], "fp_mul2add": [1, 1], "fp_mul2add2sub": [1, 1, -1, -1],
          "fp_mulsum_ilp4": [1, 1, -1, -1]}.get(op, [1])
    if op == "fp_sqr":
        return [a * a for a in v[0]]
    return [sum(sg[j] * v[2 * j][i] * v[2 * j + 1][i] for j in range(k)) for i in range(len(v[0]))]


FP_PRODUCTS = {  # op: (operand pairs, class-product budget, square)
    "fp_mul": (1, 8, False), "fp_sqr": (1, 8, True), "fp_mul2sub": (2, 8, False), "fp_mul2add": (2, 8, False),
    "fp_mul2add2sub": (4, 8, False), "fp_mul_ilp": (1, 8, False), "fp_mul2sub_ilp": (2, 8, False),
    "fp_mulsum_ilp4": (4, 8, False),
}


def test_emulation_matches_host_cpp_forms(host_eval, tmp_path):
    """The model against field.hpp compiled for the host (the C++ forms), bit for bit, on the worst-case sets and a slice
    of the random ones -- the emulation is anchored before any GPU time is spent."""
    for op, (nops, lim, sq) in FP_PRODUCTS.items():
        x = product_sets(nops, lim, sq)[:4000]
        got = _run_host(host_eval, op, x, tmp_path)
        assert_rows(got, _fp_emul(op, x)[0], f"host {op} vs emulation")
    rng = _rng("frhost")
    x = np.concatenate([fr_worst_set(rng), fp_random_set(FR_CLASSES, 4000, rng, fm.FR_L, fm.FR_TOP_SPAN)])
    got = _run_host(host_eval, "fr_mul", x, tmp_path)
    s = split(x, fm.FR_L)
    assert_rows(got, fm.fr_mul_cpp(s[0], s[1])[0], "host fr_mul vs emulation")
    x = fp_random_set([(8,)], 2000, rng)
    assert_rows(_run_host(host_eval, "fp_norm", x, tmp_path), fm.norm(x), "host f_norm vs emulation")


def _run_host(exe, op, x, tmp):
    fin, fout = str(tmp / "in"), str(tmp / "out")
    np.asarray(x, dtype=np.int32).tofile(fin)
    subprocess.run([exe, op, str(len(x)), fin, fout], check=True, capture_output=True, timeout=600)
    return np.fromfile(fout, dtype=np.int32).astype(np.int64).reshape(len(x), -1)


FR_CLASSES = [(a, b) for a in range(1, 8) for b in range(1, 8) if a * b <= 11]


def fr_worst_set(rng):
    rows = []
    for ca, cb in FR_CLASSES:
        for p in range(16):
            rows.append(fm.fr_worst(ca, p & 3, rng) + fm.fr_worst(cb, p >> 2, rng))
    return np.array(rows, dtype=np.int64)


def test_column_accumulators_stay_inside_64_bits(capsys):
    """Largest |column accumulator| of every product form: exactly, over the worst-case sets in the device's term order, and
    as an upper bound over the whole contract.  Both below 2^63; the margin is printed (pytest -s)."""
    lines = []
    for op, (nops, lim, sq) in FP_PRODUCTS.items():
        rng = _rng(f"peak{op}")
        if sq:
            x = fp_worst_set([(1,), (2,)], rng)
        else:
            cls = mul_classes(lim, nops)
            if nops == 4:
                cls = [c for c in cls if sum(c[2 * j] * c[2 * j + 1] for j in range(4)) == lim][:40]
            x = fp_worst_set(cls, rng)
        _, peak = _fp_emul(op, x, dtype=object, track=True)
        bound = fm.column_bound(fm.FP_L, fm.FP_MOD, lim)
        assert peak < fm.I64_LIM and bound < fm.I64_LIM, (op, peak, bound)
        lines.append(f"{op:16s} worst-case peak {peak / 2**63:.4f} x 2^63   contract bound {bound / 2**63:.4f} x 2^63")
    x = fr_worst_set(_rng("peakfr"))
    s = split(x, fm.FR_L)
    for name, f in (("fr_mul chain", fm.fr_mul_chain), ("fr_mul C++", fm.fr_mul_cpp)):
        _, peak = f(s[0], s[1], track=True, dtype=object)
        bound = fm.column_bound(fm.FR_L, fm.FR_MOD, 11)
        assert peak < fm.I64_LIM and bound < fm.I64_LIM, (name, peak, bound)
        lines.append(f"{name:16s} worst-case peak {peak / 2**63:.4f} x 2^63   contract bound {bound / 2**63:.4f} x 2^63")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the products
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", list(FP_PRODUCTS) + ["fp_mul_call", "fp_sqr_call"])
def test_fp_products_on_device(binaries, op):
    base = {"fp_mul_call": "fp_mul", "fp_sqr_call": "fp_sqr"}.get(op, op)
    nops, lim, sq = FP_PRODUCTS[base]
    x = product_sets(nops, lim, sq)
    got = run(binaries["chain"], op, x)
    ref = run(binaries["nochain"], op, x)
    want = _fp_emul(base, x)[0]
    assert_rows(got, want, f"{op}: chain build vs emulation")
    assert_rows(ref, want, f"{op}: C++ form on the device vs emulation")
    # the column-parallel forms equal the product-scanning ones bit for bit (field.hpp's claim)
    if base.endswith("ilp") or base.endswith("ilp4"):
        scan = {"fp_mul_ilp": "fp_mul", "fp_mul2sub_ilp": "fp_mul2sub", "fp_mulsum_ilp4": "fp_mul2add2sub"}[base]
        assert_rows(got, run(binaries["chain"], scan, x), f"{op} vs {scan} on the device")
    check_fp_product_output(got, _fp_want(base, x), op, single=nops == 1)


@pytest.mark.gpu
def test_fp_cheap_operations_on_device(binaries):
    rng = _rng("fpcheap")
    lazy = np.concatenate([fp_worst_set([(c,) for c in range(1, 9)], rng), fp_random_set([(c,) for c in range(1, 9)], NRAND, rng)])
    vals = ints(lazy)
    # fp_propagate adds the carry to a limb in 32 bits: a class-8 limb (up to 2^31 - 1) plus a carry leaves int32, so its
    # domain (and fp_canon's) is class <= 7; f_norm takes the whole class-8 range
    le7 = fm.limb_class(lazy) <= 7
    for op, want, sel in (("fp_norm", fm.norm(lazy), np.ones(len(lazy), bool)), ("fp_propagate", fm.propagate(lazy), le7)):
        for b in ("chain", "nochain"):
            got = run(binaries[b], op, lazy)
            assert_rows(got, want, f"{op} ({b})")
            assert [v for v, k in zip(ints(got), sel) if k] == [v for v, k in zip(vals, sel) if k], f"{op} changed a value"
    assert (fm.limb_class(fm.norm(lazy)) <= 2).all()
    # canonical form for V in (-2p, 3p)
    spread = [int.from_bytes(rng.bytes(56), "little") % (5 * P) - 2 * P + 1 for _ in range(2048)]
    cv = np.array(fm.canon_edges(P, fm.FP_L, rng) + [fm.relayout(fm.from_int(v, fm.FP_L), 4, rng) for v in spread], dtype=np.int64)
    want = np.array([fm.from_int(v % P, fm.FP_L) for v in ints(cv)], dtype=np.int64)
    for b in ("chain", "nochain"):
        assert_rows(run(binaries[b], "fp_canon", cv), want, f"fp_canon ({b})")
    # zero tests: every k p edge, the filter boundaries, and random lazy values (non-zero)
    z = np.concatenate([np.array(fm.fp_zero_edges(rng), dtype=np.int64), lazy[:4096]])
    assert (fm.limb_class(z) <= 8).all() and max(abs(v) for v in ints(z)) <= 16 * P
    want = np.array([[1 if v % P == 0 else 0] for v in ints(z)], dtype=np.int64)
    assert want.sum() >= 33
    for b in ("chain", "nochain"):
        assert_rows(run(binaries[b], "fp_is_zero", z), want, f"f_is_zero ({b})")
        assert_rows(run(binaries[b], "fp_is_zero_exact", z), want, f"fp_is_zero_exact ({b})")
    # Montgomery conversions
    plain = np.concatenate([fp_edges()[[0, 1, 2, 3, 13]], fm.random_canon(2048, rng)])
    want = np.array([fm.from_int(v * fm.FP_RM % P, fm.FP_L) for v in ints(plain)], dtype=np.int64)
    assert_rows(run(binaries["chain"], "fp_to_mont", plain), want, "fp_to_mont")
    want = np.array([fm.from_int(v * MONT_INV_P % P, fm.FP_L) for v in ints(lazy)], dtype=np.int64)
    assert_rows(run(binaries["chain"], "fp_from_mont", lazy), want, "fp_from_mont")


def _fp2_cases(rng, cls):
    """Fp2 operands (c0, c1), one limb class per operand (both components): worst-case limbs under 16 sign patterns
    (each component its own), then random lazy ones."""
    worst = np.array([sum((fm.worst(c[k], ((p >> (2 * (k % 2))) + j) & 3, rng) for k in range(len(c)) for j in range(2)), [])
                      for c in cls for p in range(16)], dtype=np.int64)
    rand = fp_random_set([tuple(c[k] for k in range(len(c)) for _ in range(2)) for c in cls], 4096, rng)
    return np.concatenate([worst, rand])


def _f2(x, k):  # operand k of Fp2 cases: (c0, c1) limb arrays
    return x[:, 28 * k:28 * k + 14], x[:, 28 * k + 14:28 * k + 28]


def _f2_int(c0, c1):
    return list(zip(ints(c0), ints(c1)))


def _f2_mul(a, b):  # exact, unreduced
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


@pytest.mark.gpu
def test_fp2_karatsuba_on_device(binaries):
    rng = _rng("fp2")
    x = _fp2_cases(rng, [(a, b) for a in range(1, 9) for b in range(1, 9)])
    a, b = _f2(x, 0), _f2(x, 1)
    an, bn = [fm.norm(c) for c in a], [fm.norm(c) for c in b]
    t0, t1 = fm.fp_mul(an[0], bn[0])[0], fm.fp_mul(an[1], bn[1])[0]
    s = fm.fp_mul(fm.add(an[0], an[1]), fm.add(bn[0], bn[1]))[0]
    want = cat(fm.norm(fm.sub(t0, t1)), fm.norm(fm.sub(fm.sub(s, t0), t1)))
    got = run(binaries["chain"], "fp2_mul", x)
    assert_rows(got, want, "Fp2 f_mul vs emulation")
    assert_rows(run(binaries["nochain"], "fp2_mul", x), want, "Fp2 f_mul (C++ form)")
    for g, u, v in zip(_f2_int(got[:, :14], got[:, 14:]), _f2_int(*a), _f2_int(*b)):
        assert (g[0] % P, g[1] % P) == tuple(c * MONT_INV_P % P for c in _f2_mul(u, v)), "Fp2 f_mul: wrong residue"
    assert (fm.limb_class(got[:, :14]) <= 2).all() and (fm.limb_class(got[:, 14:]) <= 2).all()
    x1 = x[:, :28]
    a0, a1 = fm.norm(x1[:, :14]), fm.norm(x1[:, 14:])
    m = fm.fp_mul(a0, a1)[0]
    want = cat(fm.fp_mul(fm.add(a0, a1), fm.sub(a0, a1))[0], fm.norm(fm.add(m, m)))
    got = run(binaries["chain"], "fp2_sqr", x1)
    assert_rows(got, want, "Fp2 f_sqr vs emulation")
    for g, u in zip(_f2_int(got[:, :14], got[:, 14:]), _f2_int(x1[:, :14], x1[:, 14:])):
        assert (g[0] % P, g[1] % P) == tuple(c * MONT_INV_P % P for c in _f2_mul(u, u)), "Fp2 f_sqr: wrong residue"


def _fp2s_expect(op, x):
    """Per lane, what the lane-pair form computes: even lane c0, odd lane c1 of the Fp2 result, limb for limb."""
    ops = [_f2(x, k) for k in range(x.shape[1] // 28)]
    if op == "fp2s_mul" or op == "fp2s_mul_ilp":
        (a0, a1), (b0, b1) = ops
        even = fm.fp_mulsum([(a0, b0, False), (fm.i32(-a1), b1, False)])[0]
        odd = fm.fp_mulsum([(a1, b0, False), (a0, b1, False)])[0]
    elif op == "fp2s_sqr":
        (a0, a1), = ops
        n0, n1 = fm.norm(a0), fm.norm(a1)
        even = fm.fp_mul(fm.add(n0, n1), fm.sub(n0, n1))[0]
        odd = fm.fp_mul(fm.add(n1, n1), n0)[0]
    else:  # fp2s_mul2sub(_ilp): a b - c d after f_norm of every operand
        (a0, a1), (b0, b1), (c0, c1), (d0, d1) = [(fm.norm(p), fm.norm(q)) for p, q in ops]
        even = fm.fp_mulsum([(a0, b0, False), (fm.i32(-a1), b1, False), (c0, d0, True), (fm.i32(-c1), d1, True)])[0]
        odd = fm.fp_mulsum([(a1, b0, False), (a0, b1, False), (c1, d0, True), (c0, d1, True)])[0]
    return cat(even, odd)


def _fp2s_want(op, x):
    v = [_f2_int(*_f2(x, k)) for k in range(x.shape[1] // 28)]
    out = []
    for i in range(x.shape[0]):
        if op == "fp2s_sqr":
            r = _f2_mul(v[0][i], v[0][i])
        elif op in ("fp2s_mul", "fp2s_mul_ilp"):
            r = _f2_mul(v[0][i], v[1][i])
        else:
            p, q = _f2_mul(v[0][i], v[1][i]), _f2_mul(v[2][i], v[3][i])
            r = (p[0] - q[0], p[1] - q[1])
        out.append(r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["fp2s_mul", "fp2s_sqr", "fp2s_mul2sub", "fp2s_mul_ilp", "fp2s_mul2sub_ilp"])
def test_fp2s_on_device(binaries, op):
    """The lane-pair Fp2 (G2 kernels): one case per lane pair, DPP moves live on every lane."""
    rng = _rng(op)
    # f_mul / f_mul_ilp need class(a) class(b) <= 4 (two products per lane); f_sqr and f_mul2sub normalise their operands
    # first (the mixed addition hands f_mul2sub differences of class-2 values)
    if op in ("fp2s_mul", "fp2s_mul_ilp"):
        cls = [(a, b) for a in range(1, 5) for b in range(1, 5) if a * b <= 4]
    elif op == "fp2s_sqr":
        cls = [(a,) for a in range(1, 9)]
    else:
        cls = [(a, b, c, d) for a in (1, 2, 4) for b in (1, 2, 4) for c in (1, 4) for d in (1, 4)]
    x = _fp2_cases(rng, cls)
    got = run(binaries["chain"], op, x)
    want = _fp2s_expect(op, x)
    assert_rows(got, want, f"{op} vs emulation")
    assert_rows(run(binaries["nochain"], op, x), want, f"{op} (C++ form) vs emulation")
    res = _fp2s_want(op, x)
    for j, (g0, g1) in enumerate(_f2_int(got[:, :14], got[:, 14:])):
        assert (g0 % P, g1 % P) == (res[j][0] * MONT_INV_P % P, res[j][1] * MONT_INV_P % P), f"{op}: wrong residue in case {j}"
    check_fp_product_output(got[:, :14], [w[0] for w in res], op + " c0", single=False)
    check_fp_product_output(got[:, 14:], [w[1] for w in res], op + " c1", single=False)


@pytest.mark.gpu
def test_fp2s_is_zero_on_device(binaries):
    rng = _rng("fp2sz")
    z = np.array(fm.fp_zero_edges(rng), dtype=np.int64)
    zero = z[[i for i, v in enumerate(ints(z)) if v % P == 0]]
    nz = z[[i for i, v in enumerate(ints(z)) if v % P != 0]]
    n = min(len(zero), len(nz))
    x = np.concatenate([cat(zero[:n], zero[::-1][:n]), cat(zero[:n], nz[:n]), cat(nz[:n], zero[:n]), cat(nz[:n], nz[::-1][:n])])
    want = np.repeat(np.array([1] * n + [0] * (3 * n))[:, None], 2, axis=1)
    got = run(binaries["chain"], "fp2s_is_zero", x)
    assert_rows(got, want, "Fp2s f_is_zero (both lanes)")


@pytest.mark.gpu
def test_fr_on_device(binaries, capsys):
    rng = _rng("fr")
    x = np.concatenate([fr_worst_set(rng), fp_random_set(FR_CLASSES, NRAND, rng, fm.FR_L, fm.FR_TOP_SPAN)])
    a, b = split(x, fm.FR_L)
    got, ref = run(binaries["chain"], "fr_mul", x), run(binaries["nochain"], "fr_mul", x)
    products = got
    assert_rows(got, fm.fr_mul_chain(a, b)[0], "fr_mul chain vs negated-domain emulation")
    assert_rows(ref, fm.fr_mul_cpp(a, b)[0], "fr_mul C++ form on the device vs emulation")
    vg, vr = ints(got), ints(ref)
    assert vg == vr, "the chain and the C++ form give different values (the same value is expected, in other limbs)"
    want = [u * v * MONT_INV_R % R for u, v in zip(ints(a), ints(b))]
    assert all(g % R == w for g, w in zip(vg, want)), "fr_mul: wrong residue"
    # the device output contract: limbs 0..8 in (-2^28, 0], value in (-r/8, 9r/8)
    assert (got[:, :-1] <= 0).all() and (got[:, :-1] > -(1 << 28)).all()
    lo, hi = min(vg), max(vg)
    assert -R // 8 < lo and hi < 9 * R // 8
    with capsys.disabled():
        print(f"\ndevice fr_mul: limbs 0..8 in [{got[:, :-1].min()}, {got[:, :-1].max()}], top limb in [{got[:, -1].min()}, "
              f"{got[:, -1].max()}], value in [{lo / R:.4f} r, {hi / R:.4f} r]")
    # fr_reduce, fr_norm, fr_propagate, fr_canon
    one = np.array([fm.fr_mont(1)] * len(a), dtype=np.int64)
    assert_rows(run(binaries["chain"], "fr_reduce", a), fm.fr_mul_chain(a, one)[0], "fr_reduce (chain)")
    assert_rows(run(binaries["nochain"], "fr_reduce", a), fm.fr_mul_cpp(a, one)[0], "fr_reduce (C++ form)")
    for op, want in (("fr_norm", fm.norm(a)), ("fr_propagate", fm.propagate(a))):
        got = run(binaries["chain"], op, a)
        assert_rows(got, want, op)
        assert ints(got) == ints(a)
    cv = np.array(fm.canon_edges(R, fm.FR_L, rng), dtype=np.int64)
    cv = np.concatenate([cv, products[:4096], ref[:4096]])
    want = np.array([fm.from_int(v % R, fm.FR_L) for v in ints(cv)], dtype=np.int64)
    assert_rows(run(binaries["chain"], "fr_canon", cv), want, "fr_canon")


def _words(v, n):
    return [((v >> (32 * i)) & 0xFFFFFFFF) - (1 << 32 if (v >> (32 * i)) & 0x80000000 else 0) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("field", ["fp", "fr"])
def test_saturated_forms_on_device(binaries, field):
    """fe_mul (the noinline mont_mul_raw path), fe_add, fe_sub on canonical edges."""
    mod, nw = (P, 12) if field == "fp" else (R, 8)
    rng = _rng("fe" + field)
    edges = [0, 1, 2, mod - 1, mod - 2, (mod - 1) // 2, (mod + 1) // 2, (1 << (32 * nw - 32)) % mod, mod - (1 << 32)]
    vals = edges + [int.from_bytes(rng.bytes(48), "little") % mod for _ in range(512)]
    pairs = [(u, v) for u in edges for v in edges] + list(zip(vals, vals[::-1]))
    x = np.array([_words(u, nw) + _words(v, nw) for u, v in pairs], dtype=np.int64)
    rinv = pow(1 << (32 * nw), -1, mod)
    for op, f in (("mul", lambda u, v: u * v * rinv % mod), ("add", lambda u, v: (u + v) % mod), ("sub", lambda u, v: (u - v) % mod)):
        got = run(binaries["chain"], f"fe_{op}_{field}", x)
        want = np.array([_words(f(u, v), nw) for u, v in pairs], dtype=np.int64)
        assert_rows(got, want, f"fe_{op}<{field}>")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the group law (bucket chains) over Fp and Fp2s
# ---------------------------------------------------------------------------------------------------------------------------
GL_K = 40


def _chains(grp, rng, nchains=8):
    pool = [grp.mul(int.from_bytes(rng.bytes(8), "little") | 1) for _ in range(24)]
    chains = []
    for kind in range(nchains):
        pts = []
        for i in range(GL_K):
            p = pool[int(rng.integers(len(pool)))]
            if i % 7 == 3:
                p = pts[-1]  # a repeat
            pts.append(p)
        if kind == 1:  # acc == P (doubling branch), then acc == -2P (P + (-P)), then from the identity again
            p = pool[0]
            pts[:3] = [p, p, grp.neg(grp.add(p, p))]
        if kind == 2:  # the halves are equal: left + right doubles
            pts[GL_K // 2:] = pts[:GL_K // 2]
        if kind == 3:  # the halves cancel: the sum is the identity, and so is its double
            pts[GL_K // 2:] = [grp.neg(q) for q in pts[:GL_K // 2]]
        if kind == 4:  # P, -P pairs all along
            for i in range(0, GL_K, 4):
                pts[i + 1] = grp.neg(pts[i])
        chains.append(pts)
    return chains


def _xyzz_affine(grp, X, Y, ZZ, ZZZ, f2):
    if f2:
        from oracle import pyref as pr
        if ZZ[0] % P == 0 and ZZ[1] % P == 0:
            return None
        return (pr.f2_mul(X, pr.f2_inv(ZZ)), pr.f2_mul(Y, pr.f2_inv(ZZZ)))
    if ZZ % P == 0:
        return None
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


@pytest.mark.gpu
@pytest.mark.parametrize("g", ["g1", "g2"])
def test_group_law_chains_on_device(binaries, g, capsys):
    from oracle import pyref as pr

    grp, f2 = (pr.G1, False) if g == "g1" else (pr.G2, True)
    rng = _rng("gl" + g)
    chains = _chains(grp, rng)

    def enc(c):
        if f2:
            return fm.fp_mont(c[0]) + fm.fp_mont(c[1])
        return fm.fp_mont(c)

    x = np.array([sum((enc(p[0]) + enc(p[1]) for p in pts), []) for pts in chains], dtype=np.int64)
    out = run(binaries["chain"], f"group_law_{g}", x)
    worst = 0
    for i, pts in enumerate(chains):
        total = None
        for p in pts:
            total = grp.add(total, p)
        want = [total, total, grp.add(total, total)]
        if f2:
            lanes = out[i].reshape(2, -1)
            worst = max(worst, lanes[0, -1], lanes[1, -1])
            assert lanes[0, -1] == lanes[1, -1]
            coords = [(fm.to_int(lanes[0, 14 * j:14 * j + 14]) % P, fm.to_int(lanes[1, 14 * j:14 * j + 14]) % P) for j in range(12)]
        else:
            worst = max(worst, out[i, -1])
            coords = [fm.to_int(out[i, 14 * j:14 * j + 14]) for j in range(12)]
        for j, name in enumerate(("acc", "left + right", "2 acc")):
            got = _xyzz_affine(grp, *coords[4 * j:4 * j + 4], f2)
            assert got == want[j], f"{g} chain {i}: {name} != the oracle's sum"
    assert worst <= 2, f"{g}: a stored coordinate reached limb class {worst}"
    with capsys.disabled():
        print(f"\n{g} bucket chains: stored coordinates at limb class <= {worst}")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the NTT butterflies of the shipped pass kernel (ntt.hpp, ntt_tile_stages + k_ntt_pass's scaling store)
# ---------------------------------------------------------------------------------------------------------------------------
NB_TILE, NB_MAXPASS = 512, 8


def _inv2pow():
    with open(os.path.join(CSRC, "bls12_381_constants.h")) as f:
        txt = f.read()
    body = txt[txt.index("#define PS_FR28_INV2POW"):]
    body = body[:body.index("}}") + 2]
    nums = [int(v) for v in re.findall(r"-?\d+", body.split(" ", 2)[2])]
    return np.array(nums, dtype=np.int64).reshape(-1, fm.FR_L)


class _Limbs:
    """Limb-exact Fr operations on arrays (..., 10); mul is the product the build under test runs."""

    def __init__(self, mul, track):
        self._mul, self.track = mul, track
        self.mul_cls, self.mul_val, self.store_cls, self.store_val = 0, 0.0, 0, 0.0

    def _v(self, a):
        return np.abs((a * (2.0 ** (28 * np.arange(fm.FR_L)))).sum(axis=-1)).max() / R

    def mul(self, a, w):
        sh = a.shape
        self.mul_cls = max(self.mul_cls, int(fm.limb_class(a.reshape(-1, fm.FR_L)).max()))
        self.mul_val = max(self.mul_val, self._v(a))
        return self._mul(a.reshape(-1, fm.FR_L), np.broadcast_to(w, sh).reshape(-1, fm.FR_L))[0].reshape(sh)

    def add(self, a, b):
        return fm.i32(a + b)

    def sub(self, a, b):
        return fm.i32(a - b)

    def norm(self, a):
        r = fm.norm(a.reshape(-1, fm.FR_L)).reshape(a.shape)
        return r

    def stored(self, a):
        self.store_cls = max(self.store_cls, int(fm.limb_class(a.reshape(-1, fm.FR_L)).max()))
        self.store_val = max(self.store_val, self._v(a))
        return a


class _Mod:
    """The reduced recurrence: values mod r, Montgomery products, norm = identity."""

    def mul(self, a, w):
        return a * w * MONT_INV_R % R

    def add(self, a, b):
        return (a + b) % R

    def sub(self, a, b):
        return (a - b) % R

    def norm(self, a):
        return a

    def stored(self, a):
        return a


def _replay(F, inv, passes, T, TW, sc_tab):
    """ntt_tile_stages<INV> for p = k, logD = 0 on every pass, exactly as ntt.hpp issues the butterflies.  T: (cases, 512, ...)
    in logical order e = t * COLS + col; TW: (cases, 512, ...)."""
    T = T.copy()
    for k, logc, scale in passes:
        cols = np.arange(1 << logc)
        rows = 1 << k

        def at(t):
            return (t[:, None] * (1 << logc) + cols[None, :]).reshape(-1)

        def tw(t, m):
            M = k - 1 - m
            if M <= 0:
                return None
            return TW[:, np.repeat((1 << M) + (t >> (m + 1)), 1 << logc)]

        def put(idx, v):
            T[:, idx] = F.stored(v)

        done = 0
        while done < k:
            left = k - done
            if left == 1 or (not inv and left & 1):
                m = done if inv else k - 1 - done
                r = np.arange(rows >> 1)
                t0 = ((r >> m) << (m + 1)) | (r & ((1 << m) - 1))
                t1 = t0 | (1 << m)
                i0, i1 = at(t0), at(t1)
                a, b = T[:, i0], T[:, i1]
                w = tw(t0, m)
                if not inv:
                    wb = F.mul(b, w) if w is not None else b
                    put(i0, F.norm(F.add(a, wb)))
                    put(i1, F.norm(F.sub(a, wb)))
                else:
                    put(i0, F.norm(F.add(a, b)))
                    d = F.norm(F.sub(a, b))
                    put(i1, F.mul(d, w) if w is not None else d)
                done += 1
            else:
                m_lo = done if inv else k - 2 - done
                m_hi = m_lo + 1
                r = np.arange(rows >> 2)
                t00 = ((r >> m_lo) << (m_lo + 2)) | (r & ((1 << m_lo) - 1))
                t01, t10 = t00 | (1 << m_lo), t00 | (1 << m_hi)
                t11 = t10 | (1 << m_lo)
                i00, i01, i10, i11 = at(t00), at(t01), at(t10), at(t11)
                a, b, c, d = T[:, i00], T[:, i01], T[:, i10], T[:, i11]
                if not inv:
                    w = tw(t00, m_hi)
                    if w is not None:
                        c, d = F.mul(c, w), F.mul(d, w)
                    a1, c1, b1, d1 = F.add(a, c), F.sub(a, c), F.add(b, d), F.sub(b, d)
                    wb = F.mul(b1, tw(t00, m_lo))
                    put(i00, F.norm(F.add(a1, wb)))
                    put(i01, F.norm(F.sub(a1, wb)))
                    wd = F.mul(d1, tw(t10, m_lo))
                    put(i10, F.norm(F.add(c1, wd)))
                    put(i11, F.norm(F.sub(c1, wd)))
                else:
                    a1, b1 = F.add(a, b), F.mul(F.norm(F.sub(a, b)), tw(t00, m_lo))
                    c1, d1 = F.add(c, d), F.mul(F.norm(F.sub(c, d)), tw(t10, m_lo))
                    w = tw(t00, m_hi)
                    put(i00, F.norm(F.add(a1, c1)))
                    put(i01, F.norm(F.add(b1, d1)))
                    e, f = F.norm(F.sub(a1, c1)), F.norm(F.sub(b1, d1))
                    put(i10, F.mul(e, w) if w is not None else e)
                    put(i11, F.mul(f, w) if w is not None else f)
                done += 2
        if inv and scale:
            T = F.stored(F.mul(T, sc_tab[scale]))
    return T


def _plan(ks, inv):
    """ntt_run's scaling rule: divide the doubling out in the last pass, earlier only where the next would pass 2^16."""
    out, unscaled = [], 0
    for i, k in enumerate(ks):
        s = 0
        if inv:
            unscaled += k
            nxt = ks[i + 1] if i + 1 < len(ks) else 0
            if i == len(ks) - 1 or unscaled + nxt > 16:
                s, unscaled = unscaled, 0
        out.append((k, 9 - k, s))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("inv", [False, True], ids=["forward", "inverse"])
def test_ntt_butterflies_on_device(binaries, inv, capsys):
    """2^32 points, the deepest transform Fr supports: ntt_run's four passes of 8 stages, and a 9 + 9 + 9 + 5 split (single
    stages, other tile shapes).  Random data and twiddles, canonical Montgomery form."""
    rng = _rng(f"ntt{inv}")
    n = 16
    sc_tab = _inv2pow()
    assert all(fm.to_int(sc_tab[s]) * MONT_INV_R % R == pow(2, -s, R) for s in range(len(sc_tab)))
    sc_int = [fm.to_int(row) for row in sc_tab]
    report = []
    for ks in ([8, 8, 8, 8], [9, 9, 9, 5]):
        plan = _plan(ks, inv)
        TW = fm.random_canon(n * NB_TILE, rng, R, fm.FR_L).reshape(n, NB_TILE, fm.FR_L)
        D = fm.random_canon(n * NB_TILE, rng, R, fm.FR_L).reshape(n, NB_TILE, fm.FR_L)
        hdr = np.zeros((n, 1 + 3 * NB_MAXPASS), dtype=np.int64)
        hdr[:, 0] = len(plan)
        for j, p in enumerate(plan):
            hdr[:, 1 + 3 * j:4 + 3 * j] = p
        x = cat(hdr, TW.reshape(n, -1), D.reshape(n, -1))
        op = "ntt_inverse" if inv else "ntt_forward"
        for build, mul in (("chain", fm.fr_mul_chain), ("nochain", fm.fr_mul_cpp)):
            got = run(binaries[build], op, x).reshape(n, NB_TILE, fm.FR_L)
            F = _Limbs(mul, True)
            want = _replay(F, inv, plan, D, TW, sc_tab)
            assert_rows(got.reshape(-1, fm.FR_L), want.reshape(-1, fm.FR_L), f"{op} {ks} ({build}) vs limb-exact replay")
            # what ntt.hpp relies on: stored values at class <= 2, every product inside fr_mul's contract (class product
            # <= 11 with a class-1 twiddle or scale, |A| |B| <= 2^22 r^2 with |B| < 9r/8)
            assert F.store_cls <= 2 and F.mul_cls <= 11 and F.mul_val * 9 / 8 <= 2**22, (F.store_cls, F.mul_cls, F.mul_val)
            report.append(f"{op} {ks} {build}: stored class <= {F.store_cls}, product operand class <= {F.mul_cls}, "
                          f"|value| <= {F.store_val:.1f} r stored, {F.mul_val:.1f} r into a product")
        vals = np.array([ints(D[c]) for c in range(n)], dtype=object)
        tws = np.array([ints(TW[c]) for c in range(n)], dtype=object)
        ref = _replay(_Mod(), inv, plan, vals, tws, sc_int)
        gv = np.array([ints(got[c]) for c in range(n)], dtype=object) % R
        assert (gv == ref).all(), f"{op} {ks}: residues differ from the reduced recurrence"
    with capsys.disabled():
        print("\n" + "\n".join(report))
