"""The batch verifier's device side (playsnark_amd/csrc/pairing_dev.hpp, pairing_body.inc over Fp / Fp2) VALUE BY VALUE.

tests/test_pairing_product_gpu.py and tests/test_verify_batch_gpu.py compare verdicts; tests/host_pairing_batch_check.cpp
drives the helpers on the host, where every Fp product is its C++ form.  Here tests/device_pairing_check.hip launches the
shipped kernels directly -- so every lane layout is reachable with a few hundred pairs -- and runs the tower one element per
thread; every value is compared with the same function compiled for the host (limb for limb: the arithmetic is integer) and
with plain Python integers (tests/pairing_model.py, anchored to oracle/pairing.py by a ring homomorphism checked below).
  * CPU: the program cross-compiles and its k_miller_batch is the kernel the library ships (register allocation, spills);
    the model's basis map is a ring homomorphism into the oracle's Fp12; the operand sets and launch shapes hold what they
    claim; the host-compiled miller() raised to (p^12 - 1) / r is the oracle's pairing.
  * GPU: ten tower operations at the lazy-limb edges; Miller loops pair by pair in nine lane layouts; the product tree
    level by level; the weighted column sums at every block and chunk shape.
The device program runs as a subprocess with a time limit; a failed run is reported once and never retried.
Nothing here needs a tolerance."""
import itertools
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
import pairing_model as pm  # noqa: E402
from test_code_object_pairing import PINNED  # noqa: E402
from test_device_field import FLAGS, HIPCC, LLVM, assert_rows, fp_edges  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "device_pairing_check.hip")
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
P, R = fm.P, fm.R
W1, W2, W6, W12 = pm.W1, pm.W2, pm.W6, pm.W12
PAD = 8  # device_pairing_check.hip: elements past the end of an output buffer
POISON = np.int64(np.int32(-0x5A5A5A5B))  # 0xA5A5A5A5
NRAND = 1 << 12


def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


# ---------------------------------------------------------------------------------------------------------------------------
# build and run
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("device_pairing") / "device_pairing_check")
    res = subprocess.run([HIPCC, *FLAGS, SRC, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert res.returncode == 0, f"build failed:\n{res.stdout[-4000:]}"
    return out


def run(exe, op, n, parts, timeout=600):
    """One run of the program (a copy of test_device_field.run for inputs with a header): reported, never retried.
    Returns the flat int32 output as int64."""
    x = np.concatenate([np.asarray(p, dtype=np.int64).ravel() for p in parts])
    assert x.min() >= -(1 << 31) and x.max() < (1 << 32)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        (x & 0xFFFFFFFF).astype(np.uint32).tofile(fin)
        res = subprocess.run([exe, op, str(n), fin, fout], capture_output=True, text=True, timeout=timeout)
        assert res.returncode == 0, f"{op}: exit status {res.returncode}\n{res.stdout[-1000:]}{res.stderr[-2000:]}"
        return np.fromfile(fout, dtype=np.int32).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# tower operations: operands (coefficient counts), the limb classes their contract admits, the reference
# ---------------------------------------------------------------------------------------------------------------------------
# Contracts.  field.hpp: Fp2 f_mul / f_sqr normalise their operands first, so each takes any limb class <= 8; f_norm takes
# class <= 8; an Fp product needs class(a) class(b) <= 8.  Every coefficient holds |V| <= 16 p (the builders' top limb).
#   mul_xi       f_norm(a0 -+ a1): a at class <= 4
#   f2_scale     f_mul(f_norm(a.c), k): a <= 8, and class 2 x class(k) <= 8: k <= 4
#   f2_reduce    f_norm, then a product by one: a <= 8
#   f6_mul, f6_mul_01, f6_mul_1, f12_mul: the raw coefficients go into Fp2 products only: every operand <= 8
#   f12_sqr      f6_norm(a.c0 + a.c1) and f6_norm(a.c0 + v a.c1): a <= 4
#   f12_mul_mem  pairing_dev.hpp: raw coefficients into Fp2 products: <= 8 each (the tree itself feeds class <= 2; the host
#                check runs 2 x 2 and 4 x 1)
#   f12_mul_line as miller() feeds it: f out of f12_sqr or f12_mul_line (f6_norm: class <= 2), la and lb out of f_norm
#                (class <= 2), lc out of f2_scale (a product: class 1)
_ALL = range(1, 9)
OPS = {  # op: (coefficients of every operand, class tuples, output coefficients, largest output class)
    "mul_xi": ((2,), [(c,) for c in range(1, 5)], 2, 2),
    "f2_scale": ((2, 1), [(a, k) for a in _ALL for k in range(1, 5)], 2, 1),
    "f2_reduce": ((2,), [(c,) for c in _ALL], 2, 1),
    "f6_mul": ((6, 6), list(itertools.product(_ALL, _ALL)), 6, 2),
    "f6_mul_01": ((6, 2, 2), list(itertools.product(_ALL, _ALL, _ALL)), 6, 2),
    "f6_mul_1": ((6, 2), list(itertools.product(_ALL, _ALL)), 6, 2),
    "f12_mul": ((12, 12), list(itertools.product(_ALL, _ALL)), 12, 2),
    "f12_sqr": ((12,), [(c,) for c in range(1, 5)], 12, 2),
    "f12_mul_line": ((12, 2, 2, 2), [(f, a, b, 1) for f in (1, 2) for a in (1, 2) for b in (1, 2)], 12, 2),
    "f12_mul_mem": ((12, 12), list(itertools.product(_ALL, _ALL)), 12, 2),
}
NPATTERNS = 16


def _f6(c):  # three Fp2 in memory order are the coefficients of 1, v, v^2
    return list(c)


def reference(op, operands):
    """operands: per operand its Fp2 list in memory order (a lone Fp for f2_scale's k) -> the result's Fp2 list"""
    z = (0, 0)
    if op == "mul_xi":
        return [pm.f2_mul(operands[0][0], pm.XI)]
    if op == "f2_scale":
        return [pm.f2_scale(operands[0][0], operands[1])]
    if op == "f2_reduce":
        return [operands[0][0]]
    if op == "f6_mul":
        return pm.f6_mul(_f6(operands[0]), _f6(operands[1]))
    if op == "f6_mul_01":
        return pm.f6_mul(_f6(operands[0]), [operands[1][0], operands[2][0], z])
    if op == "f6_mul_1":
        return pm.f6_mul(_f6(operands[0]), [z, operands[1][0], z])
    a = pm.f12_from_struct(operands[0])
    if op == "f12_sqr":
        return pm.f12_to_struct(pm.f12_sqr(a))
    if op == "f12_mul_line":
        return pm.f12_to_struct(pm.f12_mul(a, pm.f12_line(operands[1][0], operands[2][0], operands[3][0])))
    return pm.f12_to_struct(pm.f12_mul(a, pm.f12_from_struct(operands[1])))


def tower_cases(op):
    """(worst-case rows, edge rows, random rows): every class tuple under 16 sign patterns (operand j under seed
    ((p >> 2 (j % 2)) + j) & 3 of the host check's rotating scheme); every Fp edge in every coefficient position in turn among
    random canonical coefficients; 2^12 random lazy operands over the class tuples."""
    shape, classes, _, _ = OPS[op]
    rng = _rng("tower" + op)
    worst = np.array([sum((pm.worst_coeffs(k, c, ((p >> (2 * (j % 2))) + j) & 3, rng) for j, (k, c) in enumerate(zip(shape, cl))), [])
                      for cl in classes for p in range(NPATTERNS)], dtype=np.int64)
    ncoef = sum(shape)
    edges = fp_edges()
    base = pm.canon_coeffs(ncoef, ncoef * len(edges), rng)
    for pos in range(ncoef):
        base[pos * len(edges):(pos + 1) * len(edges), pos * W1:(pos + 1) * W1] = edges
    per = -(-NRAND // len(classes))
    rand = np.concatenate([np.concatenate([pm.random_coeffs(k, c, per, rng) for k, c in zip(shape, cl)], axis=1) for cl in classes])[:NRAND]
    return worst, base, rand


def split_operands(op, x):
    out, at = [], 0
    for k in OPS[op][0]:
        out.append(x[:, at:at + k * W1])
        at += k * W1
    assert at == x.shape[1]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Miller pairs and launch shapes
# ---------------------------------------------------------------------------------------------------------------------------
MILLER_SHAPES = [(1, 1), (3, 1), (2, 5), (5, 3), (130, 7), (64, 64), (65, 64), (200, 64), (257, 63)]
# first pair of the pool every shape runs, so that the small shapes meet the edges too
SHAPE_OFFSET = {(1, 1): 0, (3, 1): 7, (2, 5): 10, (5, 3): 12}
NPOOL = 257
# the pool's first sixteen pairs: a, b in {1, 2, r - 1} (index 3 ia + ib), then the edges named here
EDGE_VALUES = (1, 2, R - 1)
I_ID_P, I_ID_Q, I_ID_BOTH, I_PAIR, I_REPEAT, I_NEG, I_OFF = 9, 10, 11, 12, 13, 14, 15
# (shape index, element of that launch) of the 16 pairs that go through the pure-Python oracle: the edges and one pair of
# every shape -- pool indices 0, 7, 8, 9, 10, 11, 12, 13, 14, 15, 5, 129, 63, 64, 199, 256
ORACLE_SUBSET = [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (3, 3), (4, 5), (4, 129), (5, 63),
                 (6, 64), (7, 199), (8, 256)]


def miller_scalars():
    """(a, b) of the pool's pairs; None marks the identity; 'off' the point outside the subgroup"""
    rng = _rng("millerpool")
    draw = lambda: int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1
    out = [(a, b) for a in EDGE_VALUES for b in EDGE_VALUES]
    out += [(None, draw()), (draw(), None), (None, None)]
    a, b = draw(), draw()
    out += [(a, b), (a, b), (R - a, b), ("off", draw())]
    while len(out) < NPOOL:
        out.append((draw(), draw()))
    return out


def _words(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def pair_words(p1, q2):
    """72 canonical words of a pair; the identity is all zero (as the library stores it)"""
    g1 = [0] * 24 if p1 is None else _words(p1[0], 12) + _words(p1[1], 12)
    g2 = [0] * 48 if q2 is None else sum((_words(c, 12) for xy in q2 for c in xy), [])
    return g1 + g2


def miller_points(grp1, grp2, off_g1, only=None):
    """The pool as points of an oracle (grp.mul(k) gives k times the generator); only: the indices wanted (others None)"""
    pts = []
    for i, (a, b) in enumerate(miller_scalars()):
        if only is not None and i not in only:
            pts.append(None)
            continue
        p1 = None if a is None else off_g1 if a == "off" else grp1.mul(a)
        q2 = None if b is None else grp2.mul(b)
        pts.append((p1, q2))
    return pts


F12_ONE_LIMBS = np.array(fm.fp_mont(1) + [0] * (W12 - W1), dtype=np.int64)
FINAL_EXP = (P**12 - 1) // R
# The device's miller() and oracle.pairing.pair() compute f_{|z|,Q}(P) with lines that differ by factors in proper
# subfields of Fp12 (Fp2 scalings of the projective lines, w^3 in Fp4): the final exponentiation removes them, so
# map(miller)^((p^12 - 1) / r) == pair(P, Q) exactly -- power ONE.  Established on the CPU from the host-compiled
# pairing_dev::miller alone (test_host_compiled_miller_is_the_oracles_pairing); never fitted to device output.
NORMALISATION_POWER = 1


def miller_to_gt(limbs168):
    from oracle import pairing as pg

    res = pm.fp_residues(np.asarray(limbs168, dtype=np.int64).reshape(1, W12))[0]
    return pg.f12_pow(pm.struct_residues_to_oracle(res), FINAL_EXP * NORMALISATION_POWER)


# ---------------------------------------------------------------------------------------------------------------------------
# product tree and column shapes
# ---------------------------------------------------------------------------------------------------------------------------
TREE_N = [1, 2, 3, 64, 65, 127, 128, 129, 1000]
TREE_LPW = [1, 3, 64]
COL_ROWS = [1, 15, 16, 17, 63, 64, 65, 4097]
COL_COLS = [1, 5, 255, 256, 257, 1000]
COL_LIMIT = 64 << 20  # bytes of the whole matrix


def column_shapes():
    """(rows, cols, [rows per chunk]): the cross product, without the one matrix above 64 MB (4 097 x 1 000 is 131 MB;
    4 097 rows run with 257 columns -- two grid columns -- and 1 000 columns with 65 rows -- two chunks)"""
    out = []
    for rows in COL_ROWS:
        for cols in COL_COLS:
            if rows * cols * 32 <= COL_LIMIT:
                out.append((rows, cols, list(dict.fromkeys([64, 100, rows]))))
    return out


def column_matrix(rows, cols):
    """(weights, entries) as Python ints below r.  Rows 0 .. 127 have weight r - 1 and every fourth column is r - 1
    throughout: whole chunks of (r - 1)(r - 1), what the every-16-rows fr_reduce has to hold.  The rest is drawn from
    {0, 1, r - 1} and random values."""
    rng = _rng(f"cols{rows}x{cols}")

    def draw(n):
        kind = rng.integers(0, 6, size=n)
        rnd = [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]
        return [0 if k == 0 else 1 if k == 1 else R - 1 if k == 2 else v for k, v in zip(kind, rnd)]

    w = np.array(draw(rows), dtype=object)
    w[:128] = R - 1
    m = np.array(draw(rows * cols), dtype=object).reshape(rows, cols)
    m[:, ::4] = R - 1
    return w, m


def words8(a):
    """object array of ints below 2^256 -> (..., 8) uint32 words as int64"""
    a = np.asarray(a, dtype=object)
    return np.stack([((a >> (32 * i)) & 0xFFFFFFFF).astype(np.int64) for i in range(8)], axis=-1)


def from_words8(x):
    x = (np.asarray(x, dtype=np.int64) & 0xFFFFFFFF).astype(object).reshape(-1, 8)
    return (x * np.array([1 << (32 * i) for i in range(8)], dtype=object)).sum(axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def _kernel_notes(binary, tmp):
    """name -> notes of every kernel of the gfx950 code object in a binary (as tests/test_code_object_pairing.py reads them)"""
    os.makedirs(tmp)
    shutil.copy(binary, os.path.join(tmp, "x"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "x"], cwd=tmp, check=True, capture_output=True)
    co = [f for f in os.listdir(tmp) if f.endswith("gfx950")]
    assert len(co) == 1, os.listdir(tmp)
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count" and cur.get("name"):
            kernels[cur["name"]] = cur
            cur = {}
        cur[key] = val
    if cur.get("name"):
        kernels[cur["name"]] = cur
    return kernels


def _one(notes, name):
    hit = [k for k in notes if name in k]
    assert len(hit) == 1, (name, hit)
    return notes[hit[0]]


def test_program_compiles_and_lists_its_operations(exe):
    out = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out == list(OPS) + ["miller", "tree", "columns"]


def test_the_test_build_runs_the_shipped_miller_kernel(exe, tmp_path):
    """Otherwise the GPU tests could pass on code nobody ships: the test build's k_miller_batch has the library's register
    allocation, and its spills and scratch are inside the bounds pinned for the library's."""
    assert os.path.exists(LIB), "the library has not been built"
    mine, lib = _kernel_notes(exe, str(tmp_path / "t")), _kernel_notes(LIB, str(tmp_path / "l"))
    a, b = _one(mine, "k_miller_batch"), _one(lib, "k_miller_batch")
    assert a["name"] == b["name"]
    assert (int(a["vgpr_count"]), int(a["agpr_count"])) == (int(b["vgpr_count"]), int(b["agpr_count"])) == PINNED["alloc"], (a, b)
    assert int(a["vgpr_spill_count"]) <= PINNED["spills"] and int(a["private_segment_fixed_size"]) <= PINNED["scratch"], a
    for name in ("k_f12_product", "k_fr_weighted_columns"):
        a, b = _one(mine, name), _one(lib, name)
        assert int(a["vgpr_spill_count"]) == int(b["vgpr_spill_count"]) == 0, (name, a, b)


def _random_f12(rng):
    return [(int.from_bytes(rng.bytes(56), "little") % P, int.from_bytes(rng.bytes(56), "little") % P) for _ in range(6)]


def test_basis_map_is_a_ring_homomorphism():
    from oracle import pairing as pg

    rng = _rng("homomorphism")
    for _ in range(50):
        a, b = _random_f12(rng), _random_f12(rng)
        assert pg.f12_mul(pm.to_oracle(a), pm.to_oracle(b)) == pm.to_oracle(pm.f12_mul(a, b))
        assert pg.f12_add(pm.to_oracle(a), pm.to_oracle(b)) == pm.to_oracle([pm.f2_add(x, y) for x, y in zip(a, b)])
    assert pm.to_oracle(pm.F12_ONE) == [1] + [0] * 11
    u = pm.to_oracle([(0, 1)] + [(0, 0)] * 5)
    assert pg.f12_mul(u, u) == [P - 1] + [0] * 11
    # w is w, v = w^2, and the Fp6 product is the Fp12 product on the even powers
    a, b = _random_f12(rng)[:3], _random_f12(rng)[:3]
    z = (0, 0)
    lift = lambda c: [c[0], z, c[1], z, c[2], z]
    assert lift(pm.f6_mul(a, b)) == pm.f12_mul(lift(a), lift(b))
    assert pm.f12_to_struct(pm.f12_from_struct(list(range(6)))) == list(range(6)) and pm.W_POWER == [0, 2, 4, 1, 3, 5]


@pytest.mark.parametrize("op", list(OPS))
def test_operand_sets_hold_every_class_combination_they_claim(op):
    shape, classes, _, _ = OPS[op]
    worst, edges, rand = tower_cases(op)
    seen = {}
    for row in zip(*[pm.coeff_class(o) for o in split_operands(op, worst)]):
        seen[tuple(int(c) for c in row)] = seen.get(tuple(int(c) for c in row), 0) + 1
    assert seen == {tuple(cl): NPATTERNS for cl in classes}, (op, seen)
    # every sign pattern of the first operand's first coefficient under every class tuple: + + .., - - .., alternating, mixed
    signs = {(tuple(int(c) for c in cl), tuple(np.sign(r[:W1 - 1]))) for cl, r in zip(np.repeat(np.array(classes), NPATTERNS, axis=0), worst)}
    assert len(signs) >= 3 * len(classes)  # the fixed patterns; the random one is a fourth
    # limbs AT the class edge, values at the |V| <= 16 p edge
    first = split_operands(op, worst)[0]
    assert (np.abs(first[:, :W1 - 1]).max(axis=1) == (np.array([cl[0] for cl in classes]).repeat(NPATTERNS) << fm.B) - 1).all()
    assert (np.abs(first[:, W1 - 1]) == fm.TOP_SPAN).all()
    ne = len(fp_edges())
    assert len(edges) == sum(shape) * ne
    for pos in range(sum(shape)):
        assert (edges[pos * ne:(pos + 1) * ne, pos * W1:(pos + 1) * W1] == fp_edges()).all()
    assert len(rand) == NRAND
    got = {tuple(int(c) for c in row) for row in zip(*[pm.coeff_class(o) for o in split_operands(op, rand)])}
    # a random operand of few coefficients may fall short of its class edge: never outside the contract, nearly all tuples met
    assert got <= {tuple(cl) for cl in classes} and len(got) >= 0.9 * len(classes), (len(got), len(classes))


def test_miller_launch_shapes_cover_every_lane_layout():
    lpws = {l for _, l in MILLER_SHAPES}
    assert 1 in lpws and 63 in lpws and 64 in lpws and any(l % 2 == 1 and 1 < l < 8 for l in lpws)
    fills = [(n, l) + pm.wave_fill(n, l) for n, l in MILLER_SHAPES]
    assert any(n >= l and last < l for n, l, waves, last in fills if l > 1), "no ragged last wave"
    assert any(last == l for n, l, waves, last in fills if l > 1), "no launch whose last wave holds exactly lpw elements"
    assert any(n < l for n, l, _, _ in fills), "no launch with fewer elements than lanes per wave"
    assert any(l == 64 and waves > 1 and last < 64 for n, l, waves, last in fills), "no ragged last wave at full width"
    # spread_index restated: every element is taken by exactly one thread of the launch
    for n, l in MILLER_SHAPES:
        taken = [w * l + lane for w in range(-(-n // l)) for lane in range(64) if lane < l and w * l + lane < n]
        assert sorted(taken) == list(range(n))
    # the oracle subset: 16 pairs, the edges and one of every shape
    assert len(ORACLE_SUBSET) == 16 and {s for s, _ in ORACLE_SUBSET} == set(range(len(MILLER_SHAPES)))
    pool = [SHAPE_OFFSET.get(MILLER_SHAPES[s], 0) + i for s, i in ORACLE_SUBSET]
    assert all(i < MILLER_SHAPES[s][0] for s, i in ORACLE_SUBSET) and len(set(pool)) == 16
    assert {I_ID_P, I_ID_Q, I_ID_BOTH, I_PAIR, I_REPEAT, I_NEG, I_OFF, 0, 5, 7, 8} <= set(pool)
    sc = miller_scalars()
    assert len(sc) == NPOOL and sc[:9] == [(a, b) for a in EDGE_VALUES for b in EDGE_VALUES]
    assert {v for i in (0, 5, 7, 8) for v in sc[i]} == set(EDGE_VALUES)
    assert sc[I_ID_P][0] is None and sc[I_ID_Q][1] is None and sc[I_ID_BOTH] == (None, None) and sc[I_OFF][0] == "off"
    assert sc[I_PAIR] == sc[I_REPEAT] and sc[I_NEG] == (R - sc[I_PAIR][0], sc[I_PAIR][1])
    for n, l in MILLER_SHAPES:
        assert SHAPE_OFFSET.get((n, l), 0) + n <= NPOOL


def test_tree_and_column_shapes_cover_what_they_claim():
    assert {pm.wave_fill(-(-n // 2), l)[1] < l for n in TREE_N for l in TREE_LPW if n > 1} == {True, False}
    assert any(n % 2 for n in TREE_N) and any(n % 2 == 0 for n in TREE_N)
    shapes = column_shapes()
    assert len(shapes) == len(COL_ROWS) * len(COL_COLS) - 1 and (4097, 1000) not in {(r, c) for r, c, _ in shapes}
    assert {r for r, _, _ in shapes} == set(COL_ROWS) and {c for _, c, _ in shapes} == set(COL_COLS)
    assert all(set(per) == {64, 100, r} for r, _, per in shapes)
    assert any(r > p and r % p for r, _, per in shapes for p in per), "no ragged last chunk"
    assert any(r == p for r, _, per in shapes for p in per) and any(r < p for r, _, per in shapes for p in per)
    assert any(c > 256 for _, c, _ in shapes) and any(c == 256 for _, c, _ in shapes)
    w, m = column_matrix(200, 5)
    assert (w[:128] == R - 1).all() and (m[:, 0] == R - 1).all() and {0, 1, R - 1} <= set(m[:, 1:].ravel())


def test_host_compiled_miller_is_the_oracles_pairing(exe, pr, off_subgroup):
    """NORMALISATION_POWER, from the host-compiled pairing_dev::miller alone (no HIP call is made): an ordinary pair, an
    edge pair, the point outside the subgroup and an identity."""
    from oracle import pairing as pg

    pick = [5, I_PAIR, I_OFF, I_ID_Q]
    pts = miller_points(pr.G1, pr.G2, off_subgroup[0], only=pick)
    out = run(exe, "host:miller", len(pick), [[1]] + [pair_words(*pts[i]) for i in pick]).reshape(len(pick), W12)
    for row, i in zip(out, pick):
        assert miller_to_gt(row) == pg.pair(*pts[i]), f"pool pair {i}"
    assert (out[3] == F12_ONE_LIMBS).all()
    assert miller_to_gt(out[0]) != [1] + [0] * 11


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the tower at the lazy-limb edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", list(OPS))
def test_tower_operation_on_device(exe, op, capsys):
    shape, classes, nout, max_class = OPS[op]
    x = np.concatenate(tower_cases(op))
    n = len(x)
    out = run(exe, op, n, [x]).reshape(2, n, nout * W1)
    dev, host = out[0], out[1]
    # 2. limbs: the device equals the same function compiled for the host, bit for bit
    assert_rows(dev, host, f"{op}: device limbs vs host-compiled limbs")
    # 1. residues: every coefficient is the Python reference
    ops_res = [pm.fp_residues(o) for o in split_operands(op, x)]
    got = pm.fp_residues(dev)
    for i in range(n):
        operands = [r[i][0] if k == 1 else pm.f2s(r[i]) for r, k in zip(ops_res, shape)]
        want = [c for f2 in reference(op, operands) for c in f2]
        assert got[i] == want, f"{op}: case {i} of {n}: coefficient {[j for j in range(len(want)) if got[i][j] != want[j]]} wrong"
    # 3. the range the headers state
    cls = int(pm.coeff_class(dev).max())
    assert cls <= max_class, f"{op}: output limb class {cls}"
    if op == "f12_mul_mem":
        big = max(abs(v) for row in pm.fp_values(dev) for v in row)
        assert big < 4 * P, f"f12_mul_mem: |coefficient| reached {big / P:.3f} p"
    with capsys.disabled():
        print(f"\n{op}: {n} cases ({len(classes)} class tuples x {NPATTERNS} patterns, {sum(shape) * len(fp_edges())} edge, {NRAND} random), "
              f"device == host limbs, output limb class <= {cls}")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: Miller loops pair by pair
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def miller_pool(co, off_subgroup):
    return miller_points(co.G1, co.G2, off_subgroup[0])


@pytest.fixture(scope="module")
def miller_runs(exe, miller_pool):
    """One run of k_miller_batch per shape, the first time a test asks for it: {shape index: (device rows incl. padding, host rows)}"""
    cache = {}

    def get(s):
        if s not in cache:
            n, lpw = MILLER_SHAPES[s]
            off = SHAPE_OFFSET.get((n, lpw), 0)
            try:
                out = run(exe, "miller", n, [[lpw]] + [pair_words(*miller_pool[off + i]) for i in range(n)])
            except BaseException as e:  # a failed run is reported by every test that needs it, and not started again
                cache[s] = e
                raise
            cache[s] = (out[:(n + PAD) * W12].reshape(n + PAD, W12), out[(n + PAD) * W12:].reshape(n, W12))
        if isinstance(cache[s], BaseException):
            raise cache[s]
        return cache[s]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("s", range(len(MILLER_SHAPES)), ids=[f"n{n}-lpw{l}" for n, l in MILLER_SHAPES])
def test_miller_batch_pair_by_pair(miller_runs, s, capsys):
    n, lpw = MILLER_SHAPES[s]
    off = SHAPE_OFFSET.get((n, lpw), 0)
    dev, host = miller_runs(s)
    unwritten = [i for i in range(n) if (dev[i] == POISON).all()]
    assert not unwritten, f"n = {n}, lpw = {lpw}: no lane wrote elements {unwritten}"
    assert_rows(dev[:n], host, f"k_miller_batch n = {n}, lpw = {lpw} vs host-compiled miller(), pair by pair")
    assert (dev[n:] == POISON).all(), f"n = {n}, lpw = {lpw}: an element at or past out[n] was written"
    sc = miller_scalars()
    for i in range(n):
        if sc[off + i][0] is None or sc[off + i][1] is None:
            assert (dev[i] == F12_ONE_LIMBS).all(), f"pair {i} holds an identity and is not f12_one()"
        else:
            assert not (dev[i] == F12_ONE_LIMBS).all()
    cls = int(pm.coeff_class(dev[:n]).max())
    assert cls <= 2, f"miller output at limb class {cls}"
    with capsys.disabled():
        print(f"\nk_miller_batch n = {n}, lpw = {lpw}: {n} pairs == host-compiled limbs, output limb class <= {cls}")


@pytest.mark.gpu
def test_sixteen_miller_values_are_the_oracles_pairings(miller_runs, pr, off_subgroup):
    """The device value mapped into the oracle's Fp12 and raised to (p^12 - 1) / r is oracle.pairing.pair(P, Q): about two
    seconds a pair in pure Python, so 16 pairs -- the edges and one of every shape."""
    from oracle import pairing as pg

    pts = miller_points(pr.G1, pr.G2, off_subgroup[0], only={SHAPE_OFFSET.get(MILLER_SHAPES[s], 0) + i for s, i in ORACLE_SUBSET})
    gts = {}
    for s, i in ORACLE_SUBSET:
        k = SHAPE_OFFSET.get(MILLER_SHAPES[s], 0) + i
        dev, _ = miller_runs(s)
        want = pg.pair(*pts[k])
        assert miller_to_gt(dev[i]) == want, f"shape {MILLER_SHAPES[s]}, element {i} (pool pair {k})"
        gts[k] = want
    one = [1] + [0] * 11
    assert gts[I_ID_P] == gts[I_ID_Q] == gts[I_ID_BOTH] == one and gts[I_PAIR] != one
    assert gts[I_REPEAT] == gts[I_PAIR] and pg.f12_mul(gts[I_NEG], gts[I_PAIR]) == one  # e(-P, Q) e(P, Q) = 1


def test_pool_points_agree_between_the_oracles(co, pr, off_subgroup):
    """The GPU test generates its points with the C oracle and pairs them with the Python one"""
    for a, b in miller_scalars()[:20]:
        if a not in (None, "off"):
            assert co.G1.mul(a) == pr.G1.mul(a)
        if b is not None:
            assert co.G2.mul(b) == pr.G2.mul(b)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the product tree, level by level
# ---------------------------------------------------------------------------------------------------------------------------
def _check_tree(exe, fac, what):
    n = len(fac)
    out = run(exe, "tree", n, [[len(TREE_LPW)] + TREE_LPW, fac])
    sizes = []
    m = n
    while m > 1:
        m = (m + 1) // 2
        sizes.append(m)
    at = 0
    dev = {}
    for lpw in TREE_LPW:
        for lv, h in enumerate(sizes):
            dev[lpw, lv] = out[at:at + (h + PAD) * W12].reshape(h + PAD, W12)
            at += (h + PAD) * W12
    host = []
    for h in sizes:
        host.append(out[at:at + h * W12].reshape(h, W12))
        at += h * W12
    assert at == len(out)
    res = pm.fp_residues(fac)
    want = pm.F12_ONE
    for r in res:
        want = pm.f12_mul(want, pm.f12_from_struct(pm.f2s(r)))
    worst = 0
    for lpw in TREE_LPW:
        prev, m = fac, n
        for lv, h in enumerate(sizes):
            d = dev[lpw, lv]
            assert_rows(d[:h], host[lv], f"{what}: n = {n}, lpw = {lpw}, level {lv} ({m} -> {h}) vs host f12_tree_node")
            assert (d[h:] == POISON).all(), f"{what}: n = {n}, lpw = {lpw}, level {lv}: an element past ceil({m} / 2) was written"
            if m % 2:
                assert (d[h - 1] == prev[m - 1]).all(), f"{what}: n = {n}, lpw = {lpw}, level {lv}: the odd one out was changed"
            products = d[:m // 2]
            if len(products):
                worst = max(worst, int(pm.coeff_class(products).max()))
                assert max(abs(v) for row in pm.fp_values(products) for v in row) < 4 * P
            prev, m = d[:h], h
        root = prev[0]
        got = pm.f12_from_struct(pm.f2s(pm.fp_residues(root.reshape(1, W12))[0]))
        assert got == want, f"{what}: n = {n}, lpw = {lpw}: the root is not the product of the factors (coefficients {[k for k in range(6) if got[k] != want[k]]} of w^k)"
    assert worst <= 2
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n", TREE_N)
def test_product_tree_of_worst_case_factors(exe, n):
    rng = _rng("treeworst")
    fac = np.array([pm.worst_coeffs(12, 2, i, rng) for i in range(n)], dtype=np.int64)
    _check_tree(exe, fac, "class-2 worst-case factors")


@pytest.mark.gpu
@pytest.mark.parametrize("n", TREE_N)
def test_product_tree_of_miller_values(exe, miller_runs, n):
    dev, host = miller_runs(len(MILLER_SHAPES) - 1)  # the 257 pairs of the pool
    assert (dev[:NPOOL] == host).all(), "the Miller values differ from the host's: see test_miller_batch_pair_by_pair"
    fac = np.concatenate([host] * 4)[:n]
    _check_tree(exe, fac, "Miller values")


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: weighted column sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows", COL_ROWS)
def test_weighted_column_sums(exe, rows):
    for r, cols, pers in column_shapes():
        if r != rows:
            continue
        w, m = column_matrix(rows, cols)
        out = run(exe, "columns", rows, [[cols, len(pers)] + pers, words8(w), words8(m)])
        at = 0
        for weighted in (True, False):
            prod = (w[:, None] * m) % R if weighted else m
            full = prod.sum(axis=0) % R
            for per in pers:
                what = f"rows = {rows}, cols = {cols}, rows per chunk = {per}, {'weights' if weighted else 'w = nullptr'}"
                chunks = -(-rows // per)
                n1, n2 = (chunks + 1) * cols * 8, 2 * cols * 8
                d1, d2 = out[at:at + n1].reshape(chunks + 1, cols * 8), out[at + n1:at + n1 + n2].reshape(2, cols * 8)
                at += n1 + n2
                h1, h2 = out[at:at + chunks * cols * 8].reshape(chunks, cols * 8), out[at + chunks * cols * 8:at + (chunks + 1) * cols * 8]
                at += (chunks + 1) * cols * 8
                assert (d1[chunks] == POISON).all() and (d2[1] == POISON).all(), f"{what}: a row past the last chunk was written"
                got1 = from_words8(d1[:chunks]).reshape(chunks, cols)
                got2 = from_words8(d2[0])
                assert (got1 < R).all() and (got2 < R).all(), f"{what}: an output is not canonical"
                want1 = np.array([prod[c * per:min(rows, (c + 1) * per)].sum(axis=0) % R for c in range(chunks)], dtype=object)
                bad = np.argwhere(got1 != want1)
                assert not len(bad), f"{what}: chunk {bad[0][0]} column {bad[0][1]} is not sum w_i m_ij mod r ({len(bad)} wrong)"
                bad = np.nonzero(got2 != full)[0]
                assert not len(bad), f"{what}: second pass, column {bad[0]} is not the full column sum"
                assert_rows(d1[:chunks], h1, f"{what}: device vs host-compiled fr_weighted_column")
                assert (d2[0] == h2).all(), f"{what}: second pass, device vs host"
        assert at == len(out)
