"""The tree kernels of the locating batch verifier (playsnark_amd/csrc/locate_dev.hpp) NODE BY NODE.

tests/test_verify_locate_gpu.py compares verdicts; here tests/device_locate_check.hip launches the shipped k_g1_pair_sums
and k_fr_row_pair_sums directly, level by level as verify_locate.inc does, every level into a poisoned buffer of its own,
and every node of every level is compared: scalars with Python integers mod r, points with the oracle's Add.
  * CPU: the program cross-compiles, and its two kernels have the library's register allocation and spill nothing; the
    operand sets hold the edges they claim.
  * GPU: node counts 1, 2, 3, 5, 64, 65, 127, 130 (a carried node at two levels for 5, at six for 65, at the leaves for 127); rows of 1, 2, 22 and
    257 scalars with 0, r - 1 and pairs that sum to exactly r; points with identity operands, equal neighbours (the
    doubling), P next to -P; the segmented form with 1 and 3 segments of 1, 2 and 21 points.
The device program runs as a subprocess with a time limit; a failed run is reported once and never retried.
Nothing here needs a tolerance."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_model as fm  # noqa: E402
from test_device_field import FLAGS, HIPCC  # noqa: E402
from test_device_pairing import _kernel_notes, _one  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "device_locate_check.hip")
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
R = fm.R
PAD = 8
POISON = 0xA5A5A5A5
NODES = [1, 2, 3, 5, 64, 65, 127, 130]
WIDTHS = [1, 2, 22, 257]
SEGMENTS = [(k, n) for k in (1, 3) for n in (1, 2, 21)]
KINDS = 6  # of neighbouring pairs of points, see point_nodes


def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("device_locate") / "device_locate_check")
    res = subprocess.run([HIPCC, *FLAGS, SRC, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert res.returncode == 0, f"build failed:\n{res.stdout[-4000:]}"
    return out


def run(exe, op, n, words, timeout=300):
    """One run of the program: reported, never retried.  Returns the output words as Python-int-safe uint64."""
    x = np.asarray(words, dtype=np.uint64)
    assert x.max(initial=0) < (1 << 32)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        x.astype(np.uint32).tofile(fin)
        res = subprocess.run([exe, op, str(n), fin, fout], capture_output=True, text=True, timeout=timeout)
        assert res.returncode == 0, f"{op}: exit status {res.returncode}\n{res.stdout[-1000:]}{res.stderr[-2000:]}"
        return np.fromfile(fout, dtype=np.uint32).astype(np.uint64)


def level_sizes(n):
    """Node counts of the levels above the leaves; n = 1 runs one level 1 -> 1 (the carried copy alone)"""
    out = []
    while True:
        n = (n + 1) // 2
        out.append(n)
        if n <= 1:
            return out


# ---------------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------------
def scalar_rows(n, cols):
    """n rows of cols scalars below r: values from {0, 1, r - 1} and random ones; in every third column the odd row of a
    pair is r minus the even row (the pair sums to exactly r), in column 1 (if there is one) every value is r - 1."""
    rng = _rng(f"rows{n}x{cols}")
    kind = rng.integers(0, 6, size=(n, cols))
    rows = [[0 if k == 0 else 1 if k == 1 else R - 1 if k == 2 else int.from_bytes(rng.bytes(40), "little") % R for k in kr] for kr in kind]
    for i in range(1, n, 2):
        for j in range(0, cols, 3):
            rows[i][j] = (R - rows[i - 1][j]) % R if rows[i - 1][j] else 0
    if cols > 1:
        for i in range(n):
            rows[i][1] = R - 1
    return rows


def rows_reference(rows):
    """Every level above the leaves, as lists of rows of Python ints"""
    out, cur = [], rows
    for h in level_sizes(len(rows)):
        nxt = [[(a + b) % R for a, b in zip(cur[2 * i], cur[2 * i + 1])] if 2 * i + 1 < len(cur) else list(cur[2 * i]) for i in range(h)]
        out.append(nxt)
        cur = nxt
    return out


def words_of(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def int_of(words):
    return sum(int(w) << (32 * i) for i, w in enumerate(words))


def point_nodes(co, n, tag):
    """n points (None: the identity).  Neighbouring pair p = (2p, 2p + 1) is of kind (p + n) % 6: two unrelated points,
    P P (the doubling), P -P, O Q, Q O, O O -- so that the small trees meet the edges too.  The sums of the pairs P -P and
    O O put identities, and the pairs P P doubled points, into the levels above."""
    rng = _rng(f"points{tag}")
    draw = lambda: co.G1.mul(int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1)
    pts = []
    for p in range((n + 1) // 2):
        kind = (p + n) % KINDS
        a = draw()
        pair = [(a, draw()), (a, a), (a, co.G1.mul(R - 1, a)), (None, a), (a, None), (None, None)][kind]
        pts += list(pair)
    return pts[:n]


def points_reference(co, pts):
    out, cur = [], pts
    for h in level_sizes(len(pts)):
        nxt = [co.G1.add(cur[2 * i], cur[2 * i + 1]) if 2 * i + 1 < len(cur) else cur[2 * i] for i in range(h)]
        out.append(nxt)
        cur = nxt
    return out


def point_words(p):
    return [0] * 24 if p is None else words_of(p[0], 12) + words_of(p[1], 12)


def check_points(exe, co, segs, n, tag):
    """Run `segs` segments of n points and compare every node of every level; returns (identities, doublings met)"""
    segments = [point_nodes(co, n, f"{tag}s{s}") for s in range(segs)]
    out = run(exe, "points", n, [segs] + [w for seg in segments for p in seg for w in point_words(p)])
    refs = [points_reference(co, seg) for seg in segments]
    at, identities = 0, 0
    for lv, h in enumerate(level_sizes(n)):
        for s in range(segs):
            for i in range(h):
                got = out[at:at + 24]
                at += 24
                want = refs[s][lv][i]
                assert [int(w) for w in got] == point_words(want), f"segs = {segs}, n = {n}: segment {s}, level {lv + 1}, node {i} is not the sum of its children"
                identities += want is None
        assert int(out[at]) == 0, f"segs = {segs}, n = {n}, level {lv + 1}: {int(out[at])} slots no node owns were written"
        at += 1
    assert at == len(out)
    return identities


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_program_compiles_and_lists_its_operations(exe):
    out = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out == ["rows", "points"]


def test_the_test_build_runs_the_shipped_kernels(exe, tmp_path):
    """Otherwise the GPU tests could pass on code nobody ships: the two kernels have the library's register allocation;
    neither spills, and the point kernel fits two waves per SIMD (at most 256 registers)."""
    assert os.path.exists(LIB), "the library has not been built"
    mine, lib = _kernel_notes(exe, str(tmp_path / "t")), _kernel_notes(LIB, str(tmp_path / "l"))
    for name in ("k_g1_pair_sums", "k_fr_row_pair_sums"):
        a, b = _one(mine, name), _one(lib, name)
        assert a["name"] == b["name"]
        assert (int(a["vgpr_count"]), int(a["agpr_count"])) == (int(b["vgpr_count"]), int(b["agpr_count"])), (a, b)
        assert int(a["vgpr_spill_count"]) == int(b["vgpr_spill_count"]) == 0, (name, a, b)
    g1 = _one(lib, "k_g1_pair_sums")
    assert int(g1["vgpr_count"]) + int(g1["agpr_count"]) <= 256, g1
    for name in ("k_fr_locate_rows", "k_gather_words"):
        assert int(_one(lib, name)["vgpr_spill_count"]) == 0


def test_operand_sets_hold_the_edges_they_claim(co):
    assert [level_sizes(n) for n in (1, 2, 5)] == [[1], [1], [3, 2, 1]]
    # the levels at which the odd one out is carried up: several for 5 and 65, the leaves alone for 127
    for n, carried in ((5, [0, 1]), (65, [0, 1, 2, 3, 4, 5]), (127, [0])):
        sizes = [n] + level_sizes(n)
        assert [l for l, m in enumerate(sizes[:-1]) if m % 2 and m > 1] == carried
    rows = scalar_rows(64, 22)
    flat = [v for r in rows for v in r]
    assert 0 in flat and R - 1 in flat and all(0 <= v < R for v in flat)
    exact = [(i, j) for i in range(1, 64, 2) for j in range(0, 22, 3) if rows[i][j] and rows[i][j] + rows[i - 1][j] == R]
    assert len(exact) >= 64, "too few pairs that sum to exactly r"
    assert all(rows[i][1] == R - 1 for i in range(64))  # (r - 1) + (r - 1): the largest sum
    pts = point_nodes(co, 64, "probe")
    kinds = {(p + 64) % KINDS for p in range(32)}
    assert kinds == set(range(KINDS))
    pairs = list(zip(pts[0::2], pts[1::2]))
    assert any(a is not None and a == b for a, b in pairs) and any(a is None and b is None for a, b in pairs)
    assert any(a is None and b is not None for a, b in pairs) and any(a is not None and b is None for a, b in pairs)
    assert any(a is not None and b is not None and a != b and co.G1.add(a, b) is None for a, b in pairs)
    assert {(p + n) % KINDS for n in (2, 3, 5) for p in range(n // 2)} >= {0, 2, 3, 5}


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", NODES)
def test_scalar_tree_level_by_level(exe, n):
    for cols in WIDTHS:
        rows = scalar_rows(n, cols)
        out = run(exe, "rows", n, [cols] + [w for r in rows for v in r for w in words_of(v, 8)])
        at = 0
        for lv, (h, want) in enumerate(zip(level_sizes(n), rows_reference(rows))):
            got = out[at:at + (h + PAD) * cols * 8].reshape(h + PAD, cols, 8)
            at += (h + PAD) * cols * 8
            assert (got[h:] == POISON).all(), f"n = {n}, cols = {cols}, level {lv + 1}: a row past the last node was written"
            for i in range(h):
                vals = [int_of(got[i, j]) for j in range(cols)]
                assert all(v < R for v in vals), f"n = {n}, cols = {cols}, level {lv + 1}, node {i}: not canonical"
                bad = [j for j in range(cols) if vals[j] != want[i][j]]
                assert not bad, f"n = {n}, cols = {cols}, level {lv + 1}, node {i}: columns {bad[:8]} are not the sum mod r of the children"
        assert at == len(out)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NODES)
def test_point_tree_level_by_level(exe, co, n):
    identities = check_points(exe, co, 1, n, f"tree{n}")
    if n >= 64:
        assert identities > 0  # P + (-P) and O + O above the leaves


@pytest.mark.gpu
@pytest.mark.parametrize("segs,n", SEGMENTS)
def test_segmented_point_sums(exe, co, segs, n):
    check_points(exe, co, segs, n, f"seg{segs}x{n}")
