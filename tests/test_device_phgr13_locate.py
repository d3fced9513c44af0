"""The two kernels of the locating PHGR13 batch verifier (playsnark_amd/csrc/locate_phgr13_dev.hpp) VALUE BY VALUE.

tests/test_phgr13_verify_locate_gpu.py compares verdicts and masks; here tests/device_phgr13_locate_check.hip launches the
shipped k_g2_pair_sums and k_f12_segment_products directly, every output into a poisoned, padded buffer of its own.
  * CPU: the program cross-compiles, and its two kernels have the library's register allocation and spill nothing.
  * GPU, k_g2_pair_sums: every node of every level against the oracle's G2 addition; node counts 1, 2, 3, 5, 64, 65 (a carried
    node at two levels for 5, at six for 65); neighbouring pairs of the six kinds of test_device_locate.point_nodes (unrelated,
    P P, P -P, O Q, Q O, O O); the segmented form with 1 and 3 segments of 1, 2 and 21 points.
  * GPU, k_f12_segment_products: against pairing_model.f12_mul, values compared as tests/test_device_pairing.py compares them;
    1, 3 and 65 segments of 1, 2, 3, 7 and 64 factors, with and without `first`, operands canonical and at the worst limb
    class pairing_dev::f12_coeff documents for stored values (class 2); the stored results stay below 4 p at class <= 2.
The device program runs as a subprocess with a time limit; a failed run is reported once and never retried.
Nothing here needs a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_model as fm  # noqa: E402
import pairing_model as pm  # noqa: E402
from test_device_field import FLAGS, HIPCC  # noqa: E402
from test_device_locate import KINDS, level_sizes, run, words_of  # noqa: E402
from test_device_pairing import _kernel_notes, _one  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "device_phgr13_locate_check.hip")
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
P, R = fm.P, fm.R
W12 = pm.W12
PAD = 8
POISON = 0xA5A5A5A5
NODES = [1, 2, 3, 5, 64, 65]
SEGMENTS = [(k, n) for k in (1, 3) for n in (1, 2, 21)]
PRODUCT_SEGS = {1: 1, 3: 2, 65: 64}  # segments: active lanes per wave (one lane; two waves, the second half full; a full wave and one lane)
PRODUCT_LENS = [1, 2, 3, 7, 64]
STORED_CLASS = 2  # pairing_dev.hpp, f12_coeff: stored coefficients are below 4 p in absolute value at limb class <= 2


def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("device_phgr13_locate") / "device_phgr13_locate_check")
    res = subprocess.run([HIPCC, *FLAGS, SRC, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert res.returncode == 0, f"build failed:\n{res.stdout[-4000:]}"
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------------
def g2_nodes(co, n, tag):
    """n G2 points (None: the identity); neighbouring pair p = (2p, 2p + 1) is of kind (p + n) % 6, as
    test_device_locate.point_nodes lays them out: two unrelated points, P P, P -P, O Q, Q O, O O"""
    rng = _rng(f"g2points{tag}")
    draw = lambda: co.G2.mul(int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1)
    pts = []
    for p in range((n + 1) // 2):
        kind = (p + n) % KINDS
        a = draw()
        pair = [(a, draw()), (a, a), (a, co.G2.mul(R - 1, a)), (None, a), (a, None), (None, None)][kind]
        pts += list(pair)
    return pts[:n]


def g2_reference(co, pts):
    out, cur = [], pts
    for h in level_sizes(len(pts)):
        nxt = [co.G2.add(cur[2 * i], cur[2 * i + 1]) if 2 * i + 1 < len(cur) else cur[2 * i] for i in range(h)]
        out.append(nxt)
        cur = nxt
    return out


def g2_words(p):
    return [0] * 48 if p is None else words_of(p[0][0], 12) + words_of(p[0][1], 12) + words_of(p[1][0], 12) + words_of(p[1][1], 12)


def check_g2(exe, co, segs, n, tag):
    """Run `segs` segments of n points and compare every node of every level; returns the identities met above the leaves"""
    segments = [g2_nodes(co, n, f"{tag}s{s}") for s in range(segs)]
    out = run(exe, "g2points", n, [segs] + [w for seg in segments for p in seg for w in g2_words(p)])
    refs = [g2_reference(co, seg) for seg in segments]
    at, identities = 0, 0
    for lv, h in enumerate(level_sizes(n)):
        for s in range(segs):
            for i in range(h):
                got = out[at:at + 48]
                at += 48
                want = refs[s][lv][i]
                assert [int(w) for w in got] == g2_words(want), f"segs = {segs}, n = {n}: segment {s}, level {lv + 1}, node {i} is not the sum of its children"
                identities += want is None
        assert int(out[at]) == 0, f"segs = {segs}, n = {n}, level {lv + 1}: {int(out[at])} slots no node owns were written"
        at += 1
    assert at == len(out)
    return identities


def f12_of(rows):
    """(n, 168) limbs -> n elements as coefficient lists of 1, w, .., w^5"""
    return [pm.f12_from_struct(pm.f2s(r)) for r in pm.fp_residues(rows)]


def factors(kind, n, tag):
    """(n, 168) raw limbs: canonical Montgomery-form coefficients, or every limb at the edge of the stored class"""
    rng = _rng(f"segprod{kind}{tag}")
    if kind == "canonical":
        return pm.canon_coeffs(12, n, rng).reshape(n, W12) if n else np.zeros((0, W12), dtype=np.int64)
    return np.array([pm.worst_coeffs(12, STORED_CLASS, i, rng) for i in range(n)], dtype=np.int64).reshape(n, W12)


def check_products(exe, segs, length, with_first, kind):
    lpw = PRODUCT_SEGS[segs]
    first = factors(kind, segs, f"first{segs}x{length}") if with_first else np.zeros((0, W12), dtype=np.int64)
    fac = factors(kind, segs * length, f"{segs}x{length}{with_first}")
    words = np.concatenate([np.array([length, int(with_first), lpw], dtype=np.int64), first.ravel() & 0xFFFFFFFF, fac.ravel() & 0xFFFFFFFF])
    out = run(exe, "segprod", segs, words)
    got = out.astype(np.int64).reshape(segs + PAD, W12)
    what = f"segs = {segs}, len = {length}, first = {with_first}, {kind} operands"
    assert (got[segs:] == POISON).all(), f"{what}: an element past the last segment was written"
    dev = np.where(got[:segs] >= (1 << 31), got[:segs] - (1 << 32), got[:segs])  # limbs are signed words
    fv, xv = f12_of(first) if with_first else None, f12_of(fac)
    values = f12_of(dev)
    for s in range(segs):
        want = fv[s] if with_first else pm.F12_ONE
        for j in range(length):
            want = pm.f12_mul(want, xv[s * length + j])
        assert values[s] == want, f"{what}: segment {s} is not first * the product of its factors (coefficients {[k for k in range(6) if values[s][k] != want[k]]} of w^k)"
    if with_first or length > 1:  # products: what f12_mul_mem stores
        assert int(pm.coeff_class(dev).max()) <= STORED_CLASS, f"{what}: a stored limb left class {STORED_CLASS}"
        assert max(abs(v) for row in pm.fp_values(dev) for v in row) < 4 * P, f"{what}: a stored coefficient reached 4 p"
    else:  # one factor and no first: the factor itself, limb for limb
        assert (dev == fac).all(), f"{what}: a lone factor was changed"


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_program_compiles_and_lists_its_operations(exe):
    out = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert out == ["g2points", "segprod"]


def test_the_test_build_runs_the_shipped_kernels(exe, tmp_path):
    """Otherwise the GPU tests could pass on code nobody ships: the two kernels have the library's register allocation;
    neither spills, the point kernel fits two waves per SIMD (at most 256 registers) and the product kernel one (at most 512)."""
    assert os.path.exists(LIB), "the library has not been built"
    mine, lib = _kernel_notes(exe, str(tmp_path / "t")), _kernel_notes(LIB, str(tmp_path / "l"))
    for name in ("k_g2_pair_sums", "k_f12_segment_products"):
        a, b = _one(mine, name), _one(lib, name)
        assert a["name"] == b["name"]
        assert (int(a["vgpr_count"]), int(a["agpr_count"])) == (int(b["vgpr_count"]), int(b["agpr_count"])), (a, b)
        assert int(a["vgpr_spill_count"]) == int(b["vgpr_spill_count"]) == 0, (name, a, b)
    assert int(_one(lib, "k_g2_pair_sums")["vgpr_count"]) <= 256
    assert int(_one(lib, "k_f12_segment_products")["vgpr_count"]) <= 512
    # the G1 kernel keeps its name: tests/device_locate_check.hip launches it
    assert int(_one(lib, "k_g1_pair_sums")["vgpr_spill_count"]) == 0


def test_operand_sets_hold_the_edges_they_claim(co):
    pts = g2_nodes(co, 64, "probe")
    assert {(p + 64) % KINDS for p in range(32)} == set(range(KINDS))
    pairs = list(zip(pts[0::2], pts[1::2]))
    assert any(a is not None and a == b for a, b in pairs) and any(a is None and b is None for a, b in pairs)
    assert any(a is None and b is not None for a, b in pairs) and any(a is not None and b is None for a, b in pairs)
    assert any(a is not None and b is not None and a != b and co.G2.add(a, b) is None for a, b in pairs)
    assert all(p is None or co.G2.on_curve(p) for p in pts)
    worst = factors("worst", 5, "probe")
    assert int(pm.coeff_class(worst).max()) == STORED_CLASS and int(pm.coeff_class(factors("canonical", 5, "probe")).max()) == 1
    assert [(s + l - 1) // l for s, l in PRODUCT_SEGS.items()] == [1, 2, 2]  # waves of each launch


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", NODES)
def test_g2_tree_level_by_level(exe, co, n):
    identities = check_g2(exe, co, 1, n, f"tree{n}")
    if n >= 64:
        assert identities > 0  # P + (-P) and O + O above the leaves


@pytest.mark.gpu
@pytest.mark.parametrize("segs,n", SEGMENTS)
def test_segmented_g2_sums(exe, co, segs, n):
    check_g2(exe, co, segs, n, f"seg{segs}x{n}")


@pytest.mark.gpu
@pytest.mark.parametrize("segs", list(PRODUCT_SEGS))
@pytest.mark.parametrize("length", PRODUCT_LENS)
def test_segment_products(exe, segs, length):
    for with_first in (False, True):
        for kind in ("canonical", "worst"):
            check_products(exe, segs, length, with_first, kind)
