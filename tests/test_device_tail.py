"""The tail of a sum (playsnark_amd/csrc/qtail.hpp) VALUE BY VALUE on the device: the lane-quad group law q_add, the tree
q_block_tree, the reduction kernels k_qreduce_rowcol / k_qreduce_bits and the fix-up kernels k_qfixup, k_qfixup_chain,
k_heavy_jobs, k_qfixup_heavy_part, k_qfixup_heavy, for Fp (G1, four lanes a point) and Fp2s (G2, eight lanes).

The library-level tests compare a tail kernel's output with the oracle only as the final point of a whole sum over distinct
random points, where no two partial sums are ever equal or opposite: the doubling and cancellation branches of q_add, and a
wave whose quads take different branches at once, are reached by accident or not at all.  Here tests/device_tail_check.hip
launches the shipped kernels directly (only q_add and q_block_tree sit behind a wrapper: q_load, the call, q_store) and every
value is compared with Python integers (tests/curve_model.py: the oracle's affine law for on-curve operands, add-2008-s /
dbl-2008-s mod p for off-curve ones).  Collinear inputs m P with -3 <= m <= 3 make collisions the rule, and the expected value
of any sum one scalar multiplication.
  * CPU: the program cross-compiles with the product's flags; the two forms of the reference agree on on-curve operands in
    every branch; the operand sets and their placement in waves hold what they claim.
  * GPU: (a) q_add over every branch and at the lazy-limb edges, q_block_tree at every group size; (b) the reduction at the
    shapes on each side of every decision of msm_plan_tail, at every block size the host can pick; (c) the fix-up at every
    quads-per-bucket count, at the spans around the heavy threshold, with chain lists and heavy buckets of every size class.
The device program runs as a subprocess with a time limit; a failed run is reported once and never retried.
Nothing here needs a tolerance: every comparison is exact.

Limb classes q_add admits for STORED coordinates (its comment, qtail.hpp "Limb classes: ..", and field.hpp's contract).
A stored coordinate is "class ~1", which is one of two forms:
  P  a product: limbs 0..12 in [0, 2^28), a signed top limb.  As a limb class this is class 1 (|limb| < 2^28); the test takes
     the whole class, negative limbs included (fm.worst(1), fm.random_lazy(1)).
  N  f_norm of a sum of <= 4 fresh products, i.e. of a class-4 value: limb 0 in [0, 2^28), limbs 1..12 in [-3, 2^28 + 2].
     Built as fm.norm(fm.worst(4)) / fm.norm(fm.random_lazy(4)): the carry-save step at its extremes.
Every coordinate holds |V| <= 16 p (f_mul's and f_is_zero's range; the generators' top limb); in the doubling branch
|V| < 5 p, which covers every stored value (X3 below) and keeps 2 y inside f_sqr's range.  Every combination of P and N
over the eight coordinates of (A, B) is run, in the general branch and, with B = +-A, in the doubling and cancelling ones.
On top of that the general branch is run with every coordinate at the edge of limb class 2 proper (|limb| = 2^29 - 1,
fm.worst(2)): the comment's closing claim is "every product sees class(a) class(b) <= 4", which admits 2 x 2, and the Fp2s
products (two per lane under one reduction) need exactly that.  The doubling branch is NOT run there: xyzz_dbl squares 2 y,
which is inside f_sqr's contract for the forms P and N only.
Ranges asserted for computed results (general branch, from the comment's [qq, ZZ3, ppp, ppp] / x3 / g and field.hpp's product
range; two products under one reduction double the (-p/8) margin): ZZ3, ZZZ3 and Y3 (a product, or f_norm of one reduction)
in (-p/4, 5p/4); X3 = f_norm(rr - ppp - 2 qq) in (-4 p, 2 p), which with |qq| < 5p/4 keeps |x3 - qq| under the comment's 5.7 p.
Doubling branch (xyzz_dbl): the same, except Y3 = f_norm of a difference of two products, in (-3p/2, 3p/2)."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import curve_model as cm  # noqa: E402
import field_model as fm  # noqa: E402
from test_device_field import FLAGS, HIPCC  # noqa: E402

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_tail_check.hip")
P = fm.P
PAD = 4  # device_tail_check.hip: elements past the end of an output buffer
POISON = int(np.int32(-0x5A5A5A5B))  # 0xA5A5A5A5
QFIX_HEAVY = 16  # qtail.hpp
GROUPS = ["g1", "g2"]


def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


# ---------------------------------------------------------------------------------------------------------------------------
# build and run
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("device_tail") / "device_tail_check")
    res = subprocess.run([HIPCC, *FLAGS, SRC, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert res.returncode == 0, f"build failed:\n{res.stdout[-4000:]}"
    return out


def run(exe, op, n, parts, timeout=120):
    """One run of the program: reported, never retried.  Returns the flat int32 output as int64."""
    x = np.concatenate([np.asarray(p, dtype=np.int64).ravel() for p in parts])
    assert x.min() >= -(1 << 31) and x.max() < (1 << 31)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        x.astype(np.int32).tofile(fin)
        res = subprocess.run([exe, op, str(n), fin, fout], capture_output=True, text=True, timeout=timeout)
        assert res.returncode == 0, f"{op}: exit status {res.returncode}\n{res.stdout[-1000:]}{res.stderr[-2000:]}"
        return np.fromfile(fout, dtype=np.int32).astype(np.int64)


def take_points(cv, flat, at, count, what):
    """(count, PT) words from position `at` of an output, the PAD poisoned points behind them checked; -> rows, next position"""
    end = at + (count + PAD) * cv.PT
    assert end <= len(flat), f"{what}: output too short"
    rows = flat[at:at + count * cv.PT].reshape(count, cv.PT)
    assert (flat[at + count * cv.PT:end] == POISON).all(), f"{what}: a store past the end of the output"
    return rows, end


def take_words(flat, at, count, what, pad=PAD):
    end = at + count + pad
    assert end <= len(flat), f"{what}: output too short"
    assert (flat[at + count:end] == POISON).all(), f"{what}: a store past the end of the list"
    return flat[at:at + count], end


def is_poison(row):
    return bool((np.asarray(row) == POISON).all())


# ---------------------------------------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_point(g):
    """one subgroup point per group, the P of every collinear input"""
    return cm.CURVES[g].grp.mul(0x9E3779B97F4A7C15 if g == "g1" else 0xC2B2AE3D27D4EB4F)


@functools.lru_cache(maxsize=None)
def multiples(g):
    return cm.CURVES[g].multiples(base_point(g))


@functools.lru_cache(maxsize=None)
def random_points(g):
    """64 distinct subgroup points"""
    rng = _rng("pool" + g)
    cv = cm.CURVES[g]
    pts = [cv.grp.mul(int.from_bytes(rng.bytes(8), "little") | 1) for _ in range(64)]
    assert len(set(pts)) == 64
    return pts


@functools.lru_cache(maxsize=None)
def multiple_of_base(g, k):
    """k P (sums of collinear inputs take few different values: one scalar multiplication each)"""
    return cm.CURVES[g].times(k, base_point(g))


def identity_form(cv, rng, k):
    """the identity in several guises: all zeros; X and Y left over from an earlier value; ZZZ non-zero"""
    z = cv.zero
    return [(z, z, z, z), (cv.rand(rng), cv.rand(rng), z, z), (cv.rand(rng), z, z, cv.rand(rng))][k % 3]


def collinear_words(cv, g, ms, rng):
    """(len(ms), PT) words: m P for every m, each in a representation of its own; 0 is the identity"""
    mult = multiples(g)
    pts = [identity_form(cv, rng, i) if m == 0 else cv.rand_rep(mult[int(m)], rng) for i, m in enumerate(ms)]
    return cm.pack_points(cv, pts)


def decode_rows(cv, rows):
    return [cv.unpack([int(w) for w in row]) for row in rows]


def assert_multiple(cv, g, row, k, what):
    """the stored point is k P, consistently"""
    pt = cv.unpack([int(w) for w in row])
    want = multiple_of_base(g, int(k))
    got = cv.affine(pt)
    assert got == want, f"{what}: not {k} P"
    if got is not None:
        assert cv.consistent(pt), f"{what}: ZZ^3 != ZZZ^2"
    assert limb_classes(cv, row).max() <= 2, f"{what}: a stored coordinate at limb class {limb_classes(cv, row).max()}"


def limb_classes(cv, row):
    return fm.limb_class(np.asarray(row, dtype=np.int64).reshape(-1, fm.FP_L))


# ---------------------------------------------------------------------------------------------------------------------------
# (a) q_add: the cases and their placement
# ---------------------------------------------------------------------------------------------------------------------------
TOP_5P = 4 * fm.FP_MOD[fm.FP_L - 1]  # a top limb that keeps |V| under 5 p


def _form(form, pattern, rng, top=fm.TOP_SPAN):
    """14 limbs of one component in the form P / N (edge), C (class 2 proper, edge), p / n (random); top: the top limb's span
    (the default is the generators': |V| <= 16 p)"""
    if form == "P":
        return fm.worst(1, pattern, rng, top=top)
    if form == "N":
        return [int(v) for v in fm.norm(np.array([fm.worst(4, pattern, rng, top=top)], dtype=np.int64))[0]]
    if form == "C":
        return fm.worst(2, pattern, rng, top=top)
    if form == "p":
        return [int(v) for v in fm.random_lazy(1, 1, rng, top=top)[0]]
    assert form == "n"
    return [int(v) for v in fm.norm(fm.random_lazy(4, 1, rng, top=top))[0]]


def _lazy_point(cv, forms, pattern, rng, top=fm.TOP_SPAN):
    """a point's words, coordinate j in form forms[j] (both components of an Fp2 in the same form, other sign patterns)"""
    return sum((_form(forms[j], (pattern + j + k) & 3, rng, top) for j in range(4) for k in range(cv.comps)), [])


def _negate_y(cv, words):
    w = list(words)
    for i in range(cv.W, 2 * cv.W):
        w[i] = -w[i]
    return w


def _zero_forms(rng):
    """non-zero limbs whose value is 0 mod p, |V| < 3 p (f_is_zero's stated range, field.hpp)"""
    out = [e for e in fm.fp_zero_edges(rng) if fm.to_int(e) % P == 0 and abs(fm.to_int(e)) < 3 * P and any(e)]
    assert len(out) >= 12
    return out


class Case:
    def __init__(self, a, b, kind, geo=None):
        self.a, self.b, self.kind, self.geo = [int(v) for v in a], [int(v) for v in b], kind, geo


@functools.lru_cache(maxsize=None)
def qadd_families(g):
    """the operand families, by the branch each must take"""
    cv = cm.CURVES[g]
    rng = _rng("qadd" + g)
    pool = random_points(g)
    fam = {k: [] for k in cm.BRANCHES}

    def pick():
        return pool[int(rng.integers(len(pool)))]

    def rep(pt):
        return cv.pack(cv.rand_rep(pt, rng))

    # general: random subgroup points, every operand in a representation of its own
    for _ in range(96):
        pa, pb = pick(), pick()
        if pa[0] == pb[0]:
            continue
        fam[cm.GENERAL].append(Case(rep(pa), rep(pb), cm.GENERAL, (pa, pb)))
    # the branches, each in several representations
    zf = _zero_forms(rng)
    for i in range(9):
        pa = pick()
        ident = cv.pack(identity_form(cv, rng, i))
        fam[cm.A_IDENTITY].append(Case(ident, rep(pa), cm.A_IDENTITY, (None, pa)))
        fam[cm.B_IDENTITY].append(Case(rep(pa), ident, cm.B_IDENTITY, (pa, None)))
        fam[cm.B_IDENTITY].append(Case(ident, cv.pack(identity_form(cv, rng, i + 1)), cm.B_IDENTITY, (None, None)))  # both
        a = rep(pa)
        fam[cm.DOUBLE].append(Case(a, rep(pa), cm.DOUBLE, (pa, pa)))  # u1 = u2 mod p in other limbs
        fam[cm.DOUBLE].append(Case(a, a, cm.DOUBLE, (pa, pa)))        # limb for limb
        fam[cm.CANCEL].append(Case(a, rep(cv.grp.neg(pa)), cm.CANCEL, (pa, cv.grp.neg(pa))))
        fam[cm.CANCEL].append(Case(a, _negate_y(cv, a), cm.CANCEL, (pa, cv.grp.neg(pa))))
    # the identity with a non-zero ZZ = 0 mod p (ZZZ likewise, or zero)
    for i in range(0, len(zf) - 1, 2):
        pa = pick()
        ident = cv.pack(identity_form(cv, rng, 1))
        for k in range(cv.comps):
            ident[2 * cv.W + fm.FP_L * k:2 * cv.W + fm.FP_L * (k + 1)] = zf[(i + k) % len(zf)]
            if i % 4 == 0:
                ident[3 * cv.W + fm.FP_L * k:3 * cv.W + fm.FP_L * (k + 1)] = zf[(i + k + 1) % len(zf)]
        fam[cm.A_IDENTITY].append(Case(ident, rep(pa), cm.A_IDENTITY, (None, pa)))
        fam[cm.B_IDENTITY].append(Case(rep(pa), ident, cm.B_IDENTITY, (pa, None)))
    # G2 near-collisions (formula level): the x difference p = u2 - u1, or the y difference, is zero in ONE component only.
    # B has ZZ = ZZZ = 1, so u1 = X1, s1 = Y1, u2 = X2 ZZ1, s2 = Y2 ZZZ1.
    if cv.f2:
        one = cv.one
        for dx, dy, kind in (((0, 5), None, cm.GENERAL), ((7, 0), None, cm.GENERAL), (None, (0, 3), cm.GENERAL), (None, (9, 0), cm.GENERAL),
                             ((0, 0), (0, 11), cm.CANCEL), ((0, 0), (13, 0), cm.CANCEL), ((0, 1), (0, 0), cm.GENERAL), ((1, 0), (0, 0), cm.GENERAL)):
            A = cv.rand_rep(pick(), rng)
            dx = cv.rand(rng) if dx is None else dx
            dy = cv.rand(rng) if dy is None else dy
            X2 = cv.mul(cv.add(A[0], dx), cv.inv(A[2]))
            Y2 = cv.mul(cv.add(A[1], dy), cv.inv(A[3]))
            fam[kind].append(Case(cv.pack(A), cv.pack((X2, Y2, one, one)), kind))
    # lazy-limb edges (formula level, off the curve): every combination of the forms P and N over the eight coordinates
    for idx in range(256):
        forms = ["N" if (idx >> j) & 1 else "P" for j in range(8)]
        # (B under another sign pattern than A: the edge limbs of one form differ in nothing else, and B = A is the doubling)
        fam[cm.GENERAL].append(Case(_lazy_point(cv, forms[:4], idx, rng), _lazy_point(cv, forms[4:], idx + 1 + (idx >> 2) % 3, rng), cm.GENERAL))
    for idx in range(64):  # the same forms, random limbs
        forms = ["n" if (idx >> j) & 1 else "p" for j in range(4)] + ["n" if (idx >> (j + 2)) & 1 else "p" for j in range(4)]
        fam[cm.GENERAL].append(Case(_lazy_point(cv, forms[:4], 0, rng), _lazy_point(cv, forms[4:], 0, rng), cm.GENERAL))
    for pat in range(12):  # limb class 2 proper on every coordinate, the twelve pairs of different sign patterns
        fam[cm.GENERAL].append(Case(_lazy_point(cv, "CCCC", pat & 3, rng), _lazy_point(cv, "CCCC", (pat & 3) + 1 + (pat >> 2), rng), cm.GENERAL))
    for idx in range(16):  # B = A and B = -A at the edges of P and N; |V| < 5 p, the range of a stored X3 (xyzz_dbl doubles y and
        forms = ["N" if (idx >> j) & 1 else "P" for j in range(4)]  # triples x^2 before it multiplies: 16 p would leave f_mul's range)
        a = _lazy_point(cv, forms, idx, rng, TOP_5P)
        fam[cm.DOUBLE].append(Case(a, a, cm.DOUBLE))
        fam[cm.CANCEL].append(Case(a, _negate_y(cv, a), cm.CANCEL))
    return fam


# what every eight consecutive quads of the main run hold: five different branches
PATTERN = (cm.GENERAL, cm.A_IDENTITY, cm.DOUBLE, cm.GENERAL, cm.B_IDENTITY, cm.CANCEL, cm.GENERAL, cm.DOUBLE)
RARE = (cm.DOUBLE, cm.CANCEL, cm.A_IDENTITY, cm.B_IDENTITY)
TAIL = (cm.GENERAL, cm.DOUBLE, cm.CANCEL, cm.A_IDENTITY, cm.GENERAL)


@functools.lru_cache(maxsize=None)
def qadd_layout(g):
    """(cases in launch order, quads of the main run): the main run cycles PATTERN; then one wave each where all quads take
    the same rare branch; then a last block that is not full"""
    cv = cm.CURVES[g]
    fam = qadd_families(g)
    nxt = {k: 0 for k in fam}

    def take(kind):
        c = fam[kind][nxt[kind] % len(fam[kind])]
        nxt[kind] += 1
        return c

    main = -(-len(fam[cm.GENERAL]) // 3) * 8
    main = -(-main // cv.NPB) * cv.NPB
    cases = [take(PATTERN[i % 8]) for i in range(main)]
    for kind in RARE:
        cases += [take(kind) for _ in range(64 // cv.GL)]
    cases += [take(kind) for kind in TAIL]
    assert all(nxt[k] >= len(fam[k]) for k in fam), "a family is not used up"
    return cases, main


def test_device_program_builds_with_the_products_flags(exe):
    """The program cross-compiles for gfx950 with the product's flags and holds every operation for both groups; its layout
    constants are the test's."""
    res = subprocess.run([exe, "--list"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    for op in ("qadd", "qtree", "rowcol_bits", "qfixup", "qfixup_chain", "qfixup_heavy"):
        for g in GROUPS:
            assert f"{op}_{g}" in lines
    assert f"pad {PAD} pt_g1 {cm.G1.PT} pt_g2 {cm.G2.PT} quads_g1 {cm.G1.NPB} quads_g2 {cm.G2.NPB} qfix_heavy {QFIX_HEAVY}" in lines


@pytest.mark.parametrize("g", GROUPS)
def test_reference_forms_agree_on_curve(g):
    """add-2008-s / dbl-2008-s mod p and the affine chord-and-tangent law give the same point for on-curve operands in every
    branch, whatever the representation; the formula's result keeps ZZ^3 = ZZZ^2."""
    cv = cm.CURVES[g]
    seen = set()
    for fam in qadd_families(g).values():
        for c in fam:
            if c.geo is None:
                continue
            A, B = cv.unpack(c.a), cv.unpack(c.b)
            assert (cv.affine(A), cv.affine(B)) == c.geo
            res, kind = cv.formula_add(A, B)
            assert kind == c.kind
            assert cv.affine(res) == cv.grp.add(*c.geo), kind
            assert cv.is_identity(res) or cv.consistent(res)
            seen.add(kind)
    assert seen == set(cm.BRANCHES)
    # a chain of collinear multiples: every partial sum by the formulas is the integer sum times P
    rng = _rng("agree" + g)
    acc, total = (cv.zero,) * 4, 0
    for m in rng.integers(-3, 4, size=60):
        acc, _ = cv.formula_add(acc, cv.rand_rep(multiples(g)[int(m)], rng))
        total += int(m)
        assert cv.affine(acc) == cv.times(total, base_point(g))


@pytest.mark.parametrize("g", GROUPS)
def test_qadd_cases_take_the_branches_they_claim_wave_by_wave(g):
    """The model's branch classifier over the limbs that are sent: every case takes the branch its family names; every wave
    of the main run holds at least four different branches among its quads; four waves follow in which all quads take the
    same rare branch; the last block is not full; the lazy forms are what the header says."""
    cv = cm.CURVES[g]
    cases, main = qadd_layout(g)
    kinds = [cv.classify(cv.unpack(c.a), cv.unpack(c.b)) for c in cases]
    assert kinds == [c.kind for c in cases]
    qw = 64 // cv.GL  # quads of a wave
    assert main % cv.NPB == 0 and main >= 2 * cv.NPB
    for w in range(main // qw):
        assert len(set(kinds[w * qw:(w + 1) * qw])) >= 4, w
    for j, kind in enumerate(RARE):
        assert kinds[main + j * qw:main + (j + 1) * qw] == [kind] * qw
    assert len(cases) == main + cv.NPB + len(TAIL) and len(cases) % cv.NPB == len(TAIL)
    rng = _rng("forms")
    ends = set()
    for pat in range(4):
        n = np.array(_form("N", pat, rng))
        assert 0 <= n[0] < 1 << 28 and n[1:13].min() >= -3 and n[1:13].max() <= (1 << 28) + 2
        ends |= {int(n[1:13].min()), int(n[1:13].max())}
        assert max(abs(v) for v in _form("C", pat, rng)[:13]) == (1 << 29) - 1
    assert ends >= {-3, (1 << 28) + 2}
    if cv.f2:  # the near-collisions are there, in both branches
        fam = qadd_families(g)
        assert sum(c.geo is None and c.b[2 * cv.W:2 * cv.W + fm.FP_L] == fm.fp_mont(1) for c in fam[cm.GENERAL]) == 6
        assert sum(c.geo is None and c.b[2 * cv.W:2 * cv.W + fm.FP_L] == fm.fp_mont(1) for c in fam[cm.CANCEL]) == 2


def _in(lo, v, hi):
    return lo < v < hi


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_qadd_on_device(exe, g):
    """q_add, a quad (eight lanes) per pair, 256-thread blocks, the branches mixed inside every wave."""
    cv = cm.CURVES[g]
    cases, _ = qadd_layout(g)
    n = len(cases)
    x = np.array([c.a + c.b for c in cases], dtype=np.int64)
    flat = run(exe, f"qadd_{g}", n, [x])
    rows, end = take_points(cv, flat, 0, n, "qadd")
    assert end == len(flat)
    for i, (c, row) in enumerate(zip(cases, rows)):
        what = f"{g} case {i} ({c.kind})"
        got = [int(w) for w in row]
        A, B = cv.unpack(c.a), cv.unpack(c.b)
        want, kind = cv.formula_add(A, B)
        if kind == cm.B_IDENTITY:
            assert got == c.a, f"{what}: A + O is not A limb for limb"
        elif kind == cm.A_IDENTITY:
            assert got == c.b, f"{what}: O + B is not B limb for limb"
        elif kind == cm.CANCEL:
            assert not any(got), f"{what}: P + (-P) is not the all-zero identity"
        else:
            res = cv.unpack(got)
            assert res == want, f"{what}: wrong residue in coordinate {[a == b for a, b in zip(res, want)].index(False)}"
            assert limb_classes(cv, row).max() <= 2, f"{what}: a stored coordinate at limb class {limb_classes(cv, row).max()}"
            vals = cm.limb_values(np.asarray(row).reshape(4, cv.comps, fm.FP_L))  # (coordinate, component)
            for k in range(cv.comps):
                X, Y, ZZ, ZZZ = (int(vals[j][k]) for j in range(4))
                assert _in(-4 * P, X, 2 * P), f"{what}: X3 = {X / P:.3f} p"
                ylim = (-P // 4, 5 * P // 4) if kind == cm.GENERAL else (-3 * P // 2, 3 * P // 2)
                assert _in(ylim[0], Y, ylim[1]), f"{what}: Y3 = {Y / P:.3f} p"
                assert _in(-P // 4, ZZ, 5 * P // 4) and _in(-P // 4, ZZZ, 5 * P // 4), f"{what}: ZZ3, ZZZ3 = {ZZ / P:.3f} p, {ZZZ / P:.3f} p"
        if c.geo is not None:
            res = cv.unpack(got)
            assert cv.affine(res) == cv.grp.add(*c.geo), f"{what}: not the oracle's sum"
            assert cv.is_identity(res) or cv.consistent(res), f"{what}: ZZ^3 != ZZZ^2"


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_qtree_on_device(exe, g):
    """q_block_tree over groups of 1, 2, .. all the block's quads: three blocks, the last not full.  Collinear points (every
    level of every tree meets equal and opposite operands, and identities); at the full group size also random points
    against the oracle's additions."""
    cv = cm.CURVES[g]
    rng = _rng("qtree" + g)
    n = 2 * cv.NPB + 5
    ms = rng.integers(-3, 4, size=n)
    x = collinear_words(cv, g, ms, rng)
    grp = 1
    while grp <= cv.NPB:
        flat = run(exe, f"qtree_{g}", n, [[grp], x])
        groups = -(-n // grp)
        rows, end = take_points(cv, flat, 0, groups, f"qtree {grp}")
        assert end == len(flat)
        for j in range(groups):
            if grp == 1:
                assert (rows[j] == x[j]).all(), f"{g} group size 1: point {j} changed"
            else:
                assert_multiple(cv, g, rows[j], ms[j * grp:(j + 1) * grp].sum(), f"{g} group size {grp}, group {j}")
        grp *= 2
    pts = random_points(g) + random_points(g)[:5][::-1] + random_points(g)[:cv.NPB]
    pts = pts[:n]
    flat = run(exe, f"qtree_{g}", n, [[cv.NPB], cm.pack_points(cv, [cv.rand_rep(p, rng) for p in pts])])
    rows, _ = take_points(cv, flat, 0, 3, "qtree random")
    for j in range(3):
        want = None
        for p in pts[j * cv.NPB:(j + 1) * cv.NPB]:
            want = cv.grp.add(want, p)
        assert cv.affine(cv.unpack([int(w) for w in rows[j]])) == want, f"{g} random points, block {j}"


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the reduction: k_qreduce_rowcol, k_qreduce_bits
# ---------------------------------------------------------------------------------------------------------------------------
# (cb, s, sets) on each side of every decision of msm_plan_tail (capi.hip): rc_s = 0 while 2^(cb - 1) <= 2 * 512 / GL, that is
# up to cb = 9 (G1) / 8 (G2), then (cb + 1) / 2; an odd cb has rows != cols; 15 is the largest window's bucket set.
RC_SHAPES = {
    "g1": [(1, 0, 1), (2, 0, 1), (3, 0, 1), (3, 0, 3), (6, 0, 1), (9, 0, 1), (10, 5, 1), (10, 5, 3), (11, 6, 1), (15, 8, 1)],
    "g2": [(1, 0, 1), (2, 0, 1), (3, 0, 1), (3, 0, 3), (6, 0, 1), (8, 0, 1), (9, 5, 1), (9, 5, 3), (10, 5, 1)],
}
RC_HYBRID = [(6, 3, 1), (7, 4, 1), (7, 4, 3)]  # capi.hip: cb2 with 2^cb2 >= segs, s2 = (cb2 + 1) / 2


def _np_sweep(cv, extra):
    """every block size, in quads, the host's launch expressions can give"""
    np_, out = 64 // cv.GL, []
    while np_ <= (256 if extra else 512) // cv.GL:
        out.append(np_)
        np_ *= 2
    return out


def _bit_sums(ms):
    """per set the integers [S, W_0, ..] of qtail.hpp's second level: S = sum_b m_b, W_k = the column sums (k < s) or row
    sums (k >= s) selected by bit k -- with b = hi 2^s + lo either is the sum of the m_b whose b has bit k, whatever s"""
    sets, nb = ms.shape
    cb = nb.bit_length() - 1
    b = np.arange(nb)
    return [[int(ms[t].sum())] + [int(ms[t][(b >> k) & 1 == 1].sum()) for k in range(cb)] for t in range(sets)]


def _run_reduction(cv, g, exe, cb, s, sets, extra, x, x2, what):
    """the operation at every block size: (quads, results as (sets, cb + 1, PT) words)"""
    nres = sets * (cb + 1)
    for np_ in _np_sweep(cv, extra):
        flat = run(exe, f"rowcol_bits_{g}", sets, [[cb, s, sets, np_, int(extra)], x] + ([x2] if extra else []))
        rows, end = take_points(cv, flat, 0, nres, what)
        assert end + 1 == len(flat)
        assert flat[end] == (POISON if extra else 0x1234567), f"{what}: the entry count did not ride along"
        yield np_, rows.reshape(sets, cb + 1, cv.PT)


@pytest.mark.gpu
@pytest.mark.parametrize("g,cb,s,sets", [(g, *sh) for g in GROUPS for sh in RC_SHAPES[g]])
def test_reduction_of_collinear_buckets_on_device(exe, g, cb, s, sets):
    """B[b] = m_b P, -3 <= m_b <= 3 (one bucket in seven the identity), each in a representation of its own: the cb + 1
    results of a set are the integers [S, W_0, ..] times P, and S + sum 2^k W_k = sum (b + 1) m_b."""
    cv = cm.CURVES[g]
    rng = _rng(f"rowcol{g}{cb}{s}{sets}")
    ms = rng.integers(-3, 4, size=(sets, 1 << cb))
    x = collinear_words(cv, g, ms.ravel(), rng)
    want = _bit_sums(ms)
    for t in range(sets):
        assert want[t][0] + sum(w << k for k, w in enumerate(want[t][1:])) == int(((np.arange(1 << cb) + 1) * ms[t]).sum())
    for np_, res in _run_reduction(cv, g, exe, cb, s, sets, False, x, None, f"{g} cb {cb} s {s} sets {sets}"):
        for t in range(sets):
            total = None
            for j in range(cb + 1):
                what = f"{g} cb {cb} s {s} set {t} of {sets}, {np_} quads: " + ("S" if j == 0 else f"W_{j - 1}")
                assert_multiple(cv, g, res[t, j], want[t][j], what)
                pt = cv.affine(cv.unpack([int(w) for w in res[t, j]]))
                total = cv.grp.add(total, pt if j == 0 else cv.times(1 << (j - 1), pt) if pt else None)
            assert total == multiple_of_base(g, int(((np.arange(1 << cb) + 1) * ms[t]).sum())), f"{g} cb {cb} set {t}: the set sum"


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("cb,s,sets", RC_HYBRID)
def test_hybrid_reduction_of_collinear_segments_on_device(exe, g, cb, s, sets):
    """The long sums' hybrid tail: rows and columns of the `run` sums, the plain total of the `acc` sums through extra / R2 /
    R0 -- S is the sum of the SECOND array, every W_k of the first."""
    cv = cm.CURVES[g]
    rng = _rng(f"hybrid{g}{cb}{sets}")
    ms = rng.integers(-3, 4, size=(sets, 1 << cb))
    ms2 = rng.integers(-3, 4, size=(sets, 1 << cb))
    x, x2 = collinear_words(cv, g, ms.ravel(), rng), collinear_words(cv, g, ms2.ravel(), rng)
    want = _bit_sums(ms)
    for t in range(sets):
        want[t][0] = int(ms2[t].sum())
    assert any(want[t][0] != int(ms[t].sum()) for t in range(sets))
    for np_, res in _run_reduction(cv, g, exe, cb, s, sets, True, x, x2, f"{g} hybrid cb {cb}"):
        for t in range(sets):
            for j in range(cb + 1):
                assert_multiple(cv, g, res[t, j], want[t][j], f"{g} hybrid cb {cb} set {t} of {sets}, {np_} quads, result {j}")


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("cb,s", [(3, 0), (6, 0), (6, 3)])
def test_reduction_of_distinct_points_on_device(exe, g, cb, s):
    """The control: distinct random points (no collisions), the reference by the oracle's additions.  (6, 3) is not a shape
    the plain plan picks; it runs the row / column level at a size the additions can follow."""
    cv = cm.CURVES[g]
    rng = _rng(f"control{g}{cb}{s}")
    pts = random_points(g)[:1 << cb]
    x = cm.pack_points(cv, [cv.rand_rep(p, rng) for p in pts])
    want = [None] * (cb + 1)
    for b, p in enumerate(pts):
        want[0] = cv.grp.add(want[0], p)
        for k in range(cb):
            if (b >> k) & 1:
                want[k + 1] = cv.grp.add(want[k + 1], p)
    for np_, res in _run_reduction(cv, g, exe, cb, s, 1, False, x, None, f"{g} control cb {cb}"):
        for j in range(cb + 1):
            pt = cv.unpack([int(w) for w in res[0, j]])
            assert cv.affine(pt) == want[j] and cv.consistent(pt), f"{g} control cb {cb} s {s}, {np_} quads, result {j}"


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the fix-up: k_qfixup, k_qfixup_chain, k_heavy_jobs / k_qfixup_heavy_part / k_qfixup_heavy
# ---------------------------------------------------------------------------------------------------------------------------
def eff_slice(E, T, M):
    """fixup_class.hpp"""
    m = (4 * E + T - 1) // max(T, 1)
    return M if m >= M else max(m, min(M, 4))


def heavy_chunk_of(span, npb):
    """msm.hpp"""
    s = 1
    while s * s * npb * npb < span:
        s += 1
    return npb * s


class FixCase:
    """A sorted list cut into slices of M entries: the buckets' offsets, the multipliers of the 2 T partial slots and, per
    bucket, what the fix-up must leave.  spec: ("empty",), ("whole",) or ("cut", d) with d = t1 - t0 slice boundaries inside
    the bucket.  T = ceil(E / M), for which eff_slice(E, T, M) = M whenever 3 E >= M."""

    def __init__(self, cv, g, spec, M, rng):
        pos, offs = 0, [0]
        for item in spec:
            if item[0] == "empty":
                size = 0
            elif item[0] == "whole":
                size = int(rng.integers(1, M - pos % M + 1))
            else:
                size = (pos // M + item[1]) * M + int(rng.integers(M)) + 1 - pos
            pos += size
            offs.append(pos)
        self.M, self.G, self.E, self.offs = M, len(spec), pos, offs
        self.T = -(-pos // M)
        assert eff_slice(self.E, self.T, M) == M
        self.ms = rng.integers(-3, 4, size=2 * self.T)
        self.parts = collinear_words(cv, g, self.ms, rng)
        self.kind, self.d, self.want = [], [], []
        for b in range(self.G):
            lo, hi = offs[b], offs[b + 1]
            if lo == hi:
                self.kind.append("empty"), self.d.append(0), self.want.append(0)
                continue
            t0, t1 = lo // M, (hi - 1) // M
            self.kind.append("whole" if t0 == t1 else "cut")
            self.d.append(t1 - t0)
            # the slots the kernels are defined to read: 2 t where the bucket covers the start of slice t, else 2 t + 1
            self.want.append(int(sum(self.ms[2 * t + (0 if lo <= t * M else 1)] for t in range(t0, t1 + 1))) if t0 != t1 else None)
        assert [k for k in self.kind] == [it[0] for it in spec] and [d for k, d in zip(self.kind, self.d) if k == "cut"] == [it[1] for it in spec if it[0] == "cut"]


def _run_fixup(cv, g, exe, fc, LPB, heavy):
    flat = run(exe, f"qfixup{'_heavy' if heavy else ''}_{g}", fc.G, [[fc.G, fc.M, fc.T, LPB], fc.offs, fc.parts])
    first, at = take_points(cv, flat, 0, fc.G, "k_qfixup")
    count, at = int(flat[at]), at + 1
    hlist, at = take_words(flat, at, fc.G, "heavy_list")
    if not heavy:
        assert at == len(flat)
        return first, count, hlist, None, None
    second, at = take_points(cv, flat, at, fc.G, "heavy kernels")
    job_base, at = take_words(flat, at, fc.G + 1, "job_base")
    assert at == len(flat)
    return first, count, hlist, second, job_base


def _check_fixup(cv, g, fc, LPB, first, count, hlist, second, job_base, what):
    heavy = [b for b in range(fc.G) if fc.kind[b] == "cut" and fc.d[b] >= QFIX_HEAVY * LPB]
    assert count == len(heavy) and sorted(int(v) for v in hlist[:count]) == heavy, f"{what}: heavy_list {sorted(hlist[:count])} != {heavy}"
    assert (hlist[count:] == POISON).all()
    for b in range(fc.G):
        w = f"{what}: bucket {b} ({fc.kind[b]}, d = {fc.d[b]})"
        if fc.kind[b] == "empty":
            assert not first[b].any(), f"{w}: an empty bucket must receive the all-zero identity"
        elif fc.kind[b] == "whole" or b in heavy:
            assert is_poison(first[b]), f"{w}: k_qfixup wrote a bucket that is not its own"
        else:
            assert_multiple(cv, g, first[b], fc.want[b], w)
    if second is None:
        return
    spans = []
    for h, b in enumerate(int(v) for v in hlist[:count]):
        span = fc.d[b] + 1
        spans.append(-(-span // heavy_chunk_of(span, cv.NPB)))
        assert job_base[h + 1] - job_base[h] == spans[-1], f"{what}: jobs of heavy bucket {b}"
    assert count == 0 or job_base[0] == 0
    for b in range(fc.G):
        if b in heavy:
            assert_multiple(cv, g, second[b], fc.want[b], f"{what}: heavy bucket {b} (d = {fc.d[b]})")
        else:
            assert (second[b] == first[b]).all(), f"{what}: the heavy kernels wrote bucket {b}, which is not heavy"
    return spans


def _lpbs(cv):
    out, v = [], 1
    while v <= cv.NPB:
        out.append(v)
        v *= 2
    return out


def _fix_spec(cv, LPB, rng):
    """every kind of bucket at the spans 1, 2, LPB - 1, LPB, LPB + 1 and on both sides of the heavy threshold
    d >= QFIX_HEAVY LPB; more buckets than one block takes, and not a multiple of the buckets per block"""
    ds = sorted({d for d in (1, 2, LPB - 1, LPB, LPB + 1, QFIX_HEAVY * LPB - 1, QFIX_HEAVY * LPB, QFIX_HEAVY * LPB + 1) if d >= 1})
    unit = [("empty",), ("whole",)] + [("cut", d) for d in ds] + [("whole",), ("empty",)]
    per_block = cv.NPB // LPB
    spec = []
    while len(spec) < 2 * per_block + 1:
        spec += [unit[i] for i in rng.permutation(len(unit))]
    if per_block > 1 and len(spec) % per_block == 0:
        spec.append(("whole",))
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize("g,LPB", [(g, v) for g in GROUPS for v in _lpbs(cm.CURVES[g])])
def test_fixup_of_cut_buckets_on_device(exe, g, LPB):
    """k_qfixup at every quads-per-bucket count, then the heavy kernels over the list it left: an empty bucket receives the
    identity, an uncut one keeps the poison, a cut one is the sum of its slots, one that spans more than QFIX_HEAVY x LPB
    slices is listed exactly once, left alone by k_qfixup and written by the heavy kernels, which write nothing else."""
    cv = cm.CURVES[g]
    rng = _rng(f"fixup{g}{LPB}")
    spec = _fix_spec(cv, LPB, rng)
    fc = FixCase(cv, g, spec, 2 if LPB > 4 else 4, rng)
    per_block = cv.NPB // LPB
    assert fc.G > per_block and (per_block == 1 or fc.G % per_block != 0)
    assert {d for k, d in zip(fc.kind, fc.d) if k == "cut"} >= {2, LPB + 1, QFIX_HEAVY * LPB - 1, QFIX_HEAVY * LPB}
    res = _run_fixup(cv, g, exe, fc, LPB, True)
    _check_fixup(cv, g, fc, LPB, *res, f"{g} LPB {LPB}")
    if LPB == 2:  # the plain operation: k_qfixup alone
        res = _run_fixup(cv, g, exe, fc, LPB, False)
        _check_fixup(cv, g, fc, LPB, *res, f"{g} LPB {LPB} (k_qfixup alone)")


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_heavy_buckets_of_one_job_and_of_more_jobs_than_quads_on_device(exe, g):
    """LPB = 1: buckets of d >= 16 are heavy.  One of a single job, one of a few, and one of more jobs than a block has quads
    (65 G1 / 33 G2: the second level's strided loop runs twice before its tree)."""
    cv = cm.CURVES[g]
    rng = _rng("giant" + g)
    big = 8200 if g == "g1" else 2100
    spec = [("whole",), ("cut", 1), ("cut", 20), ("empty",), ("cut", big), ("cut", 2), ("cut", 3 * cv.NPB - 1), ("whole",), ("cut", 15), ("cut", 16)]
    fc = FixCase(cv, g, spec, 2, rng)
    res = _run_fixup(cv, g, exe, fc, 1, True)
    spans = _check_fixup(cv, g, fc, 1, *res, f"{g} heavy")
    assert sorted(spans) == [1, 1, 3, cv.NPB + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_chain_fixup_on_device(exe, g):
    """k_qfixup_chain: a quad per listed bucket adds its 3 .. 8 slots in a row; lists of 0, 1 and more entries than one round
    of the grid takes (max_chain, the host's bound on the list, sizes the grid: 1 gives one block, so 2 NPB + 3 entries are
    three strides; the list's own length gives two blocks and two strides).  Unlisted buckets keep the poison."""
    cv = cm.CURVES[g]
    rng = _rng("chain" + g)
    spec = []
    for i in range(2 * cv.NPB + 3):
        spec += [("cut", 2 + i % 6)] + ([("whole",)] if i % 3 == 0 else []) + ([("empty",)] if i % 7 == 0 else []) + ([("cut", 1)] if i % 5 == 0 else [])
    fc = FixCase(cv, g, spec, 4, rng)
    chain = [b for b in range(fc.G) if fc.kind[b] == "cut" and fc.d[b] >= 2]
    assert len(chain) == 2 * cv.NPB + 3
    order = [chain[i] for i in rng.permutation(len(chain))]
    for listed, max_chain in (([], 1), (order[:1], 1), (order, 1), (order, len(order) - cv.NPB)):
        flat = run(exe, f"qfixup_chain_{g}", fc.G, [[fc.G, fc.M, fc.T, len(listed), max_chain], fc.offs, listed, fc.parts])
        rows, end = take_points(cv, flat, 0, fc.G, "k_qfixup_chain")
        assert end == len(flat)
        for b in range(fc.G):
            what = f"{g} chain list of {len(listed)}, max_chain {max_chain}: bucket {b} (d = {fc.d[b]})"
            if b in listed:
                assert_multiple(cv, g, rows[b], fc.want[b], what)
            else:
                assert is_poison(rows[b]), f"{what}: written, but not listed"
