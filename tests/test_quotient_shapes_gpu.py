"""The QAP quotient and Poly.Mul at the sizes where their kernel sequences change, against exact CPU references.

Every transform size of ps_poly_mul from 2^1 to 2^22 (one, two and three NTT passes, ntt.hpp), the quotient at gate counts
that are not powers of two across the pass boundaries of its convolutions (qap_tables_build's n != np and np_h != np
branches, the batch of three at three passes), R1CS rows of every length around the SpMV kernels' hand-off
(SPMV_LONG_ROW = 512) with int64 coefficients at their extremes, and both setups and provers on a circuit whose transposed
matrices have long rows.  Expected values come from the C oracle (schoolbook products, Horner evaluation, the fast CPU
quotient), restate.lagrange_at and closed forms; the unmarked tests check those helpers (tests/quotient_cases.py) without a
GPU.

What the cases reach (log2 size: stages per pass, quotient_cases.ntt_passes):
  * Poly.Mul, ntt_run forward and inverse: every p = 1..22, i.e. one pass (p <= 10), (6,5) .. (9,9) (p = 11..18) and
    (7,6,6) .. (8,7,7) (p = 19..22); the inverse's early scaling (more than 16 unscaled stages) from p = 17 on.
  * the quotient, ntt_conv: n = 513 .. 2^17+1 byte for byte (conv up to 2^19 = (7,6,6), batch of three at 2^19 for 2^17+1),
    2^18+3 (conv 2^20 = (7,7,6)) and 2^20+1 (conv 2^22 = (8,7,7), h interpolated at 2^21 = (7,7,7)) by exact evaluation;
    np_h != np at 513, 1025, 4097, 2^16+1, 2^17+1 and 2^20+1, z from the Newton form (n != np) everywhere.
  * k_spmv / k_spmv_long_rows on the gate matrices: L rows of 1 .. 100 003 entries, 512 the last the per-row kernel owns;
    on the transposed matrices (the setups): rows of 512, 513 and over 1025 entries.
"""
import functools
import operator
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_cases as qc  # noqa: E402

SEED = 0x7175_6F74_6965_6E74
R = qc.R

MUL_CASES = [(p, na, nb) for p in range(1, 23) for na, nb in qc.mul_length_pairs(p)]
MUL_CLASSES = ("random", "minus_one", "monomials", "top")
QUOTIENT_EXACT_N = (513, 1000, 1025, 4097, 40000, (1 << 16) - 1, (1 << 16) + 1, (1 << 17) + 1)
QUOTIENT_EVAL_N = ((1 << 18) + 3, (1 << 20) + 1)
R_WORDS = tuple((R >> (64 * (3 - i))) & (2**64 - 1) for i in range(4))


def _all_below_r(raw: bytes) -> bool:
    """Every 32-byte big-endian word of raw is < r (lexicographic on the four 64-bit words)."""
    import numpy as np

    w = np.frombuffer(raw, dtype=">u8").reshape(-1, 4)
    below = np.zeros(len(w), dtype=bool)
    equal = np.ones(len(w), dtype=bool)
    for i, rw in enumerate(R_WORDS):
        below |= equal & (w[:, i] < rw)
        equal &= w[:, i] == rw
    return bool(below.all())


def _mul_inputs(cls: str, p: int, na: int, nb: int):
    """(a, b, exact product or None) as bytes; None: the product is checked by evaluation and sampled coefficients."""
    seed = SEED + 1000 * p + na
    rng = qc.pr.SplitMix64(seed)
    if cls == "random":
        a, b = qc.random_fr_bytes(na, seed), qc.random_fr_bytes(nb, seed + 1)
        if p <= 13:
            return a, b, qc.co.pack_fr(qc.co.poly_mul(qc.ints(a), qc.ints(b)))
        return a, b, None
    if cls == "minus_one":
        return qc.const_fr_bytes(na, R - 1), qc.const_fr_bytes(nb, R - 1), qc.all_minus_one_product(na, nb)
    if cls == "monomials":  # u x^i * v x^j = uv x^(i+j)
        i, j = rng.next() % na, rng.next() % nb
        u, v = rng.fr(), rng.fr()
        return qc.monomial_bytes(na, i, u), qc.monomial_bytes(nb, j, v), qc.monomial_bytes(na + nb - 1, i + j, u * v % R)
    # a = u x^(na-1): the product is b shifted to the top (u = 1 above 2^13, where a Python loop over b costs seconds)
    u = rng.fr() if p <= 13 else 1
    b = qc.random_fr_bytes(nb, seed + 2)
    want = bytes(32 * (na - 1)) + (b if u == 1 else qc.co.pack_fr([u * v % R for v in qc.ints(b)]))
    return qc.monomial_bytes(na, na - 1, u), b, want


@pytest.mark.gpu
@pytest.mark.parametrize("cls", MUL_CLASSES)
@pytest.mark.parametrize("p,na,nb", MUL_CASES, ids=[f"p{p}-{na}x{nb}" for p, na, nb in MUL_CASES])
def test_poly_mul_every_transform_size(ps_api, ctx, p, na, nb, cls):
    """Poly.Mul (ps_poly_mul: forward transforms of both factors, point-wise product, inverse) at transform size 2^p."""
    a, b, want = _mul_inputs(cls, p, na, nb)
    got = ps_api.Poly.upload(ctx, a).Mul(ps_api.Poly.upload(ctx, b)).download_bytes()
    nc = na + nb - 1
    assert len(got) == 32 * nc
    assert _all_below_r(got)
    if want is not None:
        assert got == want
        return
    # c(t) = a(t) b(t) at three random points: a wrong product passes with probability <= 2^p / r per point
    rng = qc.pr.SplitMix64(SEED + p)
    for _ in range(3):
        t = rng.fr()
        assert qc.eval_bytes(got, t) == qc.eval_bytes(a, t) * qc.eval_bytes(b, t) % R
    # and exact coefficients where a transform's structure changes: the ends, the tile (2^10) and the middle
    for i in sorted({0, 1, 1023, 1024, (1 << (p - 1)) - 1, 1 << (p - 1), nc // 2, nc - 1}):
        if i < nc:
            assert int.from_bytes(got[32 * i : 32 * i + 32], "big") == qc.conv_coeff(a, b, i), i


def _permutation_qap(ps_api, ctx, n):
    nv, nio, mats, sol, ys = qc.permutation_circuit(n, SEED + n)
    q = ps_api.QAP.from_csr(ctx, nv, nio, *mats)
    return q, ps_api.Poly.upload(ctx, sol), ys


@pytest.mark.gpu
@pytest.mark.parametrize("n", QUOTIENT_EXACT_N)
def test_quotient_non_power_of_two_byte_exact(ps_api, ctx, co, n):
    """Every route of the quotient at n gates != 2^k, byte for byte against the oracle's fast quotient of the exact values:
    computeAggregatePoly (A, B, C, h), computeAB (Groth16's route, h by division), Quotient (h from its values on
    n+1..2n-1), interpolate (each aggregate alone) and IsValid."""
    q, dsol, ys = _permutation_qap(ps_api, ctx, n)
    want = co.fast_quotient_bytes(*ys, n)
    got = tuple(p.download_bytes() for p in q.computeAggregatePoly(dsol))
    for name, g, w in zip("ABCh", got, want):
        assert g == w, name
    A, B, h = (p.download_bytes() for p in q.computeAB(dsol))
    assert (A, B, h) == (want[0], want[1], want[3])
    assert q.Quotient(dsol).download_bytes() == want[3]
    for k in range(3):
        assert q.interpolate(dsol, k).download_bytes() == want[k], k
    assert q.IsValid(dsol) is True


@pytest.mark.gpu
@pytest.mark.parametrize("n", QUOTIENT_EVAL_N)
def test_quotient_three_pass_by_exact_evaluation(ps_api, ctx, co, pr, n):
    """Beyond the oracle's byte-exact reach: A(t) = sum_j y_j l_j(t) (and B, C) at a random t with restate.lagrange_at, the
    QAP identity A(t) B(t) - C(t) = h(t) z(t), deg h = n - 2, and the same h bytes from the other two routes."""
    from oracle import restate as rs

    q, dsol, ys = _permutation_qap(ps_api, ctx, n)
    got = tuple(p.download_bytes() for p in q.computeAggregatePoly(dsol))
    for g in got:
        assert _all_below_r(g)
    assert [len(g) // 32 for g in got] == [n, n, n, n - 1]
    t = pr.SplitMix64(SEED + n).fr()
    lj, zt = rs.lagrange_at(n, t)
    at = []
    for name, poly, y in zip("ABC", got, ys):
        want = sum(map(operator.mul, qc.ints(y), lj)) % R
        at.append(qc.eval_bytes(poly, t))
        assert at[-1] == want, name
    assert (at[0] * at[1] - at[2]) % R == qc.eval_bytes(got[3], t) * zt % R
    assert q.Quotient(dsol).download_bytes() == got[3]
    assert tuple(p.download_bytes() for p in q.computeAB(dsol)) == (got[0], got[1], got[3])


def _dense_qap(ps_api, ctx, c):
    return ps_api.QAP.from_csr(ctx, c.nbVars, c.nbIO, *(qc.csr_of(rows) for rows in (c.left, c.right, c.out)))


def _off_by_one(b):
    """The witness with the first column of the 512-entry dense row moved by one; that gate no longer holds."""
    j = qc.DENSE_LENGTHS.index(512)
    v = b.left[j][0][0]
    bad = list(b.sol)
    bad[v] = (bad[v] + 1) % R
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("witness", ("minus_one", "random"))
@pytest.mark.parametrize("kind", qc.COEF_CLASSES)
def test_dense_rows_byte_exact(ps_api, ctx, co, kind, witness):
    """L rows of 1 .. 100 003 entries (the per-row SpMV with its periodic reduction, and the workgroup-per-row kernel above
    512) with int64 coefficients of one class and repeated columns: y through interpolate and every quotient route byte for
    byte against the oracle, IsValid; then a witness off by one is invalid and Quotient raises Apocalypse."""
    b = qc.dense_circuit(kind, witness, 1025, seed=SEED % 1000 + qc.COEF_CLASSES.index(kind))
    c = b.circuit()
    n = c.nbGates
    want = co.fast_quotient_bytes(*qc.values_bytes(c, b.sol), n)
    q = _dense_qap(ps_api, ctx, c)
    dsol = ps_api.Poly.upload(ctx, co.pack_fr(b.sol))
    for k in range(3):
        assert q.interpolate(dsol, k).download_bytes() == want[k], k
    got = tuple(p.download_bytes() for p in q.computeAggregatePoly(dsol))
    for name, g, w in zip("ABCh", got, want):
        assert g == w, name
    assert q.Quotient(dsol).download_bytes() == want[3]
    assert q.IsValid(dsol) is True
    bad = ps_api.Poly.upload(ctx, co.pack_fr(_off_by_one(b)))
    assert q.IsValid(bad) is False
    with pytest.raises(ps_api.Apocalypse):
        q.Quotient(bad)


@functools.lru_cache(maxsize=1)
def _long_transposed():
    b = qc.transposed_long_circuit(1025, seed=SEED % 997)
    return b.circuit(), b.sol


@pytest.mark.gpu
def test_groth16_setup_and_proofs_with_long_transposed_rows(ps_api, ctx, co, pr):
    """NewGroth16TrustedSetup on a circuit whose transposed matrices hold rows of 512, 513 and over 1025 entries (the
    per-variable sums u_i(x), v_i(x), w_i(x)), every CRS array against restate.groth16_setup; then proofs over the
    Lagrange-form key (h by its values, quotient_h_values) and over the monomial key equal the oracle's proof."""
    from oracle import restate as rs

    c, sol = _long_transposed()
    rng = pr.SplitMix64(SEED + 64)
    tox = [rng.fr() for _ in range(5)]
    want = rs.groth16_setup(c, *tox)
    q = _dense_qap(ps_api, ctx, c)
    tr, vk = ps_api.NewGroth16TrustedSetup(q, *tox)
    assert (tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2, vk["Gamma"]) == (
        want.Alpha, want.Beta, want.Delta, want.Beta2, want.Delta2, want.Gamma)
    assert tr.Xi.download() == want.Xi
    assert tr.Xi2.download() == want.Xi2
    assert tr.XiT.download() == want.XiT
    assert tr.NioLP.download() == want.NioLP
    assert vk["IoLP"].download() == want.IoLP
    r, s = rng.fr(), rng.fr()
    ref = rs.groth16_prove(want, c, sol, r, s, fast=True)
    dsol = ps_api.Poly.upload(ctx, co.pack_fr(sol))
    for key in (tr, tr.monomial_only()):
        proof = ps_api.Groth16Prove(key, q, dsol, r, s)
        assert (proof.A, proof.B, proof.C) == (ref.A, ref.B, ref.C)


@pytest.mark.gpu
def test_phgr13_setup_and_proofs_with_long_transposed_rows(ps_api, ctx, co, pr):
    """NewPHGR13TrustedSetup on the same circuit: the ten evaluation-key arrays and vk.vs / ws / ys against
    restate.phgr13_setup; proofs over lgsi (h by its values) and over gsi (h by its coefficients) equal the oracle's."""
    from oracle import restate as rs

    c, sol = _long_transposed()
    rng = pr.SplitMix64(SEED + 93)
    tox = [rng.fr() for _ in range(8)]
    want = rs.phgr13_setup(c, *tox)
    q = _dense_qap(ps_api, ctx, c)
    ek, vk = ps_api.NewPHGR13TrustedSetup(q, *tox)
    for f in ps_api.PHGR13EvalKey.FIELDS:
        assert getattr(ek, f).download() == getattr(want.EK, f), f
    assert vk.vs.download() == co.G1.pack(want.VK.vs)
    assert vk.ws.download() == co.G2.pack(want.VK.ws)
    assert vk.ys.download() == co.G1.pack(want.VK.ys)
    ref = rs.phgr13_prove(want.EK, c, sol, fast=True)
    dsol = ps_api.Poly.upload(ctx, co.pack_fr(sol))
    assert ek.lgsi is not None
    for key in (ek, ek.monomial_only()):
        proof = ps_api.PHGR13Prove(key, q, dsol)
        for f in ps_api.PHGR13Proof.FIELDS:
            assert getattr(proof, f) == getattr(ref, f), f


# ---------------------------------------------------------------------------------------
# CPU self-checks of the cases and their references (no GPU)
# ---------------------------------------------------------------------------------------
def test_mul_cases_reach_every_pass_shape():
    seen = {}
    for p, na, nb in MUL_CASES:
        assert qc.ilog2_ceil(na + nb - 1) == p, (p, na, nb)
        assert 1 <= na and 1 <= nb
        seen.setdefault(p, set()).add((na, nb))
    assert sorted(seen) == list(range(1, 23))
    assert all(len(v) == 3 for p, v in seen.items() if p >= 3)
    shapes = {qc.ntt_passes(p) for p in seen}
    assert {s for s in shapes if len(s) == 2} == {(6, 5), (6, 6), (7, 6), (7, 7), (8, 7), (8, 8), (9, 8), (9, 9)}
    assert {s for s in shapes if len(s) == 3} == {(7, 6, 6), (7, 7, 6), (7, 7, 7), (8, 7, 7)}
    assert [p for p in seen if len(qc.ntt_passes(p)) == 1] == list(range(1, 11))


def test_quotient_cases_reach_every_convolution_shape_and_branch():
    sizes = {n: qc.quotient_conv_sizes(n) for n in QUOTIENT_EXACT_N + QUOTIENT_EVAL_N}
    conv = set().union(*(s["interpolate"] | s["h_values"] | s["h_interpolate"] | s["product"] for s in sizes.values()))
    assert set(range(7, 23)) <= conv
    exact = set().union(*(s["interpolate"] | s["h_interpolate"] | s["product"] for n, s in sizes.items() if n in QUOTIENT_EXACT_N))
    assert set(range(7, 20)) <= exact  # byte-exact up to (7,6,6)
    assert not any(s["n_is_np"] for s in sizes.values())
    assert sorted(n for n, s in sizes.items() if s["np_h_differs"]) == [513, 1025, 4097, 65537, 131073, (1 << 20) + 1]
    assert sizes[(1 << 17) + 1]["h_values"] == {19} and len(qc.ntt_passes(19)) == 3  # the batch of three, three passes
    assert sizes[513]["h_values"] == {11} and sizes[513]["h_interpolate"] == {10} | set(range(7, 10))  # 1-pass h
    assert qc.ntt_passes(max(sizes[(1 << 18) + 3]["h_values"])) == (7, 7, 6)
    assert qc.ntt_passes(max(sizes[(1 << 20) + 1]["h_values"])) == (8, 7, 7)


def test_all_minus_one_closed_form_and_convolution_sums(co):
    for na, nb in ((1, 1), (1, 7), (5, 3), (8, 8), (33, 9), (64, 65)):
        a, b = [R - 1] * na, [R - 1] * nb
        assert qc.ints(qc.all_minus_one_product(na, nb)) == co.poly_mul(a, b)
        ra, rb = qc.random_fr_bytes(na, na), qc.random_fr_bytes(nb, nb + 100)
        want = co.poly_mul(qc.ints(ra), qc.ints(rb))
        assert [qc.conv_coeff(ra, rb, i) for i in range(na + nb - 1)] == want
        t = 0x1234567 * na + nb
        assert qc.eval_bytes(co.pack_fr(want), t) == co.poly_eval(want, t)


def test_random_bytes_are_field_elements_and_inputs_have_the_promised_form():
    raw = qc.random_fr_bytes(4096, 5)
    v = qc.ints(raw)
    assert _all_below_r(raw) and max(v) < R and max(v) > R // 2
    assert not _all_below_r(qc.const_fr_bytes(3, R - 1) + R.to_bytes(32, "big"))
    assert qc.ints(qc.small_fr_bytes([0, 1, 2**64 - 1])) == [0, 1, 2**64 - 1]
    for cls in MUL_CLASSES:
        for p, na, nb in ((3, 1, 8), (9, 256, 257), (12, 4089, 8)):
            a, b, want = _mul_inputs(cls, p, na, nb)
            assert qc.ints(want) == qc.co.poly_mul(qc.ints(a), qc.ints(b)), (cls, p)


@pytest.mark.parametrize("witness", ("minus_one", "random"))
@pytest.mark.parametrize("kind", qc.COEF_CLASSES)
def test_dense_builder_circuits_are_satisfied(co, kind, witness):
    """The circuits of test_dense_rows_byte_exact hold (the oracle's quotient exists), have the promised rows, and the
    off-by-one witness does not hold."""
    b = qc.dense_circuit(kind, witness, 1025, seed=SEED % 1000 + qc.COEF_CLASSES.index(kind))
    c = b.circuit()
    assert c.nbGates == 1025
    assert [len(r) for r in c.left[: len(qc.DENSE_LENGTHS)]] == list(qc.DENSE_LENGTHS)
    for row in c.left[1 : len(qc.DENSE_LENGTHS)]:
        assert row[0][0] == row[-1][0]  # a repeated column in every dense row
        assert all(-(1 << 63) <= v < (1 << 63) for _, v in row)
    if kind.startswith("int64"):
        assert c.left[-1 + len(qc.DENSE_LENGTHS)][0][1] == (qc.INT64_MIN if kind == "int64_min" else qc.INT64_MAX)
    yA, yB, yC = c.values(b.sol)
    assert all(a * bb % R == cc for a, bb, cc in zip(yA, yB, yC))
    assert yA[qc.DENSE_LENGTHS.index(512)] != 0  # the hand-off row is not trivially zero
    co.fast_quotient_bytes(*qc.values_bytes(c, b.sol), c.nbGates)  # raises when z does not divide A B - C
    with pytest.raises(ArithmeticError):
        co.fast_quotient_bytes(*qc.values_bytes(c, _off_by_one(b)), c.nbGates)


def test_long_transposed_circuit_has_the_promised_rows(co):
    c, sol = _long_transposed()
    assert c.nbGates == 1025
    count = lambda rows, v: sum(1 for row in rows for col, _ in row if col == v)
    assert count(c.left, 1) > 1025 and all((1, -1) in row for row in c.left)
    assert count(c.right, 2) == 512
    assert count(c.out, 0) == 513
    assert max(len(r) for r in c.left) == 8194  # 8193 dense entries and variable 1
    yA, yB, yC = c.values(sol)
    assert all(a * bb % R == cc for a, bb, cc in zip(yA, yB, yC))
    co.fast_quotient_bytes(*qc.values_bytes(c, sol), c.nbGates)


def test_permutation_circuit_matches_its_sparse_form():
    from oracle import restate as rs

    n = 100
    nv, nio, mats, sol, ys = qc.permutation_circuit(n, 9)
    rows = []
    for ptr, col, val in mats:
        rows.append([[(int(col[e]), int(val[e])) for e in range(ptr[g], ptr[g + 1])] for g in range(n)])
    c = rs.SparseR1CS(nv, nio, *rows)
    assert qc.values_bytes(c, qc.ints(sol)) == ys
    yA, yB, yC = c.values(qc.ints(sol))
    assert all(a * b % R == cc for a, b, cc in zip(yA, yB, yC))
