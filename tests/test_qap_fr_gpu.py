"""GPU: R1CS matrices with full field coefficients (ps_qap_create_fr), through every layer.

  * the same circuit through either door (int64, or the same values mod r as field elements) gives the same bytes;
  * column sums over points with WIDE coefficients (signed magnitude of 2^64 or more: csrc/ec_spmv.hpp, the four-word
    kernels) against the oracle's group arithmetic term by term, shapes (1, 1), (4, 6), (65, 40), (600, 9) as in
    tests/test_column_sums_gpu.py;
  * both setups and provers on a MiMC-style circuit whose round constants are such coefficients, against oracle/restate.py;
  * the route without toxic waste (setup from a powers-of-tau string, fold, check) on 20, 68 and 1 120 gates -- at 1 120 the
    `const` column holds 560 (L) and 1 120 (R) wide entries, so one workgroup sums a long wide row inside the real setup;
  * errors."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_circuits as wc  # noqa: E402

pytestmark = pytest.mark.gpu

R = wc.R
ARRAYS = ("Xi", "Xi2", "NioLP", "XiT", "LXi", "LXi2", "LXiT")
FIXED = ("Alpha", "Beta", "Delta", "Beta2", "Delta2")
WIDE_POOL = tuple(v for v in wc.EDGE if wc.is_wide(v))
NARROW_POOL = tuple(v for v in wc.EDGE if not wc.is_wide(v)) + tuple(v % R for v in wc.I64_EDGE)


def _qap_fr(api, ctx, c):
    return api.QAP.from_csr(ctx, c.nbVars, c.nbIO, *(wc.csr_fr(rows) for rows in (c.left, c.right, c.out)))


# ---------------------------------------------------------------------------------------------------------------------
# the same circuit, either door
# ---------------------------------------------------------------------------------------------------------------------
def _int64_circuit(n):
    from oracle import pyref, restate as rs

    if n == 4:
        c, wit = rs.toy_circuit()
        return c, [pyref.fr(v) for v in wit]
    return rs.synthetic_circuit(n)


@pytest.mark.parametrize("n", [4, 40])
def test_same_circuit_through_either_door_gives_the_same_bytes(ps_api, ctx, pr, n):
    c, sol = _int64_circuit(n)
    qi = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    qf = _qap_fr(ps_api, ctx, c)
    assert qi.wide_entries() == (0, 0, 0) and qf.wide_entries() == (0, 0, 0)
    dsol = ps_api.Poly.upload(ctx, sol)
    for a, b in zip(qi.computeAggregatePoly(dsol), qf.computeAggregatePoly(dsol)):
        assert a.download() == b.download()
    assert qi.IsValid(dsol) and qf.IsValid(dsol)
    bad = list(sol)
    bad[-1] = (bad[-1] + 1) % R
    assert not qi.IsValid(ps_api.Poly.upload(ctx, bad)) and not qf.IsValid(ps_api.Poly.upload(ctx, bad))
    rng = pr.SplitMix64(4040 + n)
    P = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, [0 if g == 1 else rng.fr() for g in range(n)]))
    for which in range(3):
        assert qi.column_sums(which, P).download() == qf.column_sums(which, P).download()
    tox = [rng.fr() for _ in range(5)]
    r, s = rng.fr(), rng.fr()
    proofs = []
    for q in (qi, qf):
        tr, _ = ps_api.NewGroth16TrustedSetup(q, *tox)
        p = ps_api.Groth16Prove(tr, q, dsol, r, s)
        proofs.append((p.A, p.B, p.C))
    assert proofs[0] == proofs[1]
    qi.free()
    qf.free()


# ---------------------------------------------------------------------------------------------------------------------
# wide column sums against the oracle, term by term
# ---------------------------------------------------------------------------------------------------------------------
def _wide(rng):
    k = rng.next() % (len(WIDE_POOL) + 2)
    if k < len(WIDE_POOL):
        return WIDE_POOL[k]
    while True:
        v = rng.fr()
        if wc.is_wide(v):
            return v


def _narrow(rng):
    return NARROW_POOL[rng.next() % len(NARROW_POOL)]


def _sign(rng):
    return 1 if rng.next() & 1 else R - 1


def _case_1x1(pr):
    # one gate, one variable: the two largest magnitudes; O leaves the variable in no gate
    return 1, 1, [{0: [(0, (R - 1) // 2)]}, {0: [(0, (R + 1) // 2)]}, {}], [0x1234567]


def _case_toy(pr):
    a = 0xABCDEF0123456789
    ks = [a, 0, a, R - a]  # P0 = P2 (the same point twice), P1 the identity, P3 = -P0
    W = (1 << 253) + 5
    L = {
        0: [(0, (1 << 64) + 1), (2, (1 << 64) + 1)],          # P + P in every plane, bit 64 included: the doubling branch
        1: [(0, W), (3, W)],                                  # P + (-P), equal wide coefficients: the identity in mid-sum
        2: [(0, 1), (1, R - (1 << 64))],                      # an identity input under a wide coefficient
        # 3: in no gate
        4: [(0, 1 << 64), (2, 1 << 64), (3, 1 << 65)],        # 2^64 a + 2^64 a - 2^65 a: cancels only with the last addition
        5: [(0, (1 << 64) - 1), (1, 5), (2, 1 << 64), (3, R - 1)],  # 2^64 - 1 and 2^64 in one column
    }
    Rm = {0: [(0, 0), (1, (R - 1) // 2), (3, (R + 1) // 2)],  # an explicit zero, and the identity as the only other early term
          2: [(2, 1 << 254), (3, 1 << 254)],
          5: [(1, 1 << 64)]}                                  # the identity alone, wide
    O = {i: [(i % 4, R - (1 << 64))] for i in range(6)}
    return 4, 6, [L, Rm, O], ks


def _case_mid(pr):
    rng = pr.SplitMix64(65040)
    n, m = 65, 40
    ks = [0 if g % 11 == 3 else rng.fr() for g in range(n)]
    ks[20] = ks[10]
    ks[30] = R - ks[10]
    mats = []
    e = 0
    for _ in range(3):
        cols = {}
        for g in range(n):
            for col in sorted({rng.next() % (m - 1) for _ in range(1 + rng.next() % 3)}):  # (variable m - 1 stays in no gate)
                cols.setdefault(col, []).append((g, _wide(rng) if e % 3 == 0 else _narrow(rng)))
                e += 1
        mats.append(cols)
    w = _wide(rng)
    mats[0][7] = [(10, w), (20, w), (30, w), (31, 1)]  # P, P again, -P with one wide coefficient, then an unrelated point
    return n, m, mats, ks


def _case_long(pr, g2):
    """(600, 9): columns of 512, 513 and 600 non-zeros in L, +-1 with every seventh entry wide, and an all-narrow long column
    beside them (R: the matrix is wide through its other columns).  g2: the wide entries are one in seven of ONE long column
    (the oracle's G2 multiplications set that limit), everything else +-1."""
    rng = pr.SplitMix64(6009)
    n, m = 600, 9
    ks = [0 if g % 97 == 5 else rng.fr() for g in range(n)]
    ks[300] = ks[100]
    ks[301] = R - ks[100]

    def column(gates, wide=True):
        return [(g, _wide(rng) if wide and i % 7 == 0 else _sign(rng)) for i, g in enumerate(gates)]

    if g2:
        L = {0: column(range(600)), 1: column(range(512), False), 2: column(range(87, 600), False), 3: [(100, 1), (300, 1), (301, 2)]}
        Rm = {0: column(range(513), False), 8: [(599, 1 << 64)]}
        O = {7: column(range(600 - 512, 600), False), 2: [(7, (R + 1) // 2)]}
    else:
        L = {0: column(range(600)), 1: column(range(512)), 2: column(range(87, 600)),
             3: [(100, 1), (300, 1), (301, 2)], 5: column(range(0, 600, 50))}  # (3: a + a - 2a, cancels only in total; 4: in no gate)
        Rm = {0: column(range(513)), 1: column(range(600), False), 6: column(range(3, 600, 40)), 8: [(599, R - 1)]}
        O = {7: column(range(600 - 512, 600)), 2: column(range(1, 600, 60))}
    assert [len(L[c]) for c in (0, 1, 2)] == [600, 512, 513] and len(Rm[0]) == 513 and len(O[7]) == 512
    return n, m, [L, Rm, O], ks


def _reference(G, pts, entries):
    """sum of coefficient * point over the entries of one column: the oracle's Mul and Add, term by term"""
    acc = None
    for g, c in entries:
        p = pts[g]
        if p is None or c == 0:
            continue
        t = p if c == 1 else G.mul(c % R, p)
        acc = t if acc is None else (acc if t is None else G.add(acc, t))
    return acc


CASES = {"1x1": _case_1x1, "toy": _case_toy, "65x40": _case_mid, "600x9": lambda pr: _case_long(pr, False),
         "600x9-one-wide-column": lambda pr: _case_long(pr, True)}


@pytest.mark.parametrize("case,group", [("1x1", 1), ("toy", 1), ("65x40", 1), ("600x9", 1), ("1x1", 2), ("toy", 2),
                                        ("600x9-one-wide-column", 2)])
def test_wide_column_sums_match_the_oracle(ps_api, ctx, co, pr, case, group):
    n, m, mats, ks = CASES[case](pr)
    G = co.G1 if group == 1 else co.G2
    rows = [wc.rows_of(n, cols) for cols in mats]
    q = ps_api.QAP.from_csr(ctx, m, 1, *[wc.csr_fr(r) for r in rows])
    counts = tuple(wc.count_wide(r) for r in rows)
    assert q.wide_entries() == counts and all(counts[k] for k in range(3) if mats[k])
    P = ps_api.Points.from_scalars(ctx, group, ps_api.Poly.upload(ctx, ks))
    pts = G.unpack(P.download())
    assert [p is None for p in pts] == [k == 0 for k in ks]
    for which, cols in enumerate(mats):
        got = q.column_sums(which, P)
        assert len(got) == m and got.group == group
        raw = got.download()
        for i in range(m):
            want = G.to_b(_reference(G, pts, cols.get(i, [])))
            assert raw[i * G.nb : (i + 1) * G.nb] == want, (case, group, which, i, len(cols.get(i, [])))
    q.free()


def test_special_columns_of_the_wide_toy_case_are_what_they_are_meant_to_be(ps_api, ctx, co, pr):
    n, m, mats, ks = _case_toy(pr)
    q = ps_api.QAP.from_csr(ctx, m, 1, *[wc.csr_fr(wc.rows_of(n, cols)) for cols in mats])
    for group, G in ((1, co.G1), (2, co.G2)):
        P = ps_api.Points.from_scalars(ctx, group, ps_api.Poly.upload(ctx, ks))
        ident = G.to_b(None)
        raw = q.column_sums(0, P).download()
        at = lambda i: raw[i * G.nb : (i + 1) * G.nb]
        assert at(1) == ident and at(3) == ident and at(4) == ident
        assert at(0) == G.to_b(G.mul(2 * ((1 << 64) + 1) * ks[0] % R)) and at(2) == G.to_b(G.mul(ks[0]))
        raw = q.column_sums(1, P).download()
        assert raw[5 * G.nb : 6 * G.nb] == ident and raw[1 * G.nb : 2 * G.nb] == ident
    q.free()


# ---------------------------------------------------------------------------------------------------------------------
# setups and provers on the MiMC circuit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [10, 34])
def test_groth16_on_the_mimc_circuit_equals_the_oracle(ps_api, ctx, co, pr, rounds):
    from oracle import restate as rs

    c, sol, cs = wc.mimc_circuit(rounds)
    n = c.nbGates
    assert n == 2 * rounds and c.nbVars == n + 2
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)  # (the list door: it must choose ps_qap_create_fr)
    nw = sum(1 for v in cs if wc.is_wide(v))
    assert q.wide_entries() == (nw, 2 * nw, 0) and nw >= 6
    rng = pr.SplitMix64(0x6731360000 + rounds)
    tox = [rng.fr() for _ in range(5)]
    want = rs.groth16_setup(c, *tox)
    tr, vk = ps_api.NewGroth16TrustedSetup(q, *tox)
    assert (tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2, vk["Gamma"]) == (
        want.Alpha, want.Beta, want.Delta, want.Beta2, want.Delta2, want.Gamma)
    assert tr.Xi.download() == want.Xi
    assert tr.Xi2.download() == want.Xi2
    assert tr.XiT.download() == want.XiT
    assert tr.NioLP.download() == want.NioLP
    assert vk["IoLP"].download() == want.IoLP
    r, s = rng.fr(), rng.fr()
    dsol = ps_api.Poly.upload(ctx, sol)
    assert q.IsValid(dsol)
    ref = rs.groth16_prove(want, c, sol, r, s, fast=n > 16)
    diff = c.nbVars - c.nbIO
    io = ps_api.Poly.upload(ctx, sol[:diff])
    for key in (tr.lagrange_only(), tr.monomial_only()):
        p = ps_api.Groth16Prove(key, q, dsol, r, s)
        assert (p.A, p.B, p.C) == (ref.A, ref.B, ref.C)
        assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], p, io)
    q.free()


@pytest.mark.parametrize("rounds", [10, 34])
def test_phgr13_on_the_mimc_circuit_equals_the_oracle(ps_api, ctx, co, pr, rounds):
    from oracle import restate as rs

    c, sol, _ = wc.mimc_circuit(rounds)
    n = c.nbGates
    diff = c.nbVars - c.nbIO
    q = _qap_fr(ps_api, ctx, c)
    rng = pr.SplitMix64(0x7068670000 + rounds)
    tox = [rng.fr() for _ in range(8)]
    want = rs.phgr13_setup(c, *tox)
    ek, vk = ps_api.NewPHGR13TrustedSetup(q, *tox)
    for f in ps_api.PHGR13EvalKey.FIELDS:
        assert getattr(ek, f).download() == getattr(want.EK, f), f
    G1, G2 = co.G1, co.G2
    groups = {"av": G2, "aw": G1, "ay": G2, "gamma": G2, "bgamma": G1, "bgamma2": G2, "yts": G2}
    for f, grp in groups.items():
        assert getattr(vk, f) == grp.to_b(getattr(want.VK, f)), f
    assert vk.vs.download() == G1.pack(want.VK.vs)
    assert vk.ws.download() == G2.pack(want.VK.ws)
    assert vk.ys.download() == G1.pack(want.VK.ys)
    sol_dev = ps_api.Poly.upload(ctx, sol)
    ref = rs.phgr13_prove(want.EK, c, sol, fast=n > 16)
    proof = ps_api.PHGR13Prove(ek, q, sol_dev)
    mono = ps_api.PHGR13Prove(ek.monomial_only(), q, sol_dev)
    for f in ps_api.PHGR13Proof.FIELDS:
        assert getattr(proof, f) == getattr(ref, f), f
        assert getattr(mono, f) == getattr(ref, f), f
    io = ps_api.Poly.upload(ctx, sol[:diff])
    args = (vk.vs.slice(0, diff), vk.ws.slice(0, diff), vk.ys.slice(0, diff))
    assert ps_api.PHGR13Verify(ctx, vk.fixed_points(), *args, proof, io)
    q.free()


@pytest.mark.parametrize("rounds", [10, 34])
def test_one_wide_constant_changed_in_the_qap_is_an_apocalypse(ps_api, ctx, rounds):
    c, sol, cs = wc.mimc_circuit(rounds)
    i = 5  # (r - 1) / 2
    assert wc.is_wide(cs[i]) and wc.is_wide(cs[i] + (1 << 64))
    bad, _, _ = wc.mimc_circuit(rounds, flip=(i, 1 << 64))  # the witness is still that of the unchanged circuit
    q = ps_api.QAP(ctx, bad.nbVars, bad.nbIO, bad.left, bad.right, bad.out)
    dsol = ps_api.Poly.upload(ctx, sol)
    assert not q.IsValid(dsol)
    with pytest.raises(ps_api.Apocalypse):
        q.Quotient(dsol)
    q.free()


# ---------------------------------------------------------------------------------------------------------------------
# the route without toxic waste
# ---------------------------------------------------------------------------------------------------------------------
def _toxic(pr):
    rng = pr.SplitMix64(20161016)
    return {k: rng.fr() for k in ("alpha", "beta", "x", "d", "g")}


def _srs(api, ctx, co, n, tw):
    x = tw["x"]
    pw = [pow(x, i, R) for i in range(2 * n - 1)]
    commit = lambda g, v: api.Points.from_scalars(ctx, g, api.Poly.upload(ctx, v))
    return api.Groth16SRS(commit(api.G1, pw), commit(api.G2, pw[:n]), commit(api.G1, [tw["alpha"] * p % R for p in pw[:n]]),
                          commit(api.G1, [tw["beta"] * p % R for p in pw[:n]]), co.G2.to_b(co.G2.mul(tw["beta"])))


def _key_bytes(pair):
    tr, vk = pair
    out = {f: getattr(tr, f) for f in FIXED}
    out["Gamma"] = vk["Gamma"]
    out["IoLP"] = vk["IoLP"].download()
    for f in ARRAYS:
        out[f] = getattr(tr, f).download()
    return out


def _assert_same_key(got, want, what):
    gb, wb = _key_bytes(got), _key_bytes(want)
    for f in wb:
        assert len(gb[f]) == len(wb[f]), (what, f, len(gb[f]), len(wb[f]))
        assert gb[f] == wb[f], (what, f)


@pytest.mark.parametrize("rounds", [10, 34, 560])
def test_setup_from_srs_fold_proof_and_check_on_the_mimc_circuit(ps_api, ctx, co, pr, rounds):
    from oracle import restate as rs

    c, sol, cs = wc.mimc_circuit(rounds)
    n, tw = c.nbGates, _toxic(pr)
    col0 = [sum(1 for row in m for col, v in row if col == 0 and wc.is_wide(v)) for m in (c.left, c.right)]
    if rounds == 560:  # the long wide row: one workgroup sums the `const` column of L and of R
        assert n == 1120 and col0[0] > 512 and col0[1] > 1024
    q = _qap_fr(ps_api, ctx, c)
    assert q.wide_entries() == (col0[0], col0[1], 0)
    srs = _srs(ps_api, ctx, co, n, tw)
    K0 = ps_api.NewGroth16SetupFromSRS(q, srs)
    _assert_same_key(K0, ps_api.NewGroth16TrustedSetup(q, tw["alpha"], tw["beta"], 1, tw["x"], 1), "delta = gamma = 1")
    K1 = ps_api.Groth16Contribute(ctx, *K0, tw["d"], tw["g"])
    _assert_same_key(K1, ps_api.NewGroth16TrustedSetup(q, tw["alpha"], tw["beta"], tw["d"], tw["x"], tw["g"]), "one fold")
    tr, vk = K1
    diff = c.nbVars - c.nbIO
    dsol, io = ps_api.Poly.upload(ctx, sol), ps_api.Poly.upload(ctx, sol[:diff])
    r, s = 0x1F2E3D4C5B6A7988, 0x0123456789ABCDEF0FEDCBA987654321
    proof = ps_api.Groth16Prove(tr, q, dsol, r, s)
    assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], proof, io)
    if n <= 68:
        ref = rs.groth16_setup(c, tw["alpha"], tw["beta"], tw["d"], tw["x"], tw["g"])
        want = rs.groth16_prove(ref, c, sol, r, s, fast=n > 16)
        assert (proof.A, proof.B, proof.C) == (want.A, want.B, want.C)
    rng = pr.SplitMix64(n)
    rhos = [(rng.next() << 64 | rng.next()) or 1 for _ in range(max(c.nbVars, n))]
    assert ps_api.Groth16CheckFromSRS(ctx, q, srs, K1, rhos)
    # a second circuit that differs in ONE wide coefficient by 2^64 -- invisible to a 64-bit truncation -- has another key
    i = 5  # (r - 1) / 2
    assert wc.is_wide(cs[i]) and wc.is_wide(cs[i] + (1 << 64))
    other, _, _ = wc.mimc_circuit(rounds, flip=(i, 1 << 64))
    q2 = _qap_fr(ps_api, ctx, other)
    assert q2.wide_entries() == q.wide_entries()
    K2 = ps_api.Groth16Contribute(ctx, *ps_api.NewGroth16SetupFromSRS(q2, srs), tw["d"], tw["g"])
    assert ps_api.Groth16CheckFromSRS(ctx, q2, srs, K2, rhos)
    assert not ps_api.Groth16CheckFromSRS(ctx, q, srs, K2, rhos)
    assert K2[0].NioLP.download() != tr.NioLP.download() or K2[1]["IoLP"].download() != vk["IoLP"].download()
    q.free()
    q2.free()


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def _one_gate(val_bytes, col=0):
    ptr = np.array([0, 1], dtype=np.uint32)
    return ptr, np.array([col], dtype=np.uint32), val_bytes


def test_errors(ps_api, ctx):
    from playsnark_amd import _lib

    one = (1).to_bytes(32, "big")
    for bad in (R, (1 << 256) - 1):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.QAP.from_csr(ctx, 2, 1, _one_gate(one), _one_gate(bad.to_bytes(32, "big")), _one_gate(one))
        assert e.value.code == _lib.PS_ERR_ENCODING
    q = ps_api.QAP.from_csr(ctx, 2, 1, _one_gate(one), _one_gate((R - 1).to_bytes(32, "big")), _one_gate(bytes(32)))  # r - 1 and an explicit zero
    assert q.wide_entries() == (0, 0, 0)
    q.free()
    texts = []
    for val in (one, np.array([1], dtype=np.int64)):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.QAP.from_csr(ctx, 2, 1, _one_gate(val), _one_gate(val, col=2), _one_gate(val))
        assert e.value.code == _lib.PS_ERR_ARG
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "column index out of range" in texts[0]
    with pytest.raises(TypeError):
        ps_api.QAP(ctx, 2, 1, [[(0, 1.0)]], [[(0, 1)]], [[(0, 1)]])
    with pytest.raises(TypeError):
        ps_api.QAP.from_dense(ctx, 2, 1, [[0.5, 0]], [[1, 0]], [[1, 0]])
    with pytest.raises(TypeError):
        f = np.array([1.0])
        ps_api.QAP.from_csr(ctx, 2, 1, _one_gate(f), _one_gate(f), _one_gate(f))
    # a value that is no int64 no longer wraps: -1 written as r - 1 is the circuit with -1
    qa = ps_api.QAP(ctx, 2, 1, [[(0, R - 1)]], [[(1, 1 << 64)]], [[(0, 5)]])
    assert qa.wide_entries() == (0, 1, 0)
    qa.free()
