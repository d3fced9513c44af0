"""ps_groth16_verify_batch: N Groth16 proofs under one key checked by a random linear combination -- N Miller loops on the
device, one sum over IoLP, one over the C_i, one final exponentiation.  Proofs are made by ps_groth16_prove for one key of
a 21-gate circuit, two different public inputs among them, fresh (r, s) per proof.  Every compared quantity is a
verdict, an error code or an index.

The independent reference is oracle.pairing.groth16_verify, per proof: its verdict on EVERY proof of every batch -- valid
or tampered -- decides which indices locate=True must return.  The oracle's pairing is pure Python (3.4 s per proof), so its
verdicts on the proofs these tests meet are recorded in tests/golden/verify_batch_verdicts.json by
tests/golden/gen_verify_batch_verdicts.py (same seeds: tests/verify_batch_cases.py; the oracle's prover gives the bytes the
device gives).  A proof whose digest is not recorded is put to the oracle on the spot."""
import threading

import pytest

pytestmark = pytest.mark.gpu

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_batch_cases as vc  # noqa: E402

SEED = vc.SEED


@pytest.fixture(scope="module")
def mat(ps_api, ctx, co, pr):
    """One key, two witnesses (x = 3 and x = 4), 300 proofs with fresh (r, s)."""
    from oracle import restate as rs

    c, sols, tr, draws, diff = vc.material(pr, rs)
    up = lambda g, b: ps_api.Points.upload(ctx, g, b)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    pk = ps_api.Groth16Setup(tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2, up(ps_api.G1, tr.Xi), up(ps_api.G2, tr.Xi2),
                             up(ps_api.G1, tr.NioLP), up(ps_api.G1, tr.XiT))
    dsols = [ps_api.Poly.upload(ctx, s) for s in sols]
    proofs = [ps_api.Groth16Prove(pk, q, dsols[w], r, s) for w, r, s in draws]
    ios = [sols[w][:diff] for w, _, _ in draws]
    iolp = up(ps_api.G1, tr.IoLP)
    trp = rs.Bag(Alpha=co.G1.from_b(tr.Alpha), Beta2=co.G2.from_b(tr.Beta2), IoLP=co.G1.unpack(tr.IoLP), Gamma=co.G2.from_b(tr.Gamma),
                 Delta2=co.G2.from_b(tr.Delta2))
    return rs.Bag(tr=tr, trp=trp, iolp=iolp, proofs=proofs, ios=ios, diff=diff, verdicts=vc.recorded_verdicts(), live=[0])


def _io(ps_api, ctx, ios):
    return ps_api.Poly.upload(ctx, [v for row in ios for v in row])


def _batch(ps_api, ctx, mat, proofs, ios, rhos, iolp=None, **kw):
    tr = mat.tr
    return ps_api.Groth16VerifyBatch(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, iolp or mat.iolp, proofs, _io(ps_api, ctx, ios), rhos, **kw)


def _single(ps_api, ctx, mat, p, io):
    tr = mat.tr
    return ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, mat.iolp, p, ps_api.Poly.upload(ctx, io))


def _oracle(co, mat, p, io):
    """oracle.pairing.groth16_verify on one proof: the recorded verdict, or the oracle itself for a proof not recorded"""
    from oracle import pairing as pg

    key = vc.digest((p.A, p.B, p.C), io)
    if key not in mat.verdicts:
        mat.live[0] += 1
        mat.verdicts[key] = bool(pg.groth16_verify(mat.trp, co.G1.from_b(p.A), co.G2.from_b(p.B), co.G1.from_b(p.C), io))
    return mat.verdicts[key]


def _rhos(pr, rng, n, bits):
    return [(rng.fr() if bits == 255 else rng.fr() >> 127) or 1 for _ in range(n)]


def _with(ps_api, p, **kw):
    return ps_api.Groth16Proof(p.R, p.S, kw.get("A", p.A), kw.get("B", p.B), kw.get("C", p.C))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_valid_batches_are_accepted_for_any_weights(ps_api, ctx, pr, mat, n):
    rng = pr.SplitMix64(SEED + n)
    for bits in (255, 128):
        rhos = _rhos(pr, rng, n, bits)
        assert all(0 < v < pr.R for v in rhos) and (bits == 255 or max(rhos) < 1 << 128)
        assert _batch(ps_api, ctx, mat, mat.proofs[:n], mat.ios[:n], rhos) is True
        assert _batch(ps_api, ctx, mat, mat.proofs[:n], mat.ios[:n], rhos, locate=True) == []
    assert len({tuple(io) for io in mat.ios[: max(n, 2)]}) == 2  # two different public inputs among them


def test_empty_batch(ps_api, ctx, mat):
    assert _batch(ps_api, ctx, mat, [], [], []) is True


def test_one_proof_with_weight_one_is_the_single_verifier(ps_api, ctx, co, pr, mat):
    p, io = mat.proofs[0], mat.ios[0]
    bad_c = _with(ps_api, p, C=co.G1.to_b(pr.G1.add(co.G1.from_b(p.C), pr.G1.gen)))
    bad_io = [io[0], (io[1] + 1) % pr.R] + io[2:]
    for pf, pub in ((p, io), (bad_c, io), (p, bad_io)):
        want = _single(ps_api, ctx, mat, pf, pub)
        assert _batch(ps_api, ctx, mat, [pf], [pub], [1]) is want
    assert _single(ps_api, ctx, mat, p, io) is True and _single(ps_api, ctx, mat, bad_c, io) is False
    assert _single(ps_api, ctx, mat, p, bad_io) is False


def test_recorded_verdicts_are_the_oracles(co, pr, mat):
    """The fixture file is not taken on trust: the oracle itself is asked about one valid and one tampered proof, and the
    device's proofs are the ones the verdicts were recorded for."""
    from oracle import pairing as pg

    assert all(vc.digest((p.A, p.B, p.C), io) in mat.verdicts for p, io in zip(mat.proofs, mat.ios))
    p, io = mat.proofs[1], mat.ios[1]
    (a, b, c), tio = vc.apply_tamper((p.A, p.B, p.C), io, "C", vc.tampers(pr, co, 2, mat.diff)[6][2])
    for abc, pub in (((p.A, p.B, p.C), io), ((a, b, c), tio)):
        live = bool(pg.groth16_verify(mat.trp, co.G1.from_b(abc[0]), co.G2.from_b(abc[1]), co.G1.from_b(abc[2]), pub))
        assert mat.verdicts[vc.digest(abc, pub)] is live


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_one_bad_element_is_rejected_and_located(ps_api, ctx, co, pr, mat, n):
    """Exactly one of A, B, C or one public input replaced, at the first, the middle and the last proof: rejected, and
    locate=True names exactly the proofs the oracle rejects -- the oracle's verdict on every proof of the batch."""
    rng = pr.SplitMix64(SEED + 2000 + n)
    cases = vc.tampers(pr, co, n, mat.diff)
    assert {pos for pos, _, _ in cases} == {0, n // 2, n - 1} and len(cases) == 4 * len({0, n // 2, n - 1})
    for pos, what, value in cases:
        proofs, ios = list(mat.proofs[:n]), [list(v) for v in mat.ios[:n]]
        p = proofs[pos]
        (a, b, c), ios[pos] = vc.apply_tamper((p.A, p.B, p.C), ios[pos], what, value)
        proofs[pos] = _with(ps_api, p, A=a, B=b, C=c)
        want = [i for i in range(n) if not _oracle(co, mat, proofs[i], ios[i])]
        assert want == [pos], (pos, what, want)
        rhos = _rhos(pr, rng, n, 128)
        assert _batch(ps_api, ctx, mat, proofs, ios, rhos) is False, (pos, what)
        assert _batch(ps_api, ctx, mat, proofs, ios, rhos, locate=True) == want, (pos, what)
    assert mat.live[0] == 0, "the recorded verdicts do not cover the proofs of this test"


def test_the_equation_is_the_linear_combination(ps_api, ctx, co, pr, mat):
    """C1' = C1 + rho2 D, C2' = C2 - rho1 D: both proofs are invalid, and the errors cancel in rho1 C1' + rho2 C2' -- under
    THAT rho the batch is accepted, under any other it is rejected.  This is why rho is drawn after the proofs are fixed."""
    rng = pr.SplitMix64(SEED + 77)
    r1, r2 = rng.fr() >> 127 or 1, rng.fr() >> 127 or 1
    D = pr.G1.mul(rng.fr())
    p1, p2 = mat.proofs[0], mat.proofs[1]
    c1 = pr.G1.add(co.G1.from_b(p1.C), pr.G1.mul_pt(r2, D))
    c2 = pr.G1.add(co.G1.from_b(p2.C), pr.G1.mul_pt(pr.R - r1, D))
    forged = [_with(ps_api, p1, C=co.G1.to_b(c1)), _with(ps_api, p2, C=co.G1.to_b(c2))]
    ios = mat.ios[:2]
    assert _single(ps_api, ctx, mat, forged[0], ios[0]) is False and _single(ps_api, ctx, mat, forged[1], ios[1]) is False
    assert _batch(ps_api, ctx, mat, forged, ios, [r1, r2]) is True
    assert _batch(ps_api, ctx, mat, forged, ios, [r1, r2 + 1]) is False
    assert _batch(ps_api, ctx, mat, forged, ios, [rng.fr(), rng.fr()]) is False
    assert _batch(ps_api, ctx, mat, forged, ios, [rng.fr(), rng.fr()], locate=True) == [0, 1]


def test_errors(ps_api, ctx, co, pr, mat, off_subgroup):
    from playsnark_amd import _lib

    n = 5
    proofs, ios = mat.proofs[:n], mat.ios[:n]
    rhos = [3, 5, 7, 11, 13]

    def code(fn):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            fn()
        return e.value.code

    for what, pt in (("A", co.G1.to_b(off_subgroup[0])), ("B", co.G2.to_b(off_subgroup[1])), ("C", co.G1.to_b(off_subgroup[0]))):
        bad = list(proofs)
        bad[2] = _with(ps_api, bad[2], **{what: pt})
        assert code(lambda: _batch(ps_api, ctx, mat, bad, ios, rhos)) == _lib.PS_ERR_ENCODING, what
    junk = list(proofs)
    junk[3] = _with(ps_api, junk[3], A=b"\x01" + junk[3].A[1:])  # not on the curve
    with pytest.raises(ps_api.PlaysnarkError) as e:
        _batch(ps_api, ctx, mat, junk, ios, rhos)
    assert e.value.code == _lib.PS_ERR_ENCODING and "proof 3" in str(e.value)
    assert code(lambda: _batch(ps_api, ctx, mat, proofs, ios, [3, 0, 7, 11, 13])) == _lib.PS_ERR_ARG
    assert code(lambda: _batch(ps_api, ctx, mat, proofs, ios, [3, pr.R, 7, 11, 13])) == _lib.PS_ERR_ENCODING
    assert code(lambda: _batch(ps_api, ctx, mat, proofs, ios, [3, 2**256 - 1, 7, 11, 13])) == _lib.PS_ERR_ENCODING
    with pytest.raises(ps_api.LengthMismatch):
        _batch(ps_api, ctx, mat, proofs, ios[:4] + [ios[4][:-1]], rhos)
    # a pending sum on the context
    pts = ps_api.Points.upload(ctx, ps_api.G1, co.G1.gen_points(3, 5, 8))
    ps_api.msm_launch(ctx, pts, ps_api.Poly.upload(ctx, list(range(1, len(pts) + 1))))
    try:
        assert code(lambda: _batch(ps_api, ctx, mat, proofs, ios, rhos)) == _lib.PS_ERR_ARG
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    assert _batch(ps_api, ctx, mat, proofs, ios, rhos) is True


def test_two_threads_two_contexts_one_key(ps_api, co, pr, mat):
    """The uploaded IoLP array is shared read-only by two contexts on two host threads; same verdicts."""
    n = 16
    bad = list(mat.proofs[:n])
    bad[5] = _with(ps_api, bad[5], C=co.G1.to_b(pr.G1.mul(12345)))
    rhos = _rhos(pr, pr.SplitMix64(SEED + 5), n, 128)
    errors, results, barrier = [], {}, threading.Barrier(2)

    def worker(tid):
        try:
            cx = ps_api.Context(0)
            barrier.wait()
            out = []
            for rep in range(3):
                out.append(_batch(ps_api, cx, mat, mat.proofs[:n], mat.ios[:n], rhos))
                out.append(_batch(ps_api, cx, mat, bad, mat.ios[:n], rhos))
            results[tid] = out
            cx.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((tid, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert results[0] == results[1] == [True, False] * 3


def test_three_passes_of_column_sums(ps_api, ctx, pr, mat):
    """N = 5 000: weighted_columns (verify_batch.inc) sums 5 000 rows in 79 chunks, those in 2, those in 1 -- three passes,
    where 300 proofs take two.  The 300 proofs repeated, fresh non-zero weights."""
    n = 5000
    rng = pr.SplitMix64(SEED + 5000)
    proofs = [mat.proofs[i % vc.NPROOFS] for i in range(n)]
    ios = [list(mat.ios[i % vc.NPROOFS]) for i in range(n)]
    per = lambda r: max(64, -(-r // max(1, min(4096, -(-65536 // mat.diff)))))
    chunks = [n]
    while chunks[-1] > 1:
        chunks.append(-(-chunks[-1] // per(chunks[-1])))
    assert chunks == [5000, 79, 2, 1]
    rhos = _rhos(pr, rng, n, 128)
    assert all(0 < v < pr.R for v in rhos)
    assert _batch(ps_api, ctx, mat, proofs, ios, rhos) is True
    ios[n - 1][1] = (ios[n - 1][1] + 1) % pr.R
    assert _batch(ps_api, ctx, mat, proofs, ios, rhos) is False
    assert _batch(ps_api, ctx, mat, proofs, ios, rhos, locate=True) == [n - 1]


def test_more_than_256_public_inputs(ps_api, ctx, co, pr):
    """A 300-gate circuit has 299 public inputs in the reference's convention (nbVars - nbIO): k_fr_weighted_columns runs
    with two grid columns (blockIdx.x > 0).  130 proofs made by Groth16Prove; proof 0 also goes through Groth16Verify and,
    live, through oracle.pairing.groth16_verify."""
    from oracle import pairing as pg
    from oracle import restate as rs

    n, gates = 130, 300
    rng = pr.SplitMix64(SEED + 300)
    circuits = [rs.synthetic_circuit(gates, x0) for x0 in (3, 4)]
    c, sols = circuits[0][0], [s for _, s in circuits]
    diff = c.nbVars - c.nbIO
    assert diff > 256
    tr = rs.groth16_setup(c, *[rng.fr() for _ in range(5)])
    up = lambda g, b: ps_api.Points.upload(ctx, g, b)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    pk = ps_api.Groth16Setup(tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2, up(ps_api.G1, tr.Xi), up(ps_api.G2, tr.Xi2),
                             up(ps_api.G1, tr.NioLP), up(ps_api.G1, tr.XiT))
    dsols = [ps_api.Poly.upload(ctx, s) for s in sols]
    proofs = [ps_api.Groth16Prove(pk, q, dsols[i % 2], rng.fr(), rng.fr()) for i in range(n)]
    ios = [sols[i % 2][:diff] for i in range(n)]
    iolp = up(ps_api.G1, tr.IoLP)
    assert len(iolp) == diff
    rhos = _rhos(pr, rng, n, 128)
    batch = lambda pub, **kw: ps_api.Groth16VerifyBatch(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, iolp, proofs, _io(ps_api, ctx, pub), rhos, **kw)
    assert batch(ios) is True
    assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, iolp, proofs[0], ps_api.Poly.upload(ctx, ios[0])) is True
    trp = rs.Bag(Alpha=co.G1.from_b(tr.Alpha), Beta2=co.G2.from_b(tr.Beta2), IoLP=co.G1.unpack(tr.IoLP), Gamma=co.G2.from_b(tr.Gamma),
                 Delta2=co.G2.from_b(tr.Delta2))
    p = proofs[0]
    assert pg.groth16_verify(trp, co.G1.from_b(p.A), co.G2.from_b(p.B), co.G1.from_b(p.C), ios[0]) is True
    # a public input in the second grid column (j >= 256) of the last proof
    bad = [list(v) for v in ios]
    bad[n - 1][diff - 1] = (bad[n - 1][diff - 1] + 1) % pr.R
    assert batch(bad) is False
