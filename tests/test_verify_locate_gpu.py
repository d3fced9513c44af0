"""ps_groth16_verify_batch_locate: WHICH proofs of a batch are invalid, by bisection over partial results kept on the device.

Material and references are those of tests/test_verify_batch_gpu.py: the 300 proofs of one key (tests/verify_batch_cases.py)
and the oracle's verdicts recorded in tests/golden/verify_batch_verdicts.json -- 300 valid proofs and the 48 tampered
variants of proofs 0, 1, 3, 6, 32, 63, 150 and 299.  A digest depends on a proof and its inputs only, so a test puts any of
the 48 at any position of a batch.  Every proof met is found in the recorded verdicts: the pure-Python oracle is never
called here.  The on-device cross-check is Groth16VerifyBatch(..., locate=True), which verifies proof by proof.
Every compared quantity is a verdict, an index, a count or an error code; the bound on the checks is the issue's:
checks == 1 for an accepted batch, checks <= 1 + 2 b ceil(log2 N) for b invalid proofs among N."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import verify_batch_cases as vc  # noqa: E402
from test_verify_batch_gpu import _io, _rhos, _single, _with, mat  # noqa: E402,F401

SEED = vc.SEED + 0x6C6F63


def _ceil_log2(n):
    return (n - 1).bit_length()


def _locate(ps_api, ctx, mat, proofs, ios, rhos):
    tr = mat.tr
    return ps_api.Groth16VerifyBatchLocate(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, mat.iolp, proofs, _io(ps_api, ctx, ios), rhos)


def _loop(ps_api, ctx, mat, proofs, ios, rhos):
    tr = mat.tr
    return ps_api.Groth16VerifyBatch(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, mat.iolp, proofs, _io(ps_api, ctx, ios), rhos, locate=True)


def _recorded(mat, p, io):
    key = vc.digest((p.A, p.B, p.C), io)
    assert key in mat.verdicts, "a proof of this test has no recorded verdict"
    return mat.verdicts[key]


@pytest.fixture(scope="module")
def tampered(ps_api, co, pr, mat):
    """The 48 tampered (proof, io) of the recorded verdicts, in the order of vc.SIZES and vc.tampers"""
    out = []
    for n in vc.SIZES:
        for pos, what, value in vc.tampers(pr, co, n, mat.diff):
            p = mat.proofs[pos]
            (a, b, c), io = vc.apply_tamper((p.A, p.B, p.C), mat.ios[pos], what, value)
            out.append((_with(ps_api, p, A=a, B=b, C=c), io))
    assert len(out) == 48 and not any(_recorded(mat, p, io) for p, io in out)
    assert len({vc.digest((p.A, p.B, p.C), io) for p, io in out}) == 48
    return out


def _check(ps_api, ctx, mat, proofs, ios, rhos, want_bad):
    """One batch: the verdict vector is the recorded one, the bad list is the per-proof loop's, the checks are bounded"""
    n = len(proofs)
    recorded = [_recorded(mat, p, io) for p, io in zip(proofs, ios)]
    want = [i for i in range(n) if not recorded[i]]
    assert want == sorted(want_bad)
    bad, info = _locate(ps_api, ctx, mat, proofs, ios, rhos)
    assert [i not in bad for i in range(n)] == recorded
    assert bad == want == _loop(ps_api, ctx, mat, proofs, ios, rhos)
    b = len(want)
    print(f"N = {n}, b = {b}: checks = {info['checks']}, levels = {info['levels']}, bound = {1 + 2 * b * _ceil_log2(n)}")
    assert info["invalid"] == b
    assert info["checks"] == 1 if b == 0 else 1 <= info["checks"] <= 1 + 2 * b * _ceil_log2(n)
    assert info["levels"] == (_ceil_log2(n) if b else 0)
    return info


@pytest.mark.parametrize("n", vc.SIZES)
def test_accepted_batches_cost_one_check(ps_api, ctx, pr, mat, n):
    rng = pr.SplitMix64(SEED + n)
    for bits in (255, 128):
        rhos = _rhos(pr, rng, n, bits)
        assert all(0 < v < pr.R for v in rhos) and (bits == 255 or max(rhos) < 1 << 128)
        assert all(_recorded(mat, p, io) for p, io in zip(mat.proofs[:n], mat.ios[:n]))
        bad, info = _locate(ps_api, ctx, mat, mat.proofs[:n], mat.ios[:n], rhos)
        assert bad == [] and info == {"checks": 1, "levels": 0, "invalid": 0}
    assert mat.live[0] == 0


@pytest.mark.parametrize("n,which", [(n, w) for n in vc.SIZES for w in range(len({0, n // 2, n - 1}))])
def test_one_bad_element_is_located(ps_api, ctx, co, pr, mat, n, which):
    """The single-tamper cases of vc.tampers: one of A, B, C or one public input replaced at the first, the middle or the
    last proof"""
    rng = pr.SplitMix64(SEED + 2000 + 8 * n + which)
    cases = vc.tampers(pr, co, n, mat.diff)
    pos = sorted({0, n // 2, n - 1})[which]
    mine = [c for c in cases if c[0] == pos]
    assert len(mine) == 4 and {w for _, w, _ in mine} == {"A", "B", "C", "io"}
    for _, what, value in mine:
        proofs, ios = list(mat.proofs[:n]), [list(v) for v in mat.ios[:n]]
        p = proofs[pos]
        (a, b, c), ios[pos] = vc.apply_tamper((p.A, p.B, p.C), ios[pos], what, value)
        proofs[pos] = _with(ps_api, p, A=a, B=b, C=c)
        info = _check(ps_api, ctx, mat, proofs, ios, _rhos(pr, rng, n, 128), [pos])
        assert info["checks"] <= 1 + 2 * _ceil_log2(n)
    assert mat.live[0] == 0


MANY = {
    "n2-both": (2, [0, 1]),
    "n7-all": (7, list(range(7))),
    "n7-last": (7, [6]),  # a node carried at two levels
    "n64-every-other": (64, list(range(0, 64, 2))),
    "n300-siblings": (300, [0, 1]),
    "n300-ends": (300, [0, 299]),
    "n300-carried-subtree": (300, [296, 299]),  # inside the subtree that is carried from the level of 75 nodes
    "n300-48-spread": (300, list(range(3, 300, 6))[:48]),
}


@pytest.mark.parametrize("case", list(MANY))
def test_several_bad_proofs_are_located(ps_api, ctx, pr, mat, tampered, case):
    n, positions = MANY[case]
    assert len(positions) <= 48 and (case != "n300-48-spread" or len(positions) == 48)
    rng = pr.SplitMix64(SEED + 3000 + sum(ord(ch) for ch in case))
    proofs, ios = list(mat.proofs[:n]), [list(v) for v in mat.ios[:n]]
    shift = rng.next() % 48  # which of the 48 go where
    for k, pos in enumerate(positions):
        proofs[pos], ios[pos] = tampered[(shift + k) % 48]
        ios[pos] = list(ios[pos])
    _check(ps_api, ctx, mat, proofs, ios, _rhos(pr, rng, n, 128), positions)
    assert mat.live[0] == 0


def test_exact_counts_of_one_carried_leaf(ps_api, ctx, pr, mat, tampered):
    """N = 7, proof 6 alone invalid: the counts of a rejected batch as exact numbers, worked out by hand from the levels of
    7, 4, 2, 1 nodes -- the batch check (1); the root's two children, nodes 0 and 1 of 2 (2), node 1 (proofs 4 .. 6) fails;
    its two children, nodes 2 and 3 of 4 (2), node 3 (proof 6) fails; node 3 has the single child 6 of 7, carried, handed
    down without a check (0).  1 + 2 + 2 + 0 = 5 checks over 3 levels."""
    n, rng = 7, pr.SplitMix64(SEED + 5000)
    proofs, ios = list(mat.proofs[:n]), [list(v) for v in mat.ios[:n]]
    bad = tampered[rng.next() % 48]
    proofs[6], ios[6] = bad[0], list(bad[1])
    info = _check(ps_api, ctx, mat, proofs, ios, _rhos(pr, rng, n, 128), [6])
    assert info == {"checks": 5, "levels": 3, "invalid": 1}


def test_tree_shape_of_the_carried_cases():
    """What the case names claim about N = 7 and N = 300"""
    sizes = lambda n: [n] + ([] if n == 1 else sizes((n + 1) // 2))
    assert sizes(7) == [7, 4, 2, 1] and sizes(300) == [300, 150, 75, 38, 19, 10, 5, 3, 2, 1]
    # proof 6 of 7 is the odd one out at level 0 and its node at level 1 (index 3 of 4) is not: carried once below the root's
    # children -- and 7 -> 4 carries it, 4 -> 2 pairs it: the leaf, and the node above it, are single children
    assert 6 // 2 == 3 and 7 % 2 == 1
    # level 2 of 300 has 75 nodes: node 74 (proofs 296 .. 299) is carried into level 3
    assert 75 % 2 == 1 and 74 * 4 == 296 and min(75 * 4, 300) == 300


def test_verdicts_are_relative_to_the_weights(ps_api, ctx, co, pr, mat):
    """The cancelling pair of test_the_equation_is_the_linear_combination: both proofs are invalid (the single verifier), under
    the cancelling rho the batch passes and both are reported valid, under fresh rho both are found"""
    rng = pr.SplitMix64(vc.SEED + 77)
    r1, r2 = rng.fr() >> 127 or 1, rng.fr() >> 127 or 1
    D = pr.G1.mul(rng.fr())
    p1, p2 = mat.proofs[0], mat.proofs[1]
    c1 = pr.G1.add(co.G1.from_b(p1.C), pr.G1.mul_pt(r2, D))
    c2 = pr.G1.add(co.G1.from_b(p2.C), pr.G1.mul_pt(pr.R - r1, D))
    forged = [_with(ps_api, p1, C=co.G1.to_b(c1)), _with(ps_api, p2, C=co.G1.to_b(c2))]
    ios = mat.ios[:2]
    assert _single(ps_api, ctx, mat, forged[0], ios[0]) is False and _single(ps_api, ctx, mat, forged[1], ios[1]) is False
    bad, info = _locate(ps_api, ctx, mat, forged, ios, [r1, r2])
    assert bad == [] and info == {"checks": 1, "levels": 0, "invalid": 0}
    bad, info = _locate(ps_api, ctx, mat, forged, ios, [rng.fr(), rng.fr()])
    assert bad == [0, 1] and info == {"checks": 3, "levels": 1, "invalid": 2}


def test_more_than_256_public_inputs(ps_api, ctx, co, pr):
    """Wide rows of the scalar tree: 299 public inputs, three proofs, one bad public input in the last column of the last
    proof.  The reference is the single verifier."""
    from oracle import restate as rs

    n, gates = 3, 300
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
    ios = [list(sols[i % 2][:diff]) for i in range(n)]
    iolp = up(ps_api.G1, tr.IoLP)
    rhos = _rhos(pr, rng, n, 128)
    locate = lambda pub: ps_api.Groth16VerifyBatchLocate(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, iolp, proofs, _io(ps_api, ctx, pub), rhos)
    single = lambda i, pub: ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, iolp, proofs[i], ps_api.Poly.upload(ctx, pub[i]))
    bad, info = locate(ios)
    assert bad == [] and info["checks"] == 1 and all(single(i, ios) for i in range(n))
    wrong = [list(v) for v in ios]
    wrong[n - 1][diff - 1] = (wrong[n - 1][diff - 1] + 1) % pr.R
    assert [single(i, wrong) for i in range(n)] == [True, True, False]
    bad, info = locate(wrong)
    assert bad == [2] and info["invalid"] == 1 and info["checks"] <= 1 + 2 * _ceil_log2(n)


def test_errors_are_those_of_the_plain_batch_call(ps_api, ctx, co, pr, mat, off_subgroup):
    """Code for code on the same inputs"""
    from playsnark_amd import _lib

    n = 5
    proofs, ios = mat.proofs[:n], mat.ios[:n]
    rhos = [3, 5, 7, 11, 13]
    tr = mat.tr
    plain = lambda pf, pub, w: ps_api.Groth16VerifyBatch(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, mat.iolp, pf, _io(ps_api, ctx, pub), w)

    def outcome(fn):
        try:
            fn()
        except ps_api.PlaysnarkError as e:
            return ("code", e.code)
        except ps_api.LengthMismatch:
            return ("length",)
        return ("ok",)

    def both(pf, pub, w, want):
        a, b = outcome(lambda: plain(pf, pub, w)), outcome(lambda: _locate(ps_api, ctx, mat, pf, pub, w))
        assert a == b == want, (a, b, want)

    both(proofs, ios, [3, 0, 7, 11, 13], ("code", _lib.PS_ERR_ARG))
    both(proofs, ios, [3, pr.R, 7, 11, 13], ("code", _lib.PS_ERR_ENCODING))
    both(proofs, ios, [3, 2**256 - 1, 7, 11, 13], ("code", _lib.PS_ERR_ENCODING))
    both(proofs, ios[:4] + [ios[4][:-1]], rhos, ("length",))
    junk = list(proofs)
    junk[3] = _with(ps_api, junk[3], A=b"\x01" + junk[3].A[1:])  # not on the curve
    both(junk, ios, rhos, ("code", _lib.PS_ERR_ENCODING))
    with pytest.raises(ps_api.PlaysnarkError) as e:
        _locate(ps_api, ctx, mat, junk, ios, rhos)
    assert "proof 3" in str(e.value) and "ps_groth16_verify_batch_locate" in str(e.value)
    for what, pt in (("A", co.G1.to_b(off_subgroup[0])), ("B", co.G2.to_b(off_subgroup[1])), ("C", co.G1.to_b(off_subgroup[0]))):
        off = list(proofs)
        off[2] = _with(ps_api, off[2], **{what: pt})
        both(off, ios, rhos, ("code", _lib.PS_ERR_ENCODING))
    pts = ps_api.Points.upload(ctx, ps_api.G1, co.G1.gen_points(3, 5, 8))
    ps_api.msm_launch(ctx, pts, ps_api.Poly.upload(ctx, list(range(1, len(pts) + 1))))
    try:
        both(proofs, ios, rhos, ("code", _lib.PS_ERR_ARG))
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    both(proofs, ios, rhos, ("ok",))
    assert _locate(ps_api, ctx, mat, [], [], [])[0] == []


def test_two_calls_of_different_size_leave_no_tree_behind(ps_api, ctx, pr, mat, tampered):
    rng = pr.SplitMix64(SEED + 4000)
    for n, positions in ((64, [63]), (7, [2]), (300, [150, 151]), (7, []), (64, [0])):
        proofs, ios = list(mat.proofs[:n]), [list(v) for v in mat.ios[:n]]
        for k, pos in enumerate(positions):
            proofs[pos], ios[pos] = tampered[(n + k) % 48][0], list(tampered[(n + k) % 48][1])
        bad, info = _locate(ps_api, ctx, mat, proofs, ios, _rhos(pr, rng, n, 128))
        assert bad == positions and info["invalid"] == len(positions)
        assert info["checks"] <= 1 + 2 * len(positions) * _ceil_log2(n)
