"""GPU: ps_phgr13_verify_batch_locate -- WHICH proofs of a PHGR13 batch are invalid and which of the five equations each one
violates, by bisection over partial results kept on the device (csrc/verify_phgr13_locate.inc).

Material is that of tests/test_phgr13_verify_batch_gpu.py (its _world helper and tests/phgr13_verify_batch_cases.py, imported,
not edited).  The references are PHGR13Verify on every proof (PHGR13VerifyBatch(locate=True) runs exactly that loop) and
pc.MASK for the masks.  The weights are distinct 128-bit values drawn per test.  Every compared quantity is a verdict, an
index, a mask, a count or an error code; the bounds are the issue's: an accepted batch is checks 1, products 5, levels 0;
b invalid proofs among N cost checks <= 1 + 2 b ceil(log2 N) and products <= 5 + 2 ceil(log2 N) sum_i popcount(failed[i])."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phgr13_verify_batch_cases as pc  # noqa: E402
from test_phgr13_verify_batch_gpu import _add, _batch, _single, _tampered, _with, _world  # noqa: E402

SEED = pc.SEED + 0x6C6F63
ACCEPTED = {"checks": 1, "products": 5, "levels": 0, "invalid": 0, "failed": 0}


def _ceil_log2(n):
    return (n - 1).bit_length()


def _popcount(m):
    return bin(m).count("1")


def _rhos(pr, rng, n):
    """n distinct non-zero 128-bit weights"""
    out = []
    while len(out) < n:
        v = rng.fr() >> 127
        if v and v not in out:
            out.append(v)
    return out


def _io(ps_api, ctx, ios):
    return ps_api.Poly.upload(ctx, [v for row in ios for v in row])


def _locate(ps_api, ctx, w, proofs, ios, rhos):
    """(bad indices, {index: mask}, info)"""
    return ps_api.PHGR13VerifyBatchLocate(ctx, w.key.fixed, *w.key.arrays, proofs, _io(ps_api, ctx, ios), rhos)


def _loop(ps_api, ctx, w, proofs, ios, rhos):
    return ps_api.PHGR13VerifyBatch(ctx, w.key.fixed, *w.key.arrays, proofs, _io(ps_api, ctx, ios), rhos, locate=True)


def _check(ps_api, ctx, w, proofs, ios, rhos, want):
    """One batch with the invalid proofs `want` = {index: mask}: indices and masks exact, the per-proof loop agrees, the
    single verifier rejects exactly the reported proofs, the counts are bounded"""
    n = len(proofs)
    bad, masks, info = _locate(ps_api, ctx, w, proofs, ios, rhos)
    lg, b, bits = _ceil_log2(n), len(want), sum(_popcount(m) for m in want.values())
    print(f"N = {n}, b = {b}: checks = {info['checks']} (bound {1 + 2 * b * lg}), products = {info['products']} (bound {5 + 2 * lg * bits}), "
          f"levels = {info['levels']}")
    assert bad == sorted(want) and masks == want, (bad, {i: bin(m) for i, m in masks.items()})
    assert bad == _loop(ps_api, ctx, w, proofs, ios, rhos)
    assert [_single(ps_api, ctx, w, p, io) for p, io in zip(proofs, ios)] == [i not in want for i in range(n)]
    union = 0
    for m in want.values():
        union |= m
    assert info["invalid"] == b and info["failed"] == union
    assert ps_api.PHGR13VerifyBatchInfo(ctx)["failed"] == union  # the root's mask, as after the plain call
    if not b:
        assert info == ACCEPTED
    else:
        assert info["levels"] == lg
        assert 1 <= info["checks"] <= 1 + 2 * b * lg
        assert 5 <= info["products"] <= 5 + 2 * lg * bits
    return info


def _tamper_at(ps_api, pr, co, w, proofs, ios, pos, what, salt):
    proofs[pos], ios[pos] = _tampered(ps_api, proofs[pos], ios[pos], what, pc.tamper_value(pr, co, what, w.diff, salt=salt))


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1, 2), (2, 1), (7, 1), (7, 7), (7, 65), (64, 3)])
def test_accepted_batches_cost_one_check_and_five_products(ps_api, ctx, co, pr, n, N):
    w = _world(ps_api, ctx, co, pr, n, N)
    rng = pr.SplitMix64(SEED + 100 * n + N)
    bad, masks, info = _locate(ps_api, ctx, w, w.proofs, w.ios, _rhos(pr, rng, N))
    assert bad == [] and masks == {} and info == ACCEPTED
    assert ps_api.PHGR13VerifyBatchInfo(ctx) == {"failed": 0, "device_loops": N + w.diff}


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,which", [(N, k) for N in (1, 2, 7, 65) for k in range(len({0, N // 2, N - 1}))])
def test_one_bad_element_is_located_with_its_mask(ps_api, ctx, co, pr, N, which):
    """Each of the eight elements replaced by a random subgroup point, and one public input changed, at the first, the
    middle or the last proof"""
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 2000 + 8 * N + which)
    pos = sorted({0, N // 2, N - 1})[which]
    for what in pc.KINDS:
        proofs, ios = list(w.proofs), [list(v) for v in w.ios]
        _tamper_at(ps_api, pr, co, w, proofs, ios, pos, what, N + pos)
        bad, masks, info = _locate(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N))
        lg = _ceil_log2(N)
        assert bad == [pos] and masks == {pos: pc.MASK[what]}, (what, bad, masks)
        assert _single(ps_api, ctx, w, proofs[pos], ios[pos]) is False, what
        assert info["levels"] == lg and info["invalid"] == 1 and info["failed"] == pc.MASK[what]
        assert info["checks"] <= 1 + 2 * lg, (what, info)
        assert info["products"] <= 5 + 2 * lg * _popcount(pc.MASK[what]), (what, info)


# 3 -------------------------------------------------------------------------------------------------------------------------
MANY = {
    "n2-both": (2, [0, 1]),
    "n7-all": (7, list(range(7))),
    "n7-last": (7, [6]),  # a node carried at two levels
    "n65-ends": (65, [0, 64]),
    "n65-siblings": (65, [32, 33]),
    "n65-every-other": (65, list(range(0, 65, 2))),
}


@pytest.mark.parametrize("case", list(MANY))
def test_several_bad_proofs_are_located(ps_api, ctx, co, pr, case):
    N, positions = MANY[case]
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 3000 + sum(ord(ch) for ch in case))
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    shift = rng.next() % len(pc.KINDS)
    want = {}
    for k, pos in enumerate(positions):
        what = pc.KINDS[(shift + k) % len(pc.KINDS)]  # neighbours in the list get different kinds
        _tamper_at(ps_api, pr, co, w, proofs, ios, pos, what, 31 * N + pos)
        want[pos] = pc.MASK[what]
    assert len(positions) < 2 or len(set(want.values())) > 1
    _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N), want)


def test_exact_counts_of_one_carried_leaf(ps_api, ctx, co, pr):
    """N = 7, proof 6 alone invalid, in vss (E0, E1 and E4): the counts of a rejected batch as exact numbers, worked out by
    hand from the levels of 7, 4, 2, 1 nodes -- the batch check (1 check, 5 products); the root's two children, nodes 0 and 1
    of 2, on the root's three equations (2 checks, 6 products), node 1 (proofs 4 .. 6) fails all three; its two children,
    nodes 2 and 3 of 4 (2, 6), node 3 (proof 6) fails all three; node 3 has the single child 6 of 7, carried, handed down
    without a check (0, 0).  1 + 2 + 2 + 0 = 5 checks over 3 levels, 5 + 4 popcount(mask) = 17 products."""
    N, mask = 7, pc.MASK["vss"]
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 5000)
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 6, "vss", 5006)
    info = _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N), {6: mask})
    assert _popcount(mask) == 3
    assert info == {"checks": 5, "products": 5 + 4 * _popcount(mask), "levels": 3, "invalid": 1, "failed": mask}


def test_tree_shape_of_the_carried_case():
    sizes = lambda n: [n] + ([] if n == 1 else sizes((n + 1) // 2))
    assert sizes(7) == [7, 4, 2, 1] and sizes(65) == [65, 33, 17, 9, 5, 3, 2, 1]
    assert 6 // 2 == 3 and 7 % 2 == 1  # proof 6 of 7 is carried from the leaves, and proof 64 of 65 at six levels


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_two_equations_of_one_proof(ps_api, ctx, co, pr):
    """vass + D and wass - D in ONE proof: E1 and E2 of that proof alone"""
    w = _world(ps_api, ctx, co, pr, pc.GATES, 7)
    rng = pr.SplitMix64(SEED + 41)
    D = pr.G1.mul(rng.fr())
    proofs = list(w.proofs)
    p = proofs[4]
    proofs[4] = _with(p, vass=_add(pr, co, 1, p.vass, D), wass=_add(pr, co, 1, p.wass, pr.G1.neg(D)))
    _check(ps_api, ctx, w, proofs, w.ios, _rhos(pr, rng, 7), {4: 0b00110})


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_two_proofs_with_different_equations_keep_their_own_masks(ps_api, ctx, co, pr):
    """Proof 1 bad in vass (E1 only), proof 5 bad in yass (E3 only), in different halves of seven: the root fails E1 and E3,
    each half is tested on both, and each proof is reported with its own equation alone"""
    w = _world(ps_api, ctx, co, pr, pc.GATES, 7)
    rng = pr.SplitMix64(SEED + 51)
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 1, "vass", 501)
    _tamper_at(ps_api, pr, co, w, proofs, ios, 5, "yass", 505)
    info = _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, 7), {1: 0b00010, 5: 0b01000})
    assert info["failed"] == 0b01010


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_identity_hs(ps_api, ctx, co, pr):
    """Whatever PHGR13Verify and the plain batch's `failed` say for the same input"""
    w = _world(ps_api, ctx, co, pr, pc.GATES, 3)
    rng = pr.SplitMix64(SEED + 61)
    proofs = list(w.proofs)
    proofs[1] = _with(proofs[1], hs=bytes([0x40]) + bytes(95))
    rhos = _rhos(pr, rng, 3)
    single = _single(ps_api, ctx, w, proofs[1], w.ios[1])
    ok, failed, _ = _batch(ps_api, ctx, w, proofs, w.ios, rhos)
    assert ok is single and (failed != 0) is (not single)
    bad, masks, info = _locate(ps_api, ctx, w, proofs, w.ios, rhos)
    assert bad == ([] if single else [1]) and masks == ({} if single else {1: failed}) and info["failed"] == failed


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_no_public_inputs(ps_api, ctx, co, pr):
    """The one-gate key: diff = 0, no scalar tree, no P trees, no device loops in a round"""
    w = _world(ps_api, ctx, co, pr, 1, 2)
    assert w.diff == 0
    rng = pr.SplitMix64(SEED + 71)
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 1, "gz", 71)
    _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, 2), {1: pc.MASK["gz"]})
    # ... and E0 with diff = 0: hs
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 0, "hs", 72)
    _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, 2), {0: pc.MASK["hs"]})


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_sixty_three_public_inputs(ps_api, ctx, co, pr):
    """The 64-gate key, three proofs, one changed public input: E0 alone, 63 device loops per tested set"""
    w = _world(ps_api, ctx, co, pr, 64, 3)
    assert w.diff == 63
    rng = pr.SplitMix64(SEED + 81)
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 2, "io", 81)
    _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, 3), {2: 0b00001})
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 0, "vss", 82)  # every tree at once
    _check(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, 3), {0: pc.MASK["vss"]})


# 9 -------------------------------------------------------------------------------------------------------------------------
def _raw_locate(ps_api, ctx, w, proofs, io, rhos):
    """(return code, *ninvalid, message) of the C entry, *ninvalid set to 7 beforehand"""
    C = ps_api.C
    vk, io, raw, n, rho = ps_api._phgr13_batch_args(ctx, w.key.fixed, *w.key.arrays, proofs, io, rhos)
    valid, failed = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(n, 1))
    ninvalid = C.c_size_t(7)
    rc = ps_api.lib.ps_phgr13_verify_batch_locate(ctx._h, C.byref(vk), io._h, raw, n, rho, valid, failed, C.byref(ninvalid))
    return rc, ninvalid.value, (ps_api.lib.ps_last_error() or b"").decode()


def test_errors_are_those_of_the_plain_batch_call(ps_api, ctx, co, pr, off_subgroup):
    from playsnark_amd import _lib

    N = 5
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rhos = [3, 5, 7, 11, 13]
    io = _io(ps_api, ctx, w.ios)
    good = lambda: _locate(ps_api, ctx, w, w.proofs, w.ios, rhos) == ([], {}, ACCEPTED)

    def plain_code(proofs, pub, weights):
        try:
            ps_api.PHGR13VerifyBatch(ctx, w.key.fixed, *w.key.arrays, proofs, pub, weights)
        except ps_api.PlaysnarkError as e:
            return e.code
        except ps_api.LengthMismatch:
            return _lib.PS_ERR_LENGTH
        return _lib.PS_OK

    def both(proofs, pub, weights, want):
        rc, ninvalid, msg = _raw_locate(ps_api, ctx, w, proofs, pub, weights)
        assert rc == want == plain_code(proofs, pub, weights) and ninvalid == 0, (rc, want, ninvalid, msg)
        return msg

    assert good()
    for what in ("yass", "wss"):  # not on the curve: the message names the proof and the element
        junk = list(w.proofs)
        junk[3] = _with(junk[3], **{what: b"\x01" + getattr(junk[3], what)[1:]})
        msg = both(junk, io, rhos, _lib.PS_ERR_ENCODING)
        assert "proof 3" in msg and what in msg and "ps_phgr13_verify_batch_locate" in msg, msg
        assert good()
    for what, pt in (("vss", co.G1.to_b(off_subgroup[0])), ("wss", co.G2.to_b(off_subgroup[1])), ("gz", co.G1.to_b(off_subgroup[0]))):
        off = list(w.proofs)
        off[2] = _with(off[2], **{what: pt})
        msg = both(off, io, rhos, _lib.PS_ERR_ENCODING)
        assert "proof 2" in msg and what in msg, msg
        assert good()
    both(w.proofs, io, [3, 0, 7, 11, 13], _lib.PS_ERR_ARG)
    both(w.proofs, io, [3, pr.R, 7, 11, 13], _lib.PS_ERR_ENCODING)
    assert good()
    both(w.proofs, _io(ps_api, ctx, w.ios[:4] + [w.ios[4][:-1]]), rhos, _lib.PS_ERR_LENGTH)
    assert good()
    pts = ps_api.Points.upload(ctx, ps_api.G1, co.G1.gen_points(3, 5, 8))
    ps_api.msm_launch(ctx, pts, ps_api.Poly.upload(ctx, list(range(1, len(pts) + 1))))  # a pending sum on the context
    try:
        both(w.proofs, io, rhos, _lib.PS_ERR_ARG)
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    assert good()
    assert _raw_locate(ps_api, ctx, w, [], _io(ps_api, ctx, []), [])[:2] == (_lib.PS_OK, 0)
    assert good()


# 10 ------------------------------------------------------------------------------------------------------------------------
def test_a_plain_batch_is_the_same_before_and_after_a_locating_call(ps_api, ctx, co, pr):
    """(ok, failed, device_loops) of ps_phgr13_verify_batch on the shared context, before and after locating calls, are those
    of a context that never located anything"""
    N = 7
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 101)
    bad_proofs, bad_ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, bad_proofs, bad_ios, 3, "yss", 101)
    rhos = _rhos(pr, rng, N)
    fresh = ps_api.Context(0)
    try:
        ref_good = _batch(ps_api, fresh, w, w.proofs, w.ios, rhos)
        ref_bad = _batch(ps_api, fresh, w, bad_proofs, bad_ios, rhos)
    finally:
        fresh.close()
    assert ref_good == (True, 0, N + w.diff) and ref_bad == (False, pc.MASK["yss"], N + w.diff)
    assert _batch(ps_api, ctx, w, w.proofs, w.ios, rhos) == ref_good and _batch(ps_api, ctx, w, bad_proofs, bad_ios, rhos) == ref_bad
    assert _locate(ps_api, ctx, w, bad_proofs, bad_ios, rhos)[:2] == ([3], {3: pc.MASK["yss"]})
    assert _batch(ps_api, ctx, w, bad_proofs, bad_ios, rhos) == ref_bad and _batch(ps_api, ctx, w, w.proofs, w.ios, rhos) == ref_good
    assert _locate(ps_api, ctx, w, w.proofs, w.ios, rhos) == ([], {}, ACCEPTED)
    assert _batch(ps_api, ctx, w, bad_proofs, bad_ios, rhos) == ref_bad


def test_the_groth16_locator_on_the_same_context_keeps_its_verdicts(ps_api, ctx, co, pr):
    """The two locators share the context's tree buffers: a Groth16 descent between two PHGR13 descents still gives the
    recorded verdicts, and the PHGR13 descent after it its own"""
    from oracle import restate as rs

    import verify_batch_cases as vc

    N = 7
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 102)
    proofs, ios = list(w.proofs), [list(v) for v in w.ios]
    _tamper_at(ps_api, pr, co, w, proofs, ios, 5, "vss", 102)
    want = ([5], {5: pc.MASK["vss"]})
    assert _locate(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N))[:2] == want
    # seven Groth16 proofs of tests/verify_batch_cases.py and the first recorded tamper of the N = 7 set
    c, sols, tr, draws, diff = vc.material(pr, rs)
    up = lambda g, b: ps_api.Points.upload(ctx, g, b)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    pk = ps_api.Groth16Setup(tr.Alpha, tr.Beta, tr.Delta, tr.Beta2, tr.Delta2, up(ps_api.G1, tr.Xi), up(ps_api.G2, tr.Xi2), up(ps_api.G1, tr.NioLP),
                             up(ps_api.G1, tr.XiT))
    dsols = [ps_api.Poly.upload(ctx, s) for s in sols]
    gp = [ps_api.Groth16Prove(pk, q, dsols[wi], r, s) for wi, r, s in draws[:N]]
    gio = [list(sols[wi][:diff]) for wi, _, _ in draws[:N]]
    pos, what, value = vc.tampers(pr, co, N, diff)[0]
    (a, b, cc), gio[pos] = vc.apply_tamper((gp[pos].A, gp[pos].B, gp[pos].C), gio[pos], what, value)
    gp[pos] = ps_api.Groth16Proof(gp[pos].R, gp[pos].S, a, b, cc)
    recorded = vc.recorded_verdicts()
    verdicts = [recorded[vc.digest((p.A, p.B, p.C), io)] for p, io in zip(gp, gio)]
    assert verdicts == [i != pos for i in range(N)]
    bad, info = ps_api.Groth16VerifyBatchLocate(ctx, tr.Alpha, tr.Beta2, tr.Gamma, tr.Delta2, up(ps_api.G1, tr.IoLP), gp, _io(ps_api, ctx, gio),
                                                _rhos(pr, rng, N))
    assert bad == [pos] and info["invalid"] == 1
    assert _locate(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N))[:2] == want
