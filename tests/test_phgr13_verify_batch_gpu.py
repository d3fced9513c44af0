"""GPU: ps_phgr13_verify_batch -- PHGR13Verify (pinochio.go:281-378) for N proofs under one key: the five pairing products of
the single verifier, each weighted by the caller's rho and each with its own final exponentiation
(csrc/verify_phgr13_batch.inc).  Every compared quantity is a verdict, a mask of failed equations, a count or an error code.

Proofs come from PHGR13ProveBatch over distinct x0 of rs.synthetic_circuit(n, x0) (diff = n - 1 public inputs), as in
tests/test_phgr13_prove_batch_gpu.py; the one-gate circuit (diff = 0) is below what the device's setup takes, so its key and
proofs are the oracle's.  The references are PHGR13Verify on every proof, and for the N = 1 cases oracle.pairing.phgr13_verify
as recorded in tests/golden/phgr13_verify_batch_verdicts.json (tests/phgr13_verify_batch_cases.py holds the shared seeds)."""
import copy
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phgr13_verify_batch_cases as pc  # noqa: E402

SEED = pc.SEED
_WORLDS = {}


class _World:
    pass


def _world(ps_api, ctx, co, pr, n, k, x0s=None):
    """The key of the n-gate circuit (cached per n) and k proofs over distinct x0 with their public inputs"""
    from oracle import restate as rs

    x0s = pc.x0s(k) if x0s is None else x0s
    made = [rs.synthetic_circuit(n, x0=x) for x in x0s]
    c = made[0][0]
    for cc, _ in made[1:]:
        assert (cc.nbVars, cc.nbIO, cc.left, cc.right, cc.out) == (c.nbVars, c.nbIO, c.left, c.right, c.out)
    diff = c.nbVars - c.nbIO
    assert diff == n - 1
    up = lambda g, b: ps_api.Points.upload(ctx, g, b)
    if n not in _WORLDS:
        key = _World()
        tox = pc.toxic(pr, n)
        if n >= 2:
            key.q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
            key.ek, vk = ps_api.NewPHGR13TrustedSetup(key.q, *tox)
            key.fixed = vk.fixed_points()
            key.arrays = (vk.vs.slice(0, diff), vk.ws.slice(0, diff), vk.ys.slice(0, diff))
            key.keep = vk
        else:
            key.st = rs.phgr13_setup(c, *tox)
            v = key.st.VK
            key.fixed = {f: (co.G1 if f in ("aw", "bgamma") else co.G2).to_b(getattr(v, f)) for f in ps_api.PHGR13VerifKey.FIXED}
            key.arrays = (up(ps_api.G1, co.G1.pack(v.vs[:diff])), up(ps_api.G2, co.G2.pack(v.ws[:diff])), up(ps_api.G1, co.G1.pack(v.ys[:diff])))
        _WORLDS[n] = key
    key = _WORLDS[n]
    w = _World()
    w.key, w.diff, w.c = key, diff, c
    sols = [s for _, s in made]
    if n >= 2:
        w.proofs = ps_api.PHGR13ProveBatch(key.ek, key.q, ps_api.Poly.upload(ctx, [v for s in sols for v in s]), len(sols))
    else:
        raws = []
        for s in sols:
            o = rs.phgr13_prove(key.st.EK, c, s)
            raw = ps_api._lib.Phgr13Proof()
            for f in pc.FIELDS:
                ps_api.C.memmove(getattr(raw, f), bytes(getattr(o, f)), len(getattr(o, f)))
            raws.append(ps_api.PHGR13Proof(raw))
        w.proofs = raws
    w.ios = [s[:diff] for s in sols]
    return w


def _batch(ps_api, ctx, w, proofs, ios, rhos):
    """(verdict, failed mask, device loops)"""
    io = ps_api.Poly.upload(ctx, [v for row in ios for v in row])
    ok = ps_api.PHGR13VerifyBatch(ctx, w.key.fixed, *w.key.arrays, proofs, io, rhos)
    info = ps_api.PHGR13VerifyBatchInfo(ctx)
    return ok, info["failed"], info["device_loops"]


def _single(ps_api, ctx, w, p, io):
    return ps_api.PHGR13Verify(ctx, w.key.fixed, *w.key.arrays, p, ps_api.Poly.upload(ctx, io))


def _with(p, **kw):
    q = copy.copy(p)
    for f, v in kw.items():
        setattr(q, f, v)
    return q


def _fields(p):
    return {f: getattr(p, f) for f in pc.FIELDS}


def _tampered(ps_api, p, io, what, value):
    fields, io = pc.apply_tamper(_fields(p), io, what, value)
    return _with(p, **fields), io


def _rhos(pr, rng, n):
    return [(rng.fr() >> 127) or 1 for _ in range(n)]


def _add(pr, co, group, a_bytes, pt):
    grp, og = (pr.G2, co.G2) if group == 2 else (pr.G1, co.G1)
    return og.to_b(grp.add(og.from_b(a_bytes), pt))


@pytest.mark.parametrize("n,N", [(1, 2), (2, 1), (3, 7), (7, 1), (7, 2), (7, 65), (64, 3)])
def test_valid_batches_are_accepted(ps_api, ctx, co, pr, n, N):
    """Segments of 1, 2, 3, 7 and 64 terms (odd and even levels, carried nodes, a full wave); N = 65 crosses the 64 lanes of
    one Miller loop per lane."""
    w = _world(ps_api, ctx, co, pr, n, N)
    rng = pr.SplitMix64(SEED + 100 * n + N)
    assert _batch(ps_api, ctx, w, w.proofs, w.ios, _rhos(pr, rng, N)) == (True, 0, N + w.diff)
    assert _batch(ps_api, ctx, w, w.proofs, w.ios, [rng.fr() or 1 for _ in range(N)]) == (True, 0, N + w.diff)
    for p, io in zip(w.proofs, w.ios):
        assert _single(ps_api, ctx, w, p, io) is True


@pytest.mark.parametrize("N", [1, 7, 65])
def test_one_bad_element_is_rejected_with_the_exact_mask(ps_api, ctx, co, pr, N):
    """Each of the eight elements replaced by a random subgroup point, and one public input changed, at the first, the
    middle and the last proof: rejected, and `failed` names exactly the equations the element enters."""
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rng = pr.SplitMix64(SEED + 2000 + N)
    for pos in sorted({0, N // 2, N - 1}):
        for what in pc.KINDS:
            proofs, ios = list(w.proofs), [list(v) for v in w.ios]
            proofs[pos], ios[pos] = _tampered(ps_api, proofs[pos], ios[pos], what, pc.tamper_value(pr, co, what, w.diff, salt=N + pos))
            ok, failed, loops = _batch(ps_api, ctx, w, proofs, ios, _rhos(pr, rng, N))
            assert (ok, failed, loops) == (False, pc.MASK[what], N + w.diff), (pos, what, bin(failed))
            assert _single(ps_api, ctx, w, proofs[pos], ios[pos]) is False, (pos, what)


def test_errors_of_two_equations_of_one_proof_do_not_cancel(ps_api, ctx, co, pr):
    """vass + D and wass - D in ONE proof: under equal weights across the equations the two errors would cancel in a merged
    product.  The five products are checked apart, so E1 and E2 both fail."""
    w = _world(ps_api, ctx, co, pr, pc.GATES, 3)
    rng = pr.SplitMix64(SEED + 31)
    D = pr.G1.mul(rng.fr())
    p = w.proofs[1]
    proofs = list(w.proofs)
    proofs[1] = _with(p, vass=_add(pr, co, 1, p.vass, D), wass=_add(pr, co, 1, p.wass, pr.G1.neg(D)))
    ok, failed, _ = _batch(ps_api, ctx, w, proofs, w.ios, _rhos(pr, rng, 3))
    assert (ok, failed) == (False, 0b00110)
    assert _single(ps_api, ctx, w, proofs[1], w.ios[1]) is False


def test_the_weights_enter_every_equation(ps_api, ctx, co, pr):
    """Proof a gets vass + D, proof b gets vass - D: both are invalid, and in S_vass = sum rho_i vass_i the errors cancel
    exactly when rho_a = rho_b.  This is why rho is drawn AFTER the proofs are fixed: a forger who knows the weights can make
    errors of different proofs cancel."""
    w = _world(ps_api, ctx, co, pr, pc.GATES, 3)
    rng = pr.SplitMix64(SEED + 32)
    D = pr.G1.mul(rng.fr())
    a, b = w.proofs[0], w.proofs[2]
    proofs = [_with(a, vass=_add(pr, co, 1, a.vass, D)), w.proofs[1], _with(b, vass=_add(pr, co, 1, b.vass, pr.G1.neg(D)))]
    assert _single(ps_api, ctx, w, proofs[0], w.ios[0]) is False and _single(ps_api, ctx, w, proofs[2], w.ios[2]) is False
    r = rng.fr() >> 127
    assert _batch(ps_api, ctx, w, proofs, w.ios, [r, 5, r + 1])[:2] == (False, 0b00010)
    assert _batch(ps_api, ctx, w, proofs, w.ios, [r, 5, r])[:2] == (True, 0)


def test_identities_and_degenerate_sums(ps_api, ctx, co, pr):
    w = _world(ps_api, ctx, co, pr, pc.GATES, 3, x0s=[0, 0, 0])
    rng = pr.SplitMix64(SEED + 33)
    # the x0 = 0 witness: four all-zero io columns give four identity P_k, and zero scalars enter the scaling
    assert w.ios[0] == [1, 0, 130, 0, 0, 0]
    assert _batch(ps_api, ctx, w, w.proofs, w.ios, _rhos(pr, rng, 3)) == (True, 0, 3 + w.diff)
    w = _world(ps_api, ctx, co, pr, pc.GATES, 3)
    ident = {1: bytes([0x40]) + bytes(95), 2: bytes([0x40]) + bytes(191)}
    for what in ("vss", "wss", "hs"):
        proofs = list(w.proofs)
        proofs[1] = _with(proofs[1], **{what: ident[2 if what == "wss" else 1]})
        want = _single(ps_api, ctx, w, proofs[1], w.ios[1])
        assert want is False
        ok, failed, _ = _batch(ps_api, ctx, w, proofs, w.ios, _rhos(pr, rng, 3))
        assert (ok, failed) == (want, pc.MASK[what]), what
    # vss = -vio: rho gv is the identity (its Miller loop contributes one); vss = +vio: the last addition of gv is a doubling
    io1 = ps_api.Poly.upload(ctx, w.ios[1])
    vio = co.G1.from_b(io1.BlindEval(w.key.arrays[0]))
    for forged in (pr.G1.neg(vio), vio):
        proofs = list(w.proofs)
        proofs[1] = _with(proofs[1], vss=co.G1.to_b(forged))
        want = _single(ps_api, ctx, w, proofs[1], w.ios[1])
        assert want is False
        for N, ps, ios in ((3, proofs, w.ios), (1, proofs[1:2], w.ios[1:2])):
            ok, failed, _ = _batch(ps_api, ctx, w, ps, ios, _rhos(pr, rng, N))
            assert (ok, failed) == (want, pc.MASK["vss"])


def test_one_proof_with_weight_one_is_the_single_verifier_and_the_oracle(ps_api, ctx, co, pr):
    """N = 1, rho = 1: the verdict of PHGR13Verify, and of oracle.pairing.phgr13_verify as recorded for these very bytes."""
    from oracle import restate as rs

    recorded = pc.recorded_verdicts()
    w = _world(ps_api, ctx, co, pr, pc.GATES, 1)
    w0 = _world(ps_api, ctx, co, pr, pc.GATES, 1, x0s=[0])
    p, io = w.proofs[0], w.ios[0]
    cases = [("valid", p, io)] + [(what,) + _tampered(ps_api, p, io, what, pc.tamper_value(pr, co, what, w.diff)) for what in pc.KINDS]
    cases.append(("x0=0", w0.proofs[0], w0.ios[0]))
    assert len(cases) == 11 == len(recorded)
    for name, pf, pub in cases:
        key = pc.digest(_fields(pf), pub)
        assert key in recorded, name  # the device's proof is the bytes the oracle's verdict was recorded for
        single = _single(ps_api, ctx, w, pf, pub)
        ok, failed, loops = _batch(ps_api, ctx, w, [pf], [pub], [1])
        assert ok is single is recorded[key], name
        assert recorded[key] is (name in ("valid", "x0=0"))
        assert failed == (0 if ok else pc.MASK[name]) and loops == 1 + w.diff


def test_errors(ps_api, ctx, co, pr, off_subgroup):
    from playsnark_amd import _lib

    N = 5
    w = _world(ps_api, ctx, co, pr, pc.GATES, N)
    rhos = [3, 5, 7, 11, 13]
    good = lambda: _batch(ps_api, ctx, w, w.proofs, w.ios, rhos) == (True, 0, N + w.diff)

    def err(fn):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            fn()
        return e.value.code, str(e.value)

    assert good()
    for what in ("yass", "wss"):  # not on the curve: the message names the proof and the element
        junk = list(w.proofs)
        junk[3] = _with(junk[3], **{what: b"\x01" + getattr(junk[3], what)[1:]})
        code, msg = err(lambda: _batch(ps_api, ctx, w, junk, w.ios, rhos))
        assert code == _lib.PS_ERR_ENCODING and "proof 3" in msg and what in msg, msg
        assert good()
    for what, pt in (("vss", co.G1.to_b(off_subgroup[0])), ("wss", co.G2.to_b(off_subgroup[1])), ("gz", co.G1.to_b(off_subgroup[0]))):
        bad = list(w.proofs)
        bad[2] = _with(bad[2], **{what: pt})
        code, msg = err(lambda: _batch(ps_api, ctx, w, bad, w.ios, rhos))
        assert code == _lib.PS_ERR_ENCODING and "proof 2" in msg and what in msg, msg
        assert good()
    assert err(lambda: _batch(ps_api, ctx, w, w.proofs, w.ios, [3, 0, 7, 11, 13]))[0] == _lib.PS_ERR_ARG
    assert good()
    assert err(lambda: _batch(ps_api, ctx, w, w.proofs, w.ios, [3, pr.R, 7, 11, 13]))[0] == _lib.PS_ERR_ENCODING
    assert err(lambda: _batch(ps_api, ctx, w, w.proofs, w.ios, [3, 2**256 - 1, 7, 11, 13]))[0] == _lib.PS_ERR_ENCODING
    assert good()
    with pytest.raises(ps_api.LengthMismatch):
        _batch(ps_api, ctx, w, w.proofs, w.ios[:4] + [w.ios[4][:-1]], rhos)
    assert good()
    with pytest.raises(ps_api.LengthMismatch):  # key arrays of different lengths
        ps_api.PHGR13VerifyBatch(ctx, w.key.fixed, w.key.arrays[0], w.key.arrays[1].slice(0, w.diff - 1), w.key.arrays[2], w.proofs,
                                 ps_api.Poly.upload(ctx, [v for row in w.ios for v in row]), rhos)
    assert good()
    pts = ps_api.Points.upload(ctx, ps_api.G1, co.G1.gen_points(3, 5, 8))
    ps_api.msm_launch(ctx, pts, ps_api.Poly.upload(ctx, list(range(1, len(pts) + 1))))  # a pending sum on the context
    try:
        assert err(lambda: _batch(ps_api, ctx, w, w.proofs, w.ios, rhos))[0] == _lib.PS_ERR_ARG
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    assert good()
    assert _batch(ps_api, ctx, w, [], [], []) == (True, 0, 0)
    assert good()


def test_caps_are_checked_before_any_device_work(ps_api, ctx, co, pr):
    """More than 2^20 proofs, and proofs x (diff + 1) >= 2^24: PS_ERR_ARG with the advice to split, before the proofs or the
    weights are read (one proof and one weight stand for all: a call that read further would fail differently)."""
    from playsnark_amd import _lib

    C = ps_api.C
    w = _world(ps_api, ctx, co, pr, 64, 3)
    vk = _lib.Phgr13Vk()
    for name in ps_api.PHGR13VerifKey.FIXED:
        C.memmove(getattr(vk, name), w.key.fixed[name], len(w.key.fixed[name]))
    vk.vs_io, vk.ws_io, vk.ys_io = (a._h for a in w.key.arrays)
    raw = (_lib.Phgr13Proof * 1)()
    io = ps_api.Poly.upload(ctx, w.ios[0])
    for nproofs in ((1 << 20) + 1, 1 << 18):  # 2^18 x 64 = 2^24
        ok = C.c_int(7)
        assert ps_api.lib.ps_phgr13_verify_batch(ctx._h, C.byref(vk), io._h, raw, nproofs, bytes(32), C.byref(ok)) == _lib.PS_ERR_ARG
        assert ok.value == 0 and b"split" in ps_api.lib.ps_last_error()
    assert _batch(ps_api, ctx, w, w.proofs, w.ios, [3, 5, 7]) == (True, 0, 3 + w.diff)
