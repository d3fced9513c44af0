"""GPU: ps_phgr13_prove_batch -- K witnesses of one circuit under one evaluation key in one call (csrc/phgr13_batch.inc) --
field by field against K calls of PHGR13Prove, against the oracle's restatement of pinochio.go:207-254, and through
PHGR13Verify.

Witnesses: rs.synthetic_circuit(n, x0=...) tiles the same gates whatever x0 is; only the wire values change.  Every case
checks that on the CPU first (the three matrices of all K circuits are equal) and then proves the K solution vectors over
the FIRST circuit's QAP and key.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x70686772626174 & 0xFFFFFFFFFFFFFFFF


class _World:
    pass


def _world(ps_api, ctx, pr, n, k, salt=0):
    """One circuit of n gates, its device key (gsi in both forms) and K witnesses from K values of x0."""
    from oracle import restate as rs

    w = _World()
    rng = pr.SplitMix64(SEED + 1000 * n + k + salt)
    made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(k)]
    w.c = made[0][0]
    for c, _ in made[1:]:  # the matrices do not depend on x0
        assert (c.nbVars, c.nbIO, c.left, c.right, c.out) == (w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.sols = [sol for _, sol in made]
    assert len({tuple(s) for s in w.sols}) == k
    w.tox = [rng.fr() for _ in range(8)]
    w.q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.ek, w.vk = ps_api.NewPHGR13TrustedSetup(w.q, *w.tox)
    w.flat = [v for s in w.sols for v in s]
    return w


def _fields(ps_api, p):
    return tuple(getattr(p, f) for f in ps_api.PHGR13Proof.FIELDS)


def _singles(ps_api, ctx, w, idx=None):
    idx = range(len(w.sols)) if idx is None else idx
    return {j: _fields(ps_api, ps_api.PHGR13Prove(w.ek, w.q, ps_api.Poly.upload(ctx, w.sols[j]))) for j in idx}


ZERO = (bytes(96), bytes(96), bytes(192), bytes(96), bytes(96), bytes(96), bytes(96), bytes(96))


@pytest.mark.parametrize("n,k", [(2, 1), (7, 3), (64, 8), (300, 5)])
def test_batch_proofs_equal_single_proofs_and_verify(ps_api, ctx, co, pr, n, k):
    from oracle import restate as rs

    w = _world(ps_api, ctx, pr, n, k)
    got = ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, w.flat), k)
    assert len(got) == k
    want = _singles(ps_api, ctx, w)
    diff = w.c.nbVars - w.c.nbIO
    args = (w.vk.vs.slice(0, diff), w.vk.ws.slice(0, diff), w.vk.ys.slice(0, diff))
    for j in range(k):
        for f, a, b in zip(ps_api.PHGR13Proof.FIELDS, _fields(ps_api, got[j]), want[j]):
            assert a == b, (n, k, j, f)
        io = ps_api.Poly.upload(ctx, w.sols[j][:diff])
        assert ps_api.PHGR13Verify(ctx, w.vk.fixed_points(), *args, got[j], io) is True, j
    if (n, k) == (7, 3):
        ref = rs.phgr13_setup(w.c, *w.tox)
        for j in range(k):
            o = rs.phgr13_prove(ref.EK, w.c, w.sols[j])
            for f in ps_api.PHGR13Proof.FIELDS:
                assert getattr(got[j], f) == getattr(o, f), (j, f)


def test_batch_violated_gate_flags_apocalypse_and_recovery(ps_api, ctx, co, pr):
    """Witness 1 of 3 violates a gate.  With `valid`: [1, 0, 1], proof 1 all zero bytes, proofs 0 and 2 unchanged.  Without:
    Apocalypse (qap.go:158-160), the message names witness 1, and the context proves correctly right after."""
    w = _world(ps_api, ctx, pr, 7, 3, salt=1)
    want = _singles(ps_api, ctx, w)
    bad = [list(s) for s in w.sols]
    bad[1][4] = (bad[1][4] + 1) % pr.R
    flat = [v for s in bad for v in s]
    proofs, flags = ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, flat), 3, valid=True)
    assert flags == [1, 0, 1]
    assert _fields(ps_api, proofs[1]) == ZERO
    assert _fields(ps_api, proofs[0]) == want[0] and _fields(ps_api, proofs[2]) == want[2]
    with pytest.raises(ps_api.Apocalypse):
        ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, flat), 3)
    assert b"witness 1 " in ps_api.lib.ps_last_error()
    good = ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, w.flat), 3)
    assert [_fields(ps_api, p) for p in good] == [want[j] for j in range(3)]
    proofs, flags = ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, w.flat), 3, valid=True)
    assert flags == [1, 1, 1] and [_fields(ps_api, p) for p in proofs] == [want[j] for j in range(3)]


def test_batch_needs_lgsi_and_the_right_length(ps_api, ctx, co, pr):
    w = _world(ps_api, ctx, pr, 7, 3, salt=2)
    sols = ps_api.Poly.upload(ctx, w.flat)
    want = [_fields(ps_api, p) for p in ps_api.PHGR13ProveBatch(w.ek, w.q, sols, 3)]
    mono = w.ek.monomial_only()
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.PHGR13ProveBatch(mono, w.q, sols, 3)
    assert e.value.code == -5 and "ps_points_monomial_to_lagrange" in str(e.value)
    # the Lagrange form computed from gsi alone gives the same bytes
    assert [_fields(ps_api, p) for p in ps_api.PHGR13ProveBatch(mono.with_lagrange(w.q), w.q, sols, 3)] == want
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, w.flat[:-1]), 3)
    assert e.value.code == -5
    with pytest.raises(ps_api.PlaysnarkError):
        ps_api.PHGR13ProveBatch(w.ek, w.q, sols, 2)
    assert ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, []), 0) == []
    assert ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, []), 0, valid=True) == ([], [])


def test_batch_int64_witnesses_and_passes(ps_api, ctx, co, pr):
    """Witnesses uploaded as int64 (x0 = -3, -5, ..: every wire a small signed integer) give the bytes of their be32 upload;
    set_batch_chunk(2) with K = 5 (passes of 2, 2 and 1) gives the bytes of the automatic split."""
    from oracle import restate as rs

    n, k = 8, 5
    made = [rs.synthetic_circuit(n, x0=pr.R - 3 - 2 * j) for j in range(k)]
    c = made[0][0]
    for cc, _ in made[1:]:
        assert (cc.left, cc.right, cc.out, cc.nbVars) == (c.left, c.right, c.out, c.nbVars)
    sols = [s for _, s in made]
    wits = [[v if v < pr.R // 2 else v - pr.R for v in s] for s in sols]
    assert min(min(wt) for wt in wits) < 0 and max(abs(v) for wt in wits for v in wt) < 1 << 62
    rng = pr.SplitMix64(SEED + 64)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    flat = [v for s in sols for v in s]
    be = [_fields(ps_api, p) for p in ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, flat), k)]
    i64 = ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.from_values(ctx, [v for wt in wits for v in wt]), k)
    assert [_fields(ps_api, p) for p in i64] == be
    single = ps_api.PHGR13Prove(ek, q, ps_api.Poly.from_values(ctx, wits[3]))
    assert _fields(ps_api, single) == be[3]
    try:
        ctx.set_batch_chunk(2)
        chunked = ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, flat), k)
    finally:
        ctx.set_batch_chunk(0)
    assert [_fields(ps_api, p) for p in chunked] == be


def test_batch_with_a_gate_of_more_than_512_terms(ps_api, ctx, co, pr):
    """One gate of 600 terms (SPMV_LONG_ROW = 512: its row is summed by k_spmv_long_rows_batch) behind 700 tiled gates: S =
    the sum of 600 intermediate wires, a new last variable.  Two witnesses."""
    from oracle import restate as rs

    n, k, terms = 700, 2, 600
    sols, c = [], None
    for j in range(k):
        base, sol = rs.synthetic_circuit(n, x0=3 + 2 * j)
        assert base.nbVars >= 3 + terms
        cols = list(range(3, 3 + terms))
        cc = rs.SparseR1CS(base.nbVars + 1, base.nbIO, base.left + [[(i, 1) for i in cols]], base.right + [[(0, 1)]],
                           base.out + [[(base.nbVars, 1)]])
        if c is not None:
            assert (cc.left, cc.right, cc.out, cc.nbVars) == (c.left, c.right, c.out, c.nbVars)
        c = cc
        sols.append(sol + [sum(sol[i] for i in cols) % pr.R])
    assert max(len(r) for r in c.left) == terms > 512
    rng = pr.SplitMix64(SEED + 600)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    got = ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, [v for s in sols for v in s]), k)
    for j in range(k):
        assert _fields(ps_api, got[j]) == _fields(ps_api, ps_api.PHGR13Prove(ek, q, ps_api.Poly.upload(ctx, sols[j]))), j
    bad = [list(s) for s in sols]
    bad[1][-1] = (bad[1][-1] + 1) % pr.R  # the long gate alone is violated
    _, flags = ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, [v for s in bad for v in s]), k, valid=True)
    assert flags == [1, 0]


def test_other_provers_on_the_same_context_afterwards(ps_api, ctx, co, pr):
    """A PHGR13Prove and a Groth16ProveBatch on the context right after a batch are still correct (the batch leaves no sum
    pending and no workspace busy)."""
    from oracle import restate as rs

    w = _world(ps_api, ctx, pr, 8, 4, salt=3)
    before = _fields(ps_api, ps_api.PHGR13Prove(w.ek, w.q, ps_api.Poly.upload(ctx, w.sols[2])))
    batch = ps_api.PHGR13ProveBatch(w.ek, w.q, ps_api.Poly.upload(ctx, w.flat), 4)
    assert _fields(ps_api, batch[2]) == before
    assert _fields(ps_api, ps_api.PHGR13Prove(w.ek, w.q, ps_api.Poly.upload(ctx, w.sols[2]))) == before
    rng = pr.SplitMix64(SEED + 16)
    tox = [rng.fr() for _ in range(5)]
    tr, _ = ps_api.NewGroth16TrustedSetup(w.q, *tox)
    rr, ss = [rng.fr() for _ in range(4)], [rng.fr() for _ in range(4)]
    g16 = ps_api.Groth16ProveBatch(tr, w.q, ps_api.Poly.upload(ctx, w.flat), rr, ss)
    ref = rs.groth16_setup(w.c, *tox)
    for j in (0, 3):
        o = rs.groth16_prove(ref, w.c, w.sols[j], rr[j], ss[j])
        assert (g16[j].A, g16[j].B, g16[j].C) == (o.A, o.B, o.C), j
