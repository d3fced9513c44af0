"""GPU: ps_groth16_prove_batch and ps_phgr13_prove_batch with their sums over the keys' window tables (ps_msm_batch_set_table
mode 2: one bucket set per member, no fold) -- byte for byte against the loops of single proofs -- and, on a fresh context
that builds no tables (set_tables(False)), the same bytes over the plain route.  The circuits are those of
tests/test_groth16_prove_batch_gpu.py and tests/test_phgr13_prove_batch_gpu.py (300 gates), K = 5.

PHGR13 sums its solution arrays over solution[diff:], which for rs.synthetic_circuit (nbIO = 3) is THREE points per array --
below the 32 points from which the provers build tables (PS_TABLE_MIN_POINTS), for the single prover as for the batch.  Over
that circuit only the h sum (299 points of lgsi) runs over a table; it is followed by the solution sums, so last_msm_info
reports their plain pass, and what is checked is the bytes and that lgsi got its table.  The tabled route of the solution
sums is checked over rs.bit_circuit(64): 64 booleanity gates, 64 points per solution array, 63 in lgsi.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x7062746162 & 0xFFFFFFFFFFFFFFFF
N, K = 300, 5


class _World:
    pass


def _circuit(pr):
    from oracle import restate as rs

    w = _World()
    made = [rs.synthetic_circuit(N, x0=3 + 2 * j) for j in range(K)]
    w.c = made[0][0]
    for c, _ in made[1:]:  # the matrices do not depend on x0
        assert (c.nbVars, c.nbIO, c.left, c.right, c.out) == (w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.sols = [sol for _, sol in made]
    w.flat = [v for s in w.sols for v in s]
    rng = pr.SplitMix64(SEED)
    w.tox = [rng.fr() for _ in range(8)]
    w.rs = [rng.fr() for _ in range(K)]
    w.ss = [rng.fr() for _ in range(K)]
    return w


@pytest.fixture(scope="module")
def world(pr):
    return _circuit(pr)


@pytest.fixture()
def plain_ctx(ps_api):
    """A fresh context whose provers build no window tables."""
    c = ps_api.Context(0)
    c.set_tables(False)
    yield c
    c.close()


def _abc(p):
    return (p.A, p.B, p.C)


def test_groth16_batch_over_the_key_tables(ps_api, ctx, plain_ctx, pr, world):
    w = world
    q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    tr, _ = ps_api.NewGroth16TrustedSetup(q, *w.tox[:5])
    want = [_abc(ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(ctx, w.sols[j]), w.rs[j], w.ss[j])) for j in range(K)]
    try:
        ctx.set_batch_table(2)
        got = ps_api.Groth16ProveBatch(tr, q, ps_api.Poly.upload(ctx, w.flat), w.rs, w.ss)
        info = ctx.last_msm_info()
    finally:
        ctx.set_batch_table(0)
    assert [_abc(p) for p in got] == want
    assert info["window_table"] == 1, info
    # no tables at all: the plain route, the same bytes
    q2 = ps_api.QAP(plain_ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    tr2, _ = ps_api.NewGroth16TrustedSetup(q2, *w.tox[:5])
    plain_ctx.set_batch_table(2)
    got2 = ps_api.Groth16ProveBatch(tr2, q2, ps_api.Poly.upload(plain_ctx, w.flat), w.rs, w.ss)
    assert [_abc(p) for p in got2] == want
    assert plain_ctx.last_msm_info()["window_table"] == 0


def _bits(pr):
    """rs.bit_circuit(64) with K witnesses: the rows do not depend on the seed, only the bits do."""
    from oracle import restate as rs

    w = _World()
    made = [rs.bit_circuit(64, seed=11 + j) for j in range(K)]
    w.c = made[0][0]
    for c, _ in made[1:]:
        assert (c.nbVars, c.nbIO, c.left, c.right, c.out) == (w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.sols = [sol for _, sol in made]
    assert len({tuple(s) for s in w.sols}) == K
    w.flat = [v for s in w.sols for v in s]
    rng = pr.SplitMix64(SEED + 64)
    w.tox = [rng.fr() for _ in range(8)]
    return w


@pytest.mark.parametrize("circuit,tabled", [("synthetic", 0), ("bits", 1)])
def test_phgr13_batch_over_the_key_tables(ps_api, ctx, plain_ctx, pr, world, circuit, tabled):
    w = world if circuit == "synthetic" else _bits(pr)
    fields = lambda p: tuple(getattr(p, f) for f in ps_api.PHGR13Proof.FIELDS)
    q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *w.tox)
    want = [fields(ps_api.PHGR13Prove(ek, q, ps_api.Poly.upload(ctx, w.sols[j]))) for j in range(K)]
    try:
        ctx.set_batch_table(2)
        got = ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, w.flat), K)
        info = ctx.last_msm_info()
    finally:
        ctx.set_batch_table(0)
    assert [fields(p) for p in got] == want
    assert info["window_table"] == tabled, info
    assert ek.lgsi.table_window > 0 and (ek.vas.table_window > 0) == bool(tabled)
    q2 = ps_api.QAP(plain_ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    ek2, _ = ps_api.NewPHGR13TrustedSetup(q2, *w.tox)
    plain_ctx.set_batch_table(2)
    got2 = ps_api.PHGR13ProveBatch(ek2, q2, ps_api.Poly.upload(plain_ctx, w.flat), K)
    assert [fields(p) for p in got2] == want
    assert plain_ctx.last_msm_info()["window_table"] == 0 and ek2.lgsi.table_window == 0
