"""GPU: ps_groth16_prove_batch -- K witnesses of one circuit under one Lagrange-form key in one call (csrc/prove_batch.inc)
-- byte for byte against K calls of Groth16Prove, against the oracle's restatement of groth16.go:122-211, and through
Groth16Verify.

Witnesses: rs.synthetic_circuit(n, x0=...) tiles the same gates whatever x0 is; only the wire values change.  Every case
checks that on the CPU first (the three matrices of all K circuits are equal) and then proves the K solution vectors over
the FIRST circuit's QAP and key.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x67313662617463 & 0xFFFFFFFFFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _World:
    pass


def _world(ps_api, ctx, pr, n, k, salt=0):
    """One circuit of n gates, its device key (monomial + Lagrange form) and K witnesses from K values of x0."""
    from oracle import restate as rs

    w = _World()
    rng = pr.SplitMix64(SEED + 1000 * n + k + salt)
    made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(k)]
    w.c = made[0][0]
    for c, _ in made[1:]:  # the matrices do not depend on x0
        assert (c.nbVars, c.nbIO, c.left, c.right, c.out) == (w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.sols = [sol for _, sol in made]
    assert len({tuple(s) for s in w.sols}) == k
    w.tox = [rng.fr() for _ in range(5)]
    w.rs = [rng.fr() for _ in range(k)]
    w.ss = [rng.fr() for _ in range(k)]
    assert len(set(w.rs + w.ss)) == 2 * k
    w.q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.tr, w.vk = ps_api.NewGroth16TrustedSetup(w.q, *w.tox)
    w.flat = [v for s in w.sols for v in s]
    return w


def _abc(p):
    return (p.A, p.B, p.C)


def _singles(ps_api, ctx, w, idx=None):
    idx = range(len(w.sols)) if idx is None else idx
    return {j: _abc(ps_api.Groth16Prove(w.tr, w.q, ps_api.Poly.upload(ctx, w.sols[j]), w.rs[j], w.ss[j])) for j in idx}


@pytest.mark.parametrize("n,k", [(2, 1), (7, 3), (64, 8), (300, 5)])
def test_batch_proofs_equal_single_proofs_and_verify(ps_api, ctx, co, pr, n, k):
    from oracle import restate as rs

    w = _world(ps_api, ctx, pr, n, k)
    got = ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, w.flat), w.rs, w.ss)
    assert len(got) == k
    want = _singles(ps_api, ctx, w)
    diff = w.c.nbVars - w.c.nbIO
    for j in range(k):
        assert _abc(got[j]) == want[j], (n, k, j)
        assert (got[j].R, got[j].S) == (w.rs[j], w.ss[j])
        io = ps_api.Poly.upload(ctx, w.sols[j][:diff])
        assert ps_api.Groth16Verify(ctx, w.tr.Alpha, w.tr.Beta2, w.vk["Gamma"], w.tr.Delta2, w.vk["IoLP"], got[j], io) is True, j
    if (n, k) == (7, 3):
        ref = rs.groth16_setup(w.c, *w.tox)
        for j in range(k):
            o = rs.groth16_prove(ref, w.c, w.sols[j], w.rs[j], w.ss[j])
            assert _abc(got[j]) == (o.A, o.B, o.C), j
    # the key's Lagrange form alone is enough
    again = ps_api.Groth16ProveBatch(w.tr.lagrange_only(), w.q, ps_api.Poly.upload(ctx, w.flat), w.rs, w.ss)
    assert [_abc(p) for p in again] == [want[j] for j in range(k)]


def test_batch_violated_gate_flags_apocalypse_and_recovery(ps_api, ctx, co, pr):
    """Witness 1 of 3 violates a gate.  With `valid`: [1, 0, 1], proof 1 all zero bytes, proofs 0 and 2 unchanged.  Without:
    Apocalypse (qap.go:158-160), the message names witness 1, and the context proves correctly right after."""
    w = _world(ps_api, ctx, pr, 7, 3, salt=1)
    want = _singles(ps_api, ctx, w)
    bad = [list(s) for s in w.sols]
    bad[1][4] = (bad[1][4] + 1) % pr.R
    flat = [v for s in bad for v in s]
    proofs, flags = ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, flat), w.rs, w.ss, valid=True)
    assert flags == [1, 0, 1]
    assert _abc(proofs[1]) == (bytes(96), bytes(192), bytes(96))
    assert _abc(proofs[0]) == want[0] and _abc(proofs[2]) == want[2]
    with pytest.raises(ps_api.Apocalypse):
        ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, flat), w.rs, w.ss)
    assert b"witness 1 " in ps_api.lib.ps_last_error()
    good = ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, w.flat), w.rs, w.ss)
    assert [_abc(p) for p in good] == [want[j] for j in range(3)]
    proofs, flags = ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, w.flat), w.rs, w.ss, valid=True)
    assert flags == [1, 1, 1] and [_abc(p) for p in proofs] == [want[j] for j in range(3)]


def test_batch_needs_a_lagrange_form_key_and_the_right_length(ps_api, ctx, co, pr):
    w = _world(ps_api, ctx, pr, 7, 3, salt=2)
    sols = ps_api.Poly.upload(ctx, w.flat)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16ProveBatch(w.tr.monomial_only(), w.q, sols, w.rs, w.ss)
    assert e.value.code == -5 and "ps_points_monomial_to_lagrange" in str(e.value)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, w.flat[:-1]), w.rs, w.ss)
    assert e.value.code == -5
    assert ps_api.Groth16ProveBatch(w.tr, w.q, ps_api.Poly.upload(ctx, []), [], []) == []


def test_batch_int64_witnesses_and_passes(ps_api, ctx, co, pr):
    """Witnesses uploaded as int64 (x0 = -3, -5, ..: every wire a small signed integer) give the bytes of their be32 upload;
    set_chunk(2) with K = 5 (passes of 2, 2 and 1) gives the bytes of the automatic split."""
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
    tr, _ = ps_api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
    rr, ss = [rng.fr() for _ in range(k)], [rng.fr() for _ in range(k)]
    be = ps_api.Groth16ProveBatch(tr, q, ps_api.Poly.upload(ctx, [v for s in sols for v in s]), rr, ss)
    i64 = ps_api.Groth16ProveBatch(tr, q, ps_api.Poly.from_values(ctx, [v for wt in wits for v in wt]), rr, ss)
    assert [_abc(p) for p in i64] == [_abc(p) for p in be]
    single = ps_api.Groth16Prove(tr, q, ps_api.Poly.from_values(ctx, wits[3]), rr[3], ss[3])
    assert _abc(single) == _abc(be[3])
    try:
        ctx.set_batch_chunk(2)
        chunked = ps_api.Groth16ProveBatch(tr, q, ps_api.Poly.upload(ctx, [v for s in sols for v in s]), rr, ss)
    finally:
        ctx.set_batch_chunk(0)
    assert [_abc(p) for p in chunked] == [_abc(p) for p in be]


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from oracle import pyref as pr, restate as rs
from playsnark_amd import api
n, k = 64, 3
made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(k)]
c = made[0][0]
sols = [s for _, s in made]
rng = pr.SplitMix64(12345)
ctx = api.Context(0)
q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
tr, _ = api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
rr, ss = [rng.fr() for _ in range(k)], [rng.fr() for _ in range(k)]
single = [api.Groth16Prove(tr, q, api.Poly.upload(ctx, sols[j]), rr[j], ss[j]) for j in range(k)]
assert ctx.last_prove_phase_ms()["total"] > 0
batch = api.Groth16ProveBatch(tr, q, api.Poly.upload(ctx, [v for s in sols for v in s]), rr, ss)
again = api.Groth16Prove(tr, q, api.Poly.upload(ctx, sols[1]), rr[1], ss[1])
for j in range(k):
    assert (batch[j].A, batch[j].B, batch[j].C) == (single[j].A, single[j].B, single[j].C), j
assert (again.A, again.B, again.C) == (single[1].A, single[1].B, single[1].C)
print("split-form child ok", (single[0].A + single[0].B + single[0].C).hex())
"""


def test_batch_bytes_do_not_depend_on_the_single_provers_split_form(ps_api, ctx, co, pr):
    """PS_G16_B1_MIN_N=1 in a child process makes the single prover sum B in G1 on its own and add s A + r B1 on the host (the
    split form of C); the batch always uses the unsplit layout.  Same bytes, in either order of the calls on one context --
    and the bytes of the split-form proof are those of this process's (unsplit) single prover."""
    from oracle import restate as rs

    env = dict(os.environ, PS_G16_B1_MIN_N="1")
    run = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    line = [ln for ln in run.stdout.split("\n") if ln.startswith("split-form child ok")]
    assert len(line) == 1
    c, sol = rs.synthetic_circuit(64, x0=3)
    rng = pr.SplitMix64(12345)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, _ = ps_api.NewGroth16TrustedSetup(q, *[rng.fr() for _ in range(5)])
    rr, ss = [rng.fr() for _ in range(3)], [rng.fr() for _ in range(3)]
    here = ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(ctx, sol), rr[0], ss[0])
    assert line[0].split()[-1] == (here.A + here.B + here.C).hex()
