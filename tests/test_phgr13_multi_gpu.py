"""GPU: PHGR13Prove over index ranges -- ps_phgr13_prove_multi (the devices of one process, each holding only its ranges of the
evaluation key; here `ndev` contexts on the one GPU) and ps_phgr13_prove_shard (one rank's share over the whole key).  Both
give the bytes of the unsharded prover and of the oracle's restatement of pinochio.go:207-254, with the monomial key and
with the key that carries gsi's Lagrange form (lgsi); wrong ranges, mixed key forms and wrong groups are refused; a witness
that does not satisfy the QAP is "apocalypse" and leaves nothing pending on the contexts."""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x706C6179736E61726B & 0xFFFFFFFFFFFFFFFF
FIELDS = ("vs", "ws", "ys", "vas", "was", "yas", "gsi", "vbs", "wbs", "ybs")


@pytest.fixture(scope="module")
def pool(ps_api, ctx):
    """Eight contexts on the one GPU (the session context first), reused by every test: a proof after an earlier one --
    refused or not -- on the same contexts is part of what is checked."""
    extra = [ps_api.Context(0) for _ in range(7)]
    yield [ctx] + extra
    for cx in extra:
        cx.close()


def _circuit(rs, n):
    # nbIO = nbVars - 3: the non-IO part (what the solution sums run over) is nearly every variable (tests/test_scale_gpu.py)
    c, sol = rs.synthetic_circuit(n)
    return rs.SparseR1CS(c.nbVars, c.nbVars - 3, c.left, c.right, c.out), sol


def _csr(c):
    """The three matrices as numpy CSR triples, built once and handed to every context (QAP.from_csr)."""
    import numpy as np

    out = []
    for rows in (c.left, c.right, c.out):
        ptr, col, val = [0], [], []
        for r in rows:
            for j, v in r:
                if v != 0:
                    col.append(j)
                    val.append(v)
            ptr.append(len(col))
        out.append((np.asarray(ptr, np.uint32), np.asarray(col or [0], np.uint32), np.asarray(val or [0], np.int64)))
    return out


def _qap(ps_api, cx, c, csr):
    return ps_api.QAP.from_csr(cx, c.nbVars, c.nbIO, *csr)


def _group(ps_api, f):
    return ps_api.G2 if f == "ws" else ps_api.G1


def _whole_key(ps_api, cx, raw):
    return ps_api.PHGR13EvalKey(**{f: ps_api.Points.upload(cx, _group(ps_api, f), b) for f, b in raw.items()})


def _local_key(ps_api, cx, raw, d, ndev):
    """Device d's index ranges of every array of the key (raw: affine bytes of the whole arrays, lgsi included if present)."""
    from playsnark_amd.dist import shard_range

    fields = {}
    for f, b in raw.items():
        nb = 192 if f == "ws" else 96
        first, cnt = shard_range(len(b) // nb, d, ndev)
        fields[f] = ps_api.Points.upload(cx, _group(ps_api, f), b[first * nb:(first + cnt) * nb])
    return ps_api.PHGR13EvalKey(**fields)


def _with_lgsi(ps_api, ctx, q, raw):
    """The raw key plus lgsi, gsi's Lagrange form on the nodes n+1..2n-1 computed from gsi alone (PHGR13EvalKey.with_lagrange)."""
    lg = ps_api.Points.upload(ctx, ps_api.G1, raw["gsi"]).to_lagrange(q, 1)
    return dict(raw, lgsi=lg.download())


def _devices(ps_api, pool, c, csr, sol_raw, raw, ndev):
    return [(_local_key(ps_api, cx, raw, d, ndev), _qap(ps_api, cx, c, csr), ps_api.Poly.upload(cx, sol_raw))
            for d, cx in enumerate(pool[:ndev])]


def _fold(ps_api, parts):
    out = {}
    for f in ps_api.PHGR13Proof.FIELDS:
        out[f] = ps_api.points_sum(ps_api.G2 if f == "wss" else ps_api.G1, b"".join(getattr(p, f) for p in parts))
    return out


def _same(ps_api, got, want):
    for f in ps_api.PHGR13Proof.FIELDS:
        g = got[f] if isinstance(got, dict) else getattr(got, f)
        assert g == getattr(want, f), f


def _sol_bytes(sol):
    return b"".join(int(v).to_bytes(32, "big") for v in sol)


@pytest.mark.parametrize("lagrange", [False, True], ids=["monomial", "lgsi"])
@pytest.mark.parametrize("ndev", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("n", [41, 53])
def test_multi_equals_the_unsharded_prover_and_the_oracle(ps_api, ctx, pool, pr, n, ndev, lagrange):
    """ps_phgr13_prove_multi over rank-local keys == ps_phgr13_prove over the whole key == the oracle, all eight elements."""
    from oracle import restate as rs

    rng = pr.SplitMix64(SEED + 7000 + 16 * n + ndev)
    c, sol = _circuit(rs, n)
    setup = rs.phgr13_setup(c, *[rng.fr() for _ in range(8)])
    want = rs.phgr13_prove(setup.EK, c, sol, fast=True)
    csr = _csr(c)
    q = _qap(ps_api, ctx, c, csr)
    raw = {f: getattr(setup.EK, f) for f in FIELDS}
    if lagrange:
        raw = _with_lgsi(ps_api, ctx, q, raw)
    sol_raw = _sol_bytes(sol)
    single = ps_api.PHGR13Prove(_whole_key(ps_api, ctx, raw), q, ps_api.Poly.upload(ctx, sol_raw))
    _same(ps_api, single, want)
    devices = _devices(ps_api, pool, c, csr, sol_raw, raw, ndev)
    _same(ps_api, ps_api.PHGR13ProveMulti(devices), want)
    _same(ps_api, ps_api.PHGR13ProveMulti(devices), want)  # again, on the same contexts (warm: no allocation)
    for cx in pool[:ndev]:
        ms = cx.last_prove_phase_ms()
        assert all(v >= 0 for v in ms.values()), ms


@pytest.mark.parametrize("lagrange", [False, True], ids=["monomial", "lgsi"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [3, 53])
def test_shards_fold_to_the_proof(ps_api, ctx, pr, n, world, lagrange):
    """ps_phgr13_prove_shard: the element-wise sum of the ranks' parts is ps_phgr13_prove's proof.  n = 3 has two values of
    h and two non-IO variables: with world 3 and 8 some ranks have empty ranges (identity parts)."""
    from oracle import restate as rs

    rng = pr.SplitMix64(SEED + 7100 + 16 * n + world)
    c, sol = _circuit(rs, n)
    setup = rs.phgr13_setup(c, *[rng.fr() for _ in range(8)])
    want = rs.phgr13_prove(setup.EK, c, sol, fast=n > 16)
    q = _qap(ps_api, ctx, c, _csr(c))
    raw = {f: getattr(setup.EK, f) for f in FIELDS}
    if lagrange:
        raw = _with_lgsi(ps_api, ctx, q, raw)
    ek = _whole_key(ps_api, ctx, raw)
    dsol = ps_api.Poly.upload(ctx, _sol_bytes(sol))
    _same(ps_api, ps_api.PHGR13Prove(ek, q, dsol), want)
    parts = [ps_api.PHGR13ProveShard(ek, q, dsol, g, world) for g in range(world)]
    _same(ps_api, _fold(ps_api, parts), want)
    if world > n - 1:
        ident = b"\x40" + bytes(95)  # the identity's encoding (zero.Clone(), algebra.go:353)
        assert any(p.hs == ident for p in parts)
    with pytest.raises(ps_api.PlaysnarkError):
        ps_api.PHGR13ProveShard(ek, q, dsol, world, world)


@pytest.fixture(scope="module")
def whole41(ps_api, ctx, pr):
    """n = 41 on the session context: circuit, QAP, the raw key with lgsi, the solution and the oracle's proof."""
    from oracle import restate as rs

    rng = pr.SplitMix64(SEED + 7150)
    c, sol = _circuit(rs, 41)
    setup = rs.phgr13_setup(c, *[rng.fr() for _ in range(8)])
    q = _qap(ps_api, ctx, c, _csr(c))
    raw = _with_lgsi(ps_api, ctx, q, {f: getattr(setup.EK, f) for f in FIELDS})
    return q, raw, sol, rs.phgr13_prove(setup.EK, c, sol, fast=True)


@pytest.mark.parametrize("lagrange", [False, True], ids=["monomial", "lgsi"])
@pytest.mark.parametrize("n", [3, 41])
def test_the_unsharded_prover_is_rank_0_of_1(ps_api, ctx, pr, whole41, n, lagrange):
    """ps_phgr13_prove and ps_phgr13_prove_shard(rank 0, world 1) give identical bytes (the oracle's), element by element,
    not folded: with two values of h and two non-IO variables (n = 3) and with 40 (n = 41)."""
    from oracle import restate as rs

    if n == 41:
        q, raw, sol, want = whole41
    else:
        rng = pr.SplitMix64(SEED + 7160)
        c, sol = _circuit(rs, n)
        setup = rs.phgr13_setup(c, *[rng.fr() for _ in range(8)])
        want = rs.phgr13_prove(setup.EK, c, sol, fast=False)
        q = _qap(ps_api, ctx, c, _csr(c))
        raw = _with_lgsi(ps_api, ctx, q, {f: getattr(setup.EK, f) for f in FIELDS})
    ek = _whole_key(ps_api, ctx, raw if lagrange else {f: raw[f] for f in FIELDS})
    dsol = ps_api.Poly.upload(ctx, _sol_bytes(sol))
    single = ps_api.PHGR13Prove(ek, q, dsol)
    shard = ps_api.PHGR13ProveShard(ek, q, dsol, 0, 1)
    _same(ps_api, single, want)
    _same(ps_api, shard, want)


def test_unsharded_apocalypse_then_a_proof_on_the_same_context(ps_api, ctx, pr, whole41):
    """ps_phgr13_prove with a witness that violates a gate is "apocalypse"; the proof right after it on the same context is
    the oracle's, and no sum is left pending (ps_msm refuses a context with pending sums)."""
    q, raw, sol, want = whole41
    ek = _whole_key(ps_api, ctx, raw)
    bad = list(sol)
    bad[5] = (bad[5] + 1) % pr.R
    with pytest.raises(ps_api.Apocalypse):
        ps_api.PHGR13Prove(ek, q, ps_api.Poly.upload(ctx, _sol_bytes(bad)))
    dsol = ps_api.Poly.upload(ctx, _sol_bytes(sol))
    _same(ps_api, ps_api.PHGR13Prove(ek, q, dsol), want)
    with pytest.raises(ps_api.PlaysnarkError, match="nothing pending"):
        ps_api.msm_finish(ctx, ps_api.G1)
    rng = pr.SplitMix64(SEED + 7170)
    h = ps_api.Poly.upload(ctx, [rng.fr() for _ in range(len(ek.gsi))])
    assert len(h.BlindEval(ek.gsi)) == 96


def test_refusals_and_recovery(ps_api, ctx, pool, pr):
    """Wrong ranges (LengthMismatch, naming the device), lgsi on some devices only and a G2 array where a G1 one belongs
    (PS_ERR_ARG), an unsatisfied witness ("apocalypse") from both entries -- and right after each, a correct proof on the
    same contexts: no sum was left pending, no device was left waiting for h."""
    from oracle import restate as rs
    from playsnark_amd import _lib

    rng = pr.SplitMix64(SEED + 7200)
    c, sol = _circuit(rs, 41)
    setup = rs.phgr13_setup(c, *[rng.fr() for _ in range(8)])
    want = rs.phgr13_prove(setup.EK, c, sol, fast=True)
    csr = _csr(c)
    q = _qap(ps_api, ctx, c, csr)
    raw = {f: getattr(setup.EK, f) for f in FIELDS}
    lraw = _with_lgsi(ps_api, ctx, q, raw)
    ndev = 3  # 40 values of h over 3 devices: 14, 13, 13
    sol_raw = _sol_bytes(sol)
    devices = _devices(ps_api, pool, c, csr, sol_raw, raw, ndev)
    ldevices = _devices(ps_api, pool, c, csr, sol_raw, lraw, ndev)

    # devices 0 and 1 hold each other's ranges (the lengths still add up: the device that does not hold its range is named)
    swapped = [(devices[1][0], devices[0][1], devices[0][2]), (devices[0][0], devices[1][1], devices[1][2]), devices[2]]
    with pytest.raises(ps_api.LengthMismatch, match="device 0"):
        ps_api.PHGR13ProveMulti(swapped)
    wrong = devices[:2] + [(devices[0][0], devices[2][1], devices[2][2])]  # device 2 holds device 0's ranges
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.PHGR13ProveMulti(wrong)
    _same(ps_api, ps_api.PHGR13ProveMulti(devices), want)

    mixed = ldevices[:2] + devices[2:]
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.PHGR13ProveMulti(mixed)
    assert e.value.code == _lib.PS_ERR_ARG
    _same(ps_api, ps_api.PHGR13ProveMulti(ldevices), want)

    k1 = devices[1][0]
    swapped = ps_api.PHGR13EvalKey(**{f: (k1.ws if f == "vs" else getattr(k1, f)) for f in FIELDS})
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.PHGR13ProveMulti([devices[0], (swapped, devices[1][1], devices[1][2]), devices[2]])
    assert e.value.code == _lib.PS_ERR_ARG
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.PHGR13ProveMulti([])
    assert e.value.code == _lib.PS_ERR_ARG

    bad = list(sol)
    bad[5] = (bad[5] + 1) % pr.R
    bad_raw = _sol_bytes(bad)
    for devs in (devices, ldevices):
        with pytest.raises(ps_api.Apocalypse):
            ps_api.PHGR13ProveMulti([(k, qq, ps_api.Poly.upload(qq.ctx, bad_raw)) for k, qq, _ in devs])
        _same(ps_api, ps_api.PHGR13ProveMulti(devs), want)
    ek = _whole_key(ps_api, ctx, lraw)
    with pytest.raises(ps_api.Apocalypse):
        ps_api.PHGR13ProveShard(ek, q, ps_api.Poly.upload(ctx, bad_raw), 1, 3)
    dsol = ps_api.Poly.upload(ctx, sol_raw)
    _same(ps_api, _fold(ps_api, [ps_api.PHGR13ProveShard(ek, q, dsol, g, 3) for g in range(3)]), want)


@pytest.fixture(scope="module")
def key16(ps_api, ctx, pr):
    """2^16 constraints: the key made on the device (NewPHGR13TrustedSetup, with lgsi), its arrays as bytes, and the
    unsharded proofs over both key forms."""
    from oracle import restate as rs

    rng = pr.SplitMix64(SEED + 7300)
    c, sol = _circuit(rs, 1 << 16)
    csr = _csr(c)
    q = _qap(ps_api, ctx, c, csr)
    sol_raw = _sol_bytes(sol)
    dsol = ps_api.Poly.upload(ctx, sol_raw)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    raw = {f: getattr(ek, f).download() for f in FIELDS + ("lgsi",)}
    want_lag = ps_api.PHGR13Prove(ek, q, dsol)
    want_mono = ps_api.PHGR13Prove(ek.monomial_only(), q, dsol)
    _same(ps_api, {f: getattr(want_lag, f) for f in ps_api.PHGR13Proof.FIELDS}, want_mono)
    del ek
    return c, csr, sol_raw, raw, want_mono


@pytest.mark.parametrize("ndev", [2, 3, 8])
def test_multi_at_2p16(ps_api, pool, key16, ndev):
    c, csr, sol_raw, raw, want = key16
    mono = {f: b for f, b in raw.items() if f != "lgsi"}
    for key in (mono, raw):
        devices = _devices(ps_api, pool, c, csr, sol_raw, key, ndev)
        _same(ps_api, ps_api.PHGR13ProveMulti(devices), want)
        del devices


def test_multi_at_2p20_eight_devices_verifies(ps_api, ctx, pool, pr):
    """BASELINE config #5 shape: 2^20 constraints, eight rank-local keys (here eight contexts on the one GPU) of the
    Lagrange-form key NewPHGR13TrustedSetup makes; equal to ps_phgr13_prove over the whole key, and PHGR13Verify accepts."""
    import time

    from oracle import restate as rs

    t0 = time.time()
    rng = pr.SplitMix64(SEED + 7400)
    c, sol = _circuit(rs, 1 << 20)
    diff = c.nbVars - c.nbIO
    csr = _csr(c)
    sol_raw = _sol_bytes(sol)
    del sol
    q = _qap(ps_api, ctx, c, csr)
    dsol = ps_api.Poly.upload(ctx, sol_raw)
    ek, vk = ps_api.NewPHGR13TrustedSetup(q, *[rng.fr() for _ in range(8)])
    want = ps_api.PHGR13Prove(ek, q, dsol)
    raw = {f: getattr(ek, f).download() for f in FIELDS + ("lgsi",)}
    io_raw = {f: getattr(vk, f).download(0, diff) for f in ("vs", "ws", "ys")}
    fixed = vk.fixed_points()
    del ek, vk  # the whole key goes once its ranges are known
    ctx.sync()
    print(f"[2^20] circuit, key and unsharded proof: {time.time() - t0:.1f} s", flush=True)
    devices = _devices(ps_api, pool, c, csr, sol_raw, raw, 8)
    del raw
    print(f"[2^20] rank-local keys on 8 contexts: {time.time() - t0:.1f} s", flush=True)
    got = ps_api.PHGR13ProveMulti(devices)
    _same(ps_api, got, want)
    io_arrays = [ps_api.Points.upload(ctx, ps_api.G2 if f == "ws" else ps_api.G1, io_raw[f]) for f in ("vs", "ws", "ys")]
    assert ps_api.PHGR13Verify(ctx, fixed, *io_arrays, got, ps_api.Poly.upload(ctx, sol_raw[: 32 * diff]))
    print(f"[2^20] multi proof and verification: {time.time() - t0:.1f} s", flush=True)
