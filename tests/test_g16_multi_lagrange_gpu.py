"""GPU: Groth16Prove over rank-local LAGRANGE-form keys -- ps_groth16_prove_multi (the devices of one process, each holding
only its ranges of lxi / lxi2 / lxi_t / NioLP; here `ndev` contexts on the one GPU) and ps_groth16_prove_local (one rank's share,
one process per GPU).  Everything is compared byte for byte with the unsharded prover over the whole key and with the oracle's
restatement of groth16.go:122-211: there is no tolerance anywhere in this feature.  Both settings of PS_G16_MULTI_HSPLIT (the
three convolutions of the values route on devices 0, 1, 2, or all on device 0) and both forms of C of the unsharded prover
(PS_G16_B1_MIN_N) run; wrong ranges, mixed key forms, wrong groups, a context used twice and a pending sum are refused; a
witness that does not satisfy the QAP is "apocalypse" whichever device owns the failing gate, and leaves nothing pending."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_cases as qc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x706C6179736E61726B & 0xFFFFFFFFFFFFFFFF
LAG = ("LXi", "LXi2", "LXiT")
MONO = ("Xi", "Xi2", "XiT")
FIXED = ("Alpha", "Beta", "Delta", "Beta2", "Delta2")


def _contexts(ps_api, count, **env):
    """Contexts created under the given environment (the knobs are read by ps_ctx_create and by nothing else)."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return [ps_api.Context(0) for _ in range(count)]


@pytest.fixture(scope="module")
def pools(ps_api):
    """Eight contexts per value of PS_G16_MULTI_HSPLIT, reused by every test: a proof after an earlier one -- refused or not --
    on the same contexts is part of what is checked."""
    p = {h: _contexts(ps_api, 8, PS_G16_MULTI_HSPLIT=h) for h in ("1", "0")}
    yield p
    for cxs in p.values():
        for cx in cxs:
            cx.close()


@pytest.fixture(scope="module")
def single(ps_api):
    """Contexts for the unsharded reference proof, one per form of C (groth16_prove_impl: the single sum, the split form)."""
    p = {m: _contexts(ps_api, 1, PS_G16_B1_MIN_N=m)[0] for m in ("2", "1000000000")}
    yield p
    for cx in p.values():
        cx.close()


def _csr(c):
    return [qc.csr_of(rows) for rows in (c.left, c.right, c.out)]


def _qap(ps_api, cx, c, csr):
    return ps_api.QAP.from_csr(cx, c.nbVars, c.nbIO, *csr)


def _sol_bytes(sol):
    return b"".join(int(v).to_bytes(32, "big") for v in sol)


def _raw_key(ps_api, q, tox):
    """The key NewGroth16TrustedSetup makes on the device (both forms; pinned to the oracle's by tests/test_prover_gpu.py) as bytes."""
    tr, vk = ps_api.NewGroth16TrustedSetup(q, *tox)
    raw = {f: getattr(tr, f) for f in FIXED}
    raw.update({f: getattr(tr, f).download() for f in MONO + LAG + ("NioLP",)})
    return tr, vk, raw


def _local_key(ps_api, cx, raw, d, ndev, forms=LAG):
    """Device d's index ranges of the arrays in `forms` (and of NioLP); the other form's members are None."""
    from playsnark_amd.dist import shard_range

    def part(f):
        if f not in forms + ("NioLP",):
            return None
        nb = 192 if f.endswith("Xi2") else 96
        first, cnt = shard_range(len(raw[f]) // nb, d, ndev)
        return ps_api.Points.upload(cx, ps_api.G2 if nb == 192 else ps_api.G1, raw[f][first * nb:(first + cnt) * nb])

    return ps_api.Groth16Setup(*[raw[f] for f in FIXED], part("Xi"), part("Xi2"), part("NioLP"), part("XiT"),
                               part("LXi"), part("LXi2"), part("LXiT"))


def _devices(ps_api, cxs, c, csr, sol, raw, ndev, forms=LAG):
    up = (lambda cx: ps_api.Poly.upload(cx, sol)) if isinstance(sol, bytes) else (lambda cx: ps_api.Poly.from_values(cx, sol))
    return [(_local_key(ps_api, cx, raw, d, ndev, forms), _qap(ps_api, cx, c, csr), up(cx)) for d, cx in enumerate(cxs[:ndev])]


def _abc(p):
    return (p.A, p.B, p.C) if hasattr(p, "A") else tuple(p)


def _fold(ps_api, parts):
    return (ps_api.points_sum(ps_api.G1, b"".join(p[0] for p in parts)), ps_api.points_sum(ps_api.G2, b"".join(p[1] for p in parts)),
            ps_api.points_sum(ps_api.G1, b"".join(p[2] for p in parts)))


def _case(rs, pr, n, io_all, seed):
    c, sol = rs.synthetic_circuit(n)
    if io_all:  # nbIO = nbVars - 3: NioLP is nearly every variable; otherwise nbIO = 3 and NioLP has three points
        c = rs.SparseR1CS(c.nbVars, c.nbVars - 3, c.left, c.right, c.out)
    rng = pr.SplitMix64(SEED + seed)
    return c, sol, [rng.fr() for _ in range(5)], rng.fr(), rng.fr()


@pytest.mark.parametrize("io_all", [True, False], ids=["nio-all", "nio-3"])
@pytest.mark.parametrize("ndev", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("n", [3, 41, 53])
def test_multi_over_lagrange_only_keys_equals_the_unsharded_prover_and_the_oracle(ps_api, pools, single, pr, n, ndev, io_all):
    """Lagrange-ONLY rank-local keys (the monomial members None; the parent commit refused them: PS_ERR_ARG "NULL handle").
    n = 3 over 8 devices leaves most devices with empty ranges: identities, not errors."""
    from oracle import restate as rs

    c, sol, tox, r, s = _case(rs, pr, n, io_all, 9000 + 64 * n + 2 * ndev + io_all)
    want = _abc(rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s, fast=n > 16))
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    raw = None
    for min_n, cx in single.items():  # the unsharded proof in the single and in the split form of C
        q = _qap(ps_api, cx, c, csr)
        tr, _, raw = _raw_key(ps_api, q, tox)
        assert _abc(ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(cx, sol_raw), r, s)) == want, min_n
        assert _abc(ps_api.Groth16Prove(tr.lagrange_only(), q, ps_api.Poly.upload(cx, sol_raw), r, s)) == want, min_n
    for hsplit, cxs in pools.items():
        devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, ndev)
        assert all(k.Xi is None and k.Xi2 is None and k.XiT is None for k, _, _ in devices)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, hsplit
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, hsplit  # again on the same contexts (warm: no allocation)
        for cx in cxs[:ndev]:
            ms = cx.last_prove_phase_ms()
            assert all(v >= 0 for v in ms.values()), ms
    # keys that carry both forms on every device take the same route: same bytes
    both = _devices(ps_api, pools["1"], c, csr, sol_raw, raw, ndev, forms=LAG + MONO)
    assert _abc(ps_api.Groth16ProveMulti(both, r, s)) == want


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [3, 53])
def test_local_shares_fold_to_the_proof(ps_api, pools, pr, n, world):
    """ps_groth16_prove_local (missing on the parent commit): the element-wise sum of the ranks' parts is the unsharded proof;
    the same through ShardedGroth16Local with simulated ranks."""
    from oracle import restate as rs
    from playsnark_amd.dist import ShardedGroth16, ShardedGroth16Local

    c, sol, tox, r, s = _case(rs, pr, n, True, 9500 + 16 * n + world)
    want = _abc(rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s, fast=n > 16))
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    cxs = pools["1"]
    q0 = _qap(ps_api, cxs[0], c, csr)
    tr, _, raw = _raw_key(ps_api, q0, tox)
    assert _abc(ps_api.Groth16Prove(tr, q0, ps_api.Poly.upload(cxs[0], sol_raw), r, s)) == want
    devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, world)
    parts = [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, world) for g, (k, q, dsol) in enumerate(devices)]
    assert _fold(ps_api, parts) == want
    assert _fold(ps_api, [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, world) for g, (k, q, dsol) in enumerate(devices)]) == want
    for cx in cxs[:world]:
        assert all(v >= 0 for v in cx.last_prove_phase_ms().values())
    if world > n:
        assert any(p[0] == b"\x40" + bytes(95) for p in parts)  # an empty range: the identity
    parts = [ShardedGroth16Local(q.ctx, None, world, g).partials(k, q, dsol, r, s) for g, (k, q, dsol) in enumerate(devices)]
    assert _abc(ShardedGroth16.fold(parts, r, s)) == want
    # refusals: a rank outside the world, ranges of another world, a key without its Lagrange arrays
    from playsnark_amd import _lib

    k, q, dsol = devices[0]
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16ProveLocal(k, q, dsol, r, s, world, world)
    assert e.value.code == _lib.PS_ERR_ARG
    if n > 3:
        with pytest.raises(ps_api.LengthMismatch):
            ps_api.Groth16ProveLocal(_local_key(ps_api, q.ctx, raw, 0, world + 1), q, dsol, r, s, 0, world)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16ProveLocal(_local_key(ps_api, q.ctx, raw, 0, world, forms=MONO), q, dsol, r, s, 0, world)
    assert e.value.code == _lib.PS_ERR_ARG
    assert _abc(ps_api.Groth16ProveLocal(*devices[0], r, s, 0, world)) == parts[0]


@pytest.mark.parametrize("ndev", [2, 3])
@pytest.mark.parametrize("kind,witness", [("int64_min", "minus_one"), ("int64_max", "minus_one"), ("random", "random")])
def test_dense_rows_inside_and_outside_every_range(ps_api, pools, pr, kind, witness, ndev):
    """Rows of 512 (the last length the per-row kernel owns), 513 and more than 1025 entries, with int64-extreme coefficients
    and witnesses of r - 1, spread so that every device has workgroup-summed rows inside its range and outside it."""
    from oracle import restate as rs

    lengths = (513, 512, 1027, 3, 1100, 513, 40, 2049, 1, 512, 514, 1026)  # long (> 512) rows: 0, 2, 4, 5, 7, 10, 11
    b = qc.dense_circuit(kind, witness, 12, lengths=lengths, inputs=1024, seed=11)
    c = b.circuit(nb_io=b.nvars - 3)
    sol = b.sol
    rng = pr.SplitMix64(SEED + 9700 + ndev)
    tox, r, s = [rng.fr() for _ in range(5)], rng.fr(), rng.fr()
    want = _abc(rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s, fast=True))
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    for hsplit, cxs in pools.items():
        q0 = _qap(ps_api, cxs[0], c, csr)
        tr, _, raw = _raw_key(ps_api, q0, tox)
        assert _abc(ps_api.Groth16Prove(tr, q0, ps_api.Poly.upload(cxs[0], sol_raw), r, s)) == want
        devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, ndev)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, hsplit
        parts = [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, ndev) for g, (k, q, dsol) in enumerate(devices)]
        assert _fold(ps_api, parts) == want, hsplit
        # a dense row that is wrong in the LAST device's range only
        bad = list(sol)
        bad[c.out[11][0][0]] = (bad[c.out[11][0][0]] + 1) % pr.R
        with pytest.raises(ps_api.Apocalypse):
            ps_api.Groth16ProveMulti([(k, q, ps_api.Poly.upload(q.ctx, _sol_bytes(bad))) for k, q, _ in devices], r, s)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, hsplit


def test_int64_witness_with_negative_values(ps_api, pools, pr):
    """A witness uploaded as int64 (Poly.from_values, negative values included) keeps the short-scalar plan of its NioLP sum."""
    from oracle import restate as rs

    rng = pr.SplitMix64(SEED + 9800)
    c0, sol = rs.synthetic_circuit(8, x0=pr.R - 3)  # x = -3: every wire is a small signed integer
    wit = [v if v < pr.R // 2 else v - pr.R for v in sol]
    assert min(wit) < 0 and max(abs(v) for v in wit) < 1 << 62
    for nb_io in (3, c0.nbVars - 3):
        c = rs.SparseR1CS(c0.nbVars, nb_io, c0.left, c0.right, c0.out)
        tox, r, s = [rng.fr() for _ in range(5)], rng.fr(), rng.fr()
        want = _abc(rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s))
        csr = _csr(c)
        for hsplit, cxs in pools.items():
            _, _, raw = _raw_key(ps_api, _qap(ps_api, cxs[0], c, csr), tox)
            for ndev in (2, 3):
                devices = _devices(ps_api, cxs, c, csr, wit, raw, ndev)
                assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, (nb_io, hsplit, ndev)
                parts = [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, ndev) for g, (k, q, dsol) in enumerate(devices)]
                assert _fold(ps_api, parts) == want, (nb_io, hsplit, ndev)


def test_refusals_apocalypse_and_recovery(ps_api, pools, pr):
    """Mixed key forms, a wrong range (LengthMismatch naming the device), a G2 array where a G1 one belongs, a context used
    twice, a sum pending on a context; an off-by-one witness whose failing gates lie in device 0's range only, and one whose
    failing gate lies in the last device's range only -- and right after each, a correct proof on the SAME contexts."""
    from oracle import restate as rs
    from playsnark_amd import _lib

    n, ndev = 41, 3  # rows 0..13 | 14..27 | 28..40
    c, sol, tox, r, s = _case(rs, pr, n, True, 9900)
    want = _abc(rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s, fast=True))
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    for hsplit, cxs in pools.items():
        _, _, raw = _raw_key(ps_api, _qap(ps_api, cxs[0], c, csr), tox)
        devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, ndev)
        mono = _devices(ps_api, cxs, c, csr, sol_raw, raw, ndev, forms=MONO)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want
        assert _abc(ps_api.Groth16ProveMulti(mono, r, s)) == want  # the monomial route, as before

        with pytest.raises(ps_api.PlaysnarkError, match="on every device or on none") as e:
            ps_api.Groth16ProveMulti(devices[:2] + mono[2:], r, s)
        assert e.value.code == _lib.PS_ERR_ARG
        swapped = [(devices[1][0], devices[0][1], devices[0][2]), (devices[0][0], devices[1][1], devices[1][2]), devices[2]]
        with pytest.raises(ps_api.LengthMismatch, match="device 0"):
            ps_api.Groth16ProveMulti(swapped, r, s)
        with pytest.raises(ps_api.LengthMismatch):
            ps_api.Groth16ProveMulti(devices[:2] + [(devices[0][0], devices[2][1], devices[2][2])], r, s)
        k1 = devices[1][0]
        g2_for_g1 = ps_api.Groth16Setup(*[raw[f] for f in FIXED], None, None, k1.NioLP, None, k1.LXi2, k1.LXi2, k1.LXiT)
        with pytest.raises(ps_api.PlaysnarkError, match="wrong group") as e:
            ps_api.Groth16ProveMulti([devices[0], (g2_for_g1, devices[1][1], devices[1][2]), devices[2]], r, s)
        assert e.value.code == _lib.PS_ERR_ARG
        twice = _devices(ps_api, [cxs[0], cxs[1], cxs[0]], c, csr, sol_raw, raw, ndev)
        with pytest.raises(ps_api.PlaysnarkError, match="appears twice") as e:
            ps_api.Groth16ProveMulti(twice, r, s)
        assert e.value.code == _lib.PS_ERR_ARG
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.Groth16ProveMulti([], r, s)
        assert e.value.code == _lib.PS_ERR_ARG
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want

        # a sum left pending on device 1's context
        k, q, dsol = devices[1]
        ps_api.msm_launch(q.ctx, k.LXi, ps_api.Poly.upload(q.ctx, sol_raw[:32 * len(k.LXi)]))
        with pytest.raises(ps_api.PlaysnarkError, match="pending") as e:
            ps_api.Groth16ProveMulti(devices, r, s)
        assert e.value.code == _lib.PS_ERR_ARG
        with pytest.raises(ps_api.PlaysnarkError, match="pending"):
            ps_api.Groth16ProveLocal(k, q, dsol, r, s, 1, ndev)
        ps_api.msm_finish(q.ctx, ps_api.G1)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want

        # variable 3 is gate 0's output and gate 1's input: gates 0 and 1 fail, device 0's rows; variable 2 (OUT) is the last
        # gate's output and nothing else: gate 40 fails, the last device's rows
        for var in (3, 2):
            bad = list(sol)
            bad[var] = (bad[var] + 1) % pr.R
            vals = c.values(bad)
            failing = [j for j in range(n) if vals[0][j] * vals[1][j] % pr.R != vals[2][j]]
            assert failing == ([0, 1] if var == 3 else [n - 1])
            bad_raw = _sol_bytes(bad)
            with pytest.raises(ps_api.Apocalypse):
                ps_api.Groth16ProveMulti([(k, q, ps_api.Poly.upload(q.ctx, bad_raw)) for k, q, _ in devices], r, s)
            assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want
            for g, (k, q, _) in enumerate(devices):  # every rank of the per-process form sees it (its check covers all rows)
                with pytest.raises(ps_api.Apocalypse):
                    ps_api.Groth16ProveLocal(k, q, ps_api.Poly.upload(q.ctx, bad_raw), r, s, g, ndev)
            parts = [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, ndev) for g, (k, q, dsol) in enumerate(devices)]
            assert _fold(ps_api, parts) == want


@pytest.fixture(scope="module")
def key16(ps_api, pools, pr):
    """2^16 constraints: the key made on the device, its arrays as bytes, and the unsharded proof (pinned to the oracle at this
    size by tests/test_scale_gpu.py)."""
    from oracle import restate as rs

    c, sol, tox, r, s = _case(rs, pr, 1 << 16, True, 9990)
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    cx = pools["1"][0]
    q = _qap(ps_api, cx, c, csr)
    tr, _, raw = _raw_key(ps_api, q, tox)
    want = _abc(ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(cx, sol_raw), r, s))
    assert _abc(ps_api.Groth16Prove(tr.monomial_only(), q, ps_api.Poly.upload(cx, sol_raw), r, s)) == want
    del tr
    return c, csr, sol_raw, raw, r, s, want


@pytest.mark.parametrize("ndev", [2, 3, 8])
def test_multi_at_2p16(ps_api, pools, key16, ndev):
    c, csr, sol_raw, raw, r, s, want = key16
    for hsplit, cxs in pools.items():
        devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, ndev)
        assert _abc(ps_api.Groth16ProveMulti(devices, r, s)) == want, hsplit
        if hsplit == "1":
            parts = [ps_api.Groth16ProveLocal(k, q, dsol, r, s, g, ndev) for g, (k, q, dsol) in enumerate(devices)]
            assert _fold(ps_api, parts) == want
        del devices


def test_multi_at_2p20_eight_devices_verifies(ps_api, pools, pr):
    """2^20 constraints, eight Lagrange-only rank-local keys (eight contexts on the one GPU): equal to ps_groth16_prove over
    the whole key, and Groth16Verify accepts."""
    import time

    from oracle import restate as rs

    t0 = time.time()
    c, sol, tox, r, s = _case(rs, pr, 1 << 20, True, 9995)
    diff = c.nbVars - c.nbIO
    csr, sol_raw = _csr(c), _sol_bytes(sol)
    del sol
    cxs = pools["1"]
    q = _qap(ps_api, cxs[0], c, csr)
    tr, vk, raw = _raw_key(ps_api, q, tox)
    for f in MONO:  # the monomial arrays are not needed: Lagrange-only keys
        del raw[f]
    want = ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(cxs[0], sol_raw), r, s)
    io_raw = vk["IoLP"].download()
    gamma = vk["Gamma"]
    del tr, vk, q  # the whole key goes once its ranges are known
    cxs[0].sync()
    print(f"[2^20] circuit, key and unsharded proof: {time.time() - t0:.1f} s", flush=True)
    devices = _devices(ps_api, cxs, c, csr, sol_raw, raw, 8)
    print(f"[2^20] rank-local keys on 8 contexts: {time.time() - t0:.1f} s", flush=True)
    got = ps_api.Groth16ProveMulti(devices, r, s)
    assert _abc(got) == _abc(want)
    print("[2^20] phases per context (ms):", [cx.last_prove_phase_ms() for cx in cxs], flush=True)
    io = ps_api.Points.upload(cxs[0], ps_api.G1, io_raw)
    assert ps_api.Groth16Verify(cxs[0], raw["Alpha"], raw["Beta2"], gamma, raw["Delta2"], io, got, ps_api.Poly.upload(cxs[0], sol_raw[:32 * diff]))
    print(f"[2^20] multi proof and verification: {time.time() - t0:.1f} s", flush=True)
