"""GPU: a circuit's Groth16 key from a powers-of-tau string (ps_groth16_setup_from_srs), shares folded into it
(ps_groth16_crs_contribute) and the check of a fold (ps_groth16_crs_check_update).

The string is made here from fixed toxic values -- {x^i}, {alpha x^i}, {beta x^i} in Python integers, committed with
Points.from_scalars -- so that every array and fixed point of the SRS-made key can be compared, byte for byte, with the key the
toxic-waste setup NewGroth16TrustedSetup makes from the same values: with delta = gamma = 1, after one fold (d, g) and after
two (the products).  A proof under the SRS-made, contributed key verifies and (n <= 68) equals the oracle's proof bytes."""
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("Xi", "Xi2", "NioLP", "XiT", "LXi", "LXi2", "LXiT")
FIXED = ("Alpha", "Beta", "Delta", "Beta2", "Delta2")
SIZES = (4, 40, 68, 200)


def _toxic(pr):
    rng = pr.SplitMix64(20161016)
    return {k: rng.fr() for k in ("alpha", "beta", "x", "d", "g", "d2", "g2")}


def _circuit(n):
    from oracle import pyref, restate as rs

    if n == 4:
        c, wit = rs.toy_circuit()
        return c, [pyref.fr(v) for v in wit]
    return rs.synthetic_circuit(n)


def _srs(api, ctx, co, pr, n, tw, short=None):
    """The phase-1 string for n gates; short = name of an array to make one point too short"""
    R, x = pr.R, tw["x"]
    pw = [pow(x, i, R) for i in range(2 * n - 1)]
    cut = lambda name, v: v[:-1] if short == name else v
    commit = lambda g, v: api.Points.from_scalars(ctx, g, api.Poly.upload(ctx, v))
    return api.Groth16SRS(commit(api.G1, cut("tau_g1", pw)), commit(api.G2, cut("tau_g2", pw[:n])),
                          commit(api.G1, cut("alpha_tau_g1", [tw["alpha"] * p % R for p in pw[:n]])),
                          commit(api.G1, cut("beta_tau_g1", [tw["beta"] * p % R for p in pw[:n]])),
                          co.G2.to_b(co.G2.mul(tw["beta"])))


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


class World:
    pass


_worlds = {}


@pytest.fixture(params=SIZES)
def world(request, ps_api, ctx, co, pr):
    """Per circuit size, made once: the circuit, the SRS-made key K0 and the keys after one (K1) and two (K2) folds."""
    n = request.param
    if n not in _worlds:
        w = World()
        w.n, w.tw = n, _toxic(pr)
        w.c, w.sol = _circuit(n)
        w.q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
        w.K0 = ps_api.NewGroth16SetupFromSRS(w.q, _srs(ps_api, ctx, co, pr, n, w.tw))
        w.K1 = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d"], w.tw["g"])
        w.K2 = ps_api.Groth16Contribute(ctx, *w.K1, w.tw["d2"], w.tw["g2"])
        rng = pr.SplitMix64(n)
        w.rhos = [(rng.next() << 64 | rng.next()) or 1 for _ in range(max(w.c.nbVars, n))]
        _worlds[n] = w
    return _worlds[n]


def _trusted(ps_api, w, delta, gamma):
    return ps_api.NewGroth16TrustedSetup(w.q, w.tw["alpha"], w.tw["beta"], delta, w.tw["x"], gamma)


def test_key_from_srs_equals_the_toxic_waste_setup_at_delta_gamma_one(ps_api, world):
    _assert_same_key(world.K0, _trusted(ps_api, world, 1, 1), "delta = gamma = 1")


def test_one_and_two_folds_equal_the_setup_with_the_products(ps_api, pr, world):
    tw = world.tw
    _assert_same_key(world.K1, _trusted(ps_api, world, tw["d"], tw["g"]), "one fold")
    _assert_same_key(world.K2, _trusted(ps_api, world, tw["d"] * tw["d2"] % pr.R, tw["g"] * tw["g2"] % pr.R), "two folds")


def test_proofs_under_the_contributed_key_verify_and_equal_the_oracle(ps_api, ctx, pr, world):
    from oracle import restate as rs

    w = world
    tr, vk = w.K1
    diff = w.c.nbVars - w.c.nbIO
    sol = ps_api.Poly.upload(ctx, w.sol)
    io = ps_api.Poly.upload(ctx, w.sol[:diff])
    r, s = 0x1F2E3D4C5B6A7988, 0x0123456789ABCDEF0FEDCBA987654321
    proofs = [ps_api.Groth16Prove(form, w.q, sol, r, s) for form in (tr.lagrange_only(), tr.monomial_only())]
    assert (proofs[0].A, proofs[0].B, proofs[0].C) == (proofs[1].A, proofs[1].B, proofs[1].C)
    for p in proofs:
        assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], p, io)
    if w.n <= 68:
        ref = rs.groth16_setup(w.c, w.tw["alpha"], w.tw["beta"], w.tw["d"], w.tw["x"], w.tw["g"])
        want = rs.groth16_prove(ref, w.c, w.sol, r, s)
        assert (proofs[0].A, proofs[0].B, proofs[0].C) == (want.A, want.B, want.C)


def _with(ps_api, tr, **repl):
    f = dict(Alpha=tr.Alpha, Beta=tr.Beta, Delta=tr.Delta, Beta2=tr.Beta2, Delta2=tr.Delta2, Xi=tr.Xi, Xi2=tr.Xi2, NioLP=tr.NioLP,
             XiT=tr.XiT, LXi=tr.LXi, LXi2=tr.LXi2, LXiT=tr.LXiT)
    f.update(repl)
    return ps_api.Groth16Setup(**f)


def test_check_update_accepts_honest_folds(ps_api, ctx, world):
    w = world
    assert ps_api.Groth16CheckUpdate(ctx, w.K0, w.K1, w.rhos)
    assert ps_api.Groth16CheckUpdate(ctx, w.K1, w.K2, w.rhos)
    assert ps_api.Groth16CheckUpdate(ctx, w.K0, w.K2, w.rhos)  # two folds, checked across both
    assert ps_api.Groth16CheckUpdate(ctx, w.K0, w.K0, w.rhos)  # d = g = 1


def test_check_update_rejects_keys_no_fold_makes(ps_api, ctx, co, world):
    w = world
    tr, vk = w.K1
    # one NioLP point replaced
    raw = bytearray(tr.NioLP.download())
    raw[-96:] = co.G1.to_b(co.G1.mul(7))
    bad = _with(ps_api, tr, NioLP=ps_api.Points.upload(ctx, ps_api.G1, bytes(raw)))
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (bad, vk), w.rhos)
    # XiT scaled by another factor than NioLP
    other, _ = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d2"], w.tw["g"])
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (_with(ps_api, tr, XiT=other.XiT), vk), w.rhos)
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (_with(ps_api, tr, LXiT=other.LXiT), vk), w.rhos)
    # IoLP scaled by another factor than Gamma
    _, other_vk = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d"], w.tw["g2"])
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (tr, {"Gamma": vk["Gamma"], "IoLP": other_vk["IoLP"]}), w.rhos)
    # Delta2 not matching Delta
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (_with(ps_api, tr, Delta2=w.K2[0].Delta2), vk), w.rhos)
    # Alpha changed
    assert not ps_api.Groth16CheckUpdate(ctx, w.K0, (_with(ps_api, tr, Alpha=tr.Beta), vk), w.rhos)


def test_errors(ps_api, ctx, co, pr):
    n, tw = 4, _toxic(pr)
    c, _ = _circuit(n)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        with pytest.raises(ps_api.LengthMismatch):
            ps_api.NewGroth16SetupFromSRS(q, _srs(ps_api, ctx, co, pr, n, tw, short=name))
    key = ps_api.NewGroth16SetupFromSRS(q, _srs(ps_api, ctx, co, pr, n, tw))
    for d, g in ((0, 5), (5, 0), (pr.R, 5)):
        with pytest.raises(ps_api.PlaysnarkError):
            ps_api.Groth16Contribute(ctx, *key, d, g)
    with pytest.raises(ps_api.LengthMismatch):  # fewer weights than the longest scaled array (XiT or NioLP: 3 points)
        ps_api.Groth16CheckUpdate(ctx, key, key, [3, 5])


def test_const_column_long_inside_the_full_route(ps_api, ctx, co, pr):
    """4 096 gates: the `const` variable's column of R has more than 512 non-zeros (half of the gates multiply by it), so the
    workgroup-per-row kernel runs inside the setup.  NioLP, IoLP and XiT against the toxic-waste setup."""
    n, tw = 4096, _toxic(pr)
    c, _ = _circuit(n)
    assert sum(1 for row in c.right for col, _ in row if col == 0) > 512
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, vk = ps_api.NewGroth16SetupFromSRS(q, _srs(ps_api, ctx, co, pr, n, tw))
    want, want_vk = ps_api.NewGroth16TrustedSetup(q, tw["alpha"], tw["beta"], 1, tw["x"], 1)
    assert tr.NioLP.download() == want.NioLP.download()
    assert vk["IoLP"].download() == want_vk["IoLP"].download()
    assert tr.XiT.download() == want.XiT.download()
