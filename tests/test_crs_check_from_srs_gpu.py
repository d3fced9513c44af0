"""GPU: is a Groth16 key what its powers-of-tau string makes of it (ps_groth16_crs_check_from_srs), and is an array the Lagrange
form of another (ps_points_lagrange_check) -- without the conversions over group elements.

Keys are made with NewGroth16TrustedSetup from fixed toxic values, the string from the same values with Points.from_scalars, as
tests/test_srs_setup_gpu.py does: that route is pinned there, byte for byte, to ps_groth16_setup_from_srs and to the oracle, and
it costs milliseconds.  Accepted: the key at delta = gamma = 1, after one and two folds, monomial-only, with the subgroup tests on
and off.  Rejected: keys that differ from an accepted one in exactly one thing."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = (4, 5, 40, 68, 200)  # 2n - 1 = 9 and 135 sit just past a power of two, 7 just below; 4 is the toy circuit
PROVER_ARRAYS = ("Xi", "Xi2", "NioLP", "XiT", "LXi", "LXi2", "LXiT")


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


def _weights(pr, seed, count):
    rng = pr.SplitMix64(seed)
    return [(rng.next() << 64 | rng.next()) or 1 for _ in range(count)]


class World:
    pass


_worlds = {}


def _world(ps_api, ctx, co, pr, n, circuit=None):
    w = World()
    w.n, w.tw = n, _toxic(pr)
    w.c = circuit if circuit is not None else _circuit(n)[0]
    w.q = ps_api.QAP(ctx, w.c.nbVars, w.c.nbIO, w.c.left, w.c.right, w.c.out)
    w.srs = _srs(ps_api, ctx, co, pr, n, w.tw)
    w.K0 = ps_api.NewGroth16TrustedSetup(w.q, w.tw["alpha"], w.tw["beta"], 1, w.tw["x"], 1)
    w.rhos = _weights(pr, n, max(w.c.nbVars, n))
    return w


def _shared_world(ps_api, ctx, co, pr, n):
    """Per circuit size, made once: the circuit, its string, the key K0 at delta = gamma = 1 and the keys after one (K1) and two
    (K2) folds."""
    if n not in _worlds:
        w = _world(ps_api, ctx, co, pr, n)
        w.K1 = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d"], w.tw["g"])
        w.K2 = ps_api.Groth16Contribute(ctx, *w.K1, w.tw["d2"], w.tw["g2"])
        _worlds[n] = w
    return _worlds[n]


@pytest.fixture(params=SIZES)
def world(request, ps_api, ctx, co, pr):
    return _shared_world(ps_api, ctx, co, pr, request.param)


def _check(ps_api, ctx, w, key, **kw):
    return ps_api.Groth16CheckFromSRS(ctx, w.q, w.srs, key, w.rhos, **kw)


def _with(ps_api, tr, **repl):
    f = dict(Alpha=tr.Alpha, Beta=tr.Beta, Delta=tr.Delta, Beta2=tr.Beta2, Delta2=tr.Delta2, Xi=tr.Xi, Xi2=tr.Xi2, NioLP=tr.NioLP,
             XiT=tr.XiT, LXi=tr.LXi, LXi2=tr.LXi2, LXiT=tr.LXiT)
    f.update(repl)
    return ps_api.Groth16Setup(**f)


def _points_of(key, name):
    tr, vk = key
    return vk["IoLP"] if name == "IoLP" else getattr(tr, name)


def _key_with_array(ps_api, key, name, pts):
    tr, vk = key
    if name == "IoLP":
        return tr, {"Gamma": vk["Gamma"], "IoLP": pts}
    return _with(ps_api, tr, **{name: pts}), vk


def _replaced(ps_api, ctx, co, pts, index):
    """pts with the point at `index` replaced by another point of the subgroup"""
    grp, wb = (co.G1, 96) if pts.group == ps_api.G1 else (co.G2, 192)
    raw = bytearray(pts.download())
    at = index % len(pts)
    other = grp.to_b(grp.mul(7))
    if bytes(raw[wb * at:wb * (at + 1)]) == other:
        other = grp.to_b(grp.mul(11))
    raw[wb * at:wb * (at + 1)] = other
    return ps_api.Points.upload(ctx, pts.group, bytes(raw))


def test_accepts_the_key_at_delta_gamma_one_and_after_folds(ps_api, ctx, world):
    w = world
    for key in (w.K0, w.K1, w.K2):
        assert _check(ps_api, ctx, w, key)
        assert _check(ps_api, ctx, w, key, check_subgroup=False)


def test_accepts_a_monomial_only_key(ps_api, ctx, world):
    tr, vk = world.K1
    assert _check(ps_api, ctx, world, (tr.monomial_only(), vk))
    assert _check(ps_api, ctx, world, (_with(ps_api, tr, LXi2=None, LXiT=None), vk))  # any of the three alone is checked alone


@pytest.mark.parametrize("name", PROVER_ARRAYS + ("IoLP",))
def test_rejects_one_replaced_point_in_each_array(ps_api, ctx, co, world, name):
    w = world
    for index in (0, -1):
        bad = _key_with_array(ps_api, w.K1, name, _replaced(ps_api, ctx, co, _points_of(w.K1, name), index))
        assert not _check(ps_api, ctx, w, bad), (name, index)
        assert not _check(ps_api, ctx, w, bad, check_subgroup=False), (name, index)


def test_rejects_keys_the_string_does_not_make(ps_api, ctx, co, world):
    w = world
    tr, vk = w.K1
    # two entries of LXi swapped
    raw = tr.LXi.download()
    last = len(tr.LXi) - 1
    swapped = raw[96 * last:] + raw[96:96 * last] + raw[:96]
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, LXi=ps_api.Points.upload(ctx, ps_api.G1, swapped)), vk))
    # LXiT, then XiT, of a key folded with another delta: scaled differently from each other and from NioLP
    other, _ = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d2"], w.tw["g"])
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, LXiT=other.LXiT), vk))
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, XiT=other.XiT, LXiT=other.LXiT), vk))
    # IoLP scaled differently from Gamma
    _, other_vk = ps_api.Groth16Contribute(ctx, *w.K0, w.tw["d"], w.tw["g2"])
    assert not _check(ps_api, ctx, w, (tr, {"Gamma": vk["Gamma"], "IoLP": other_vk["IoLP"]}))
    # Delta2 not matching Delta
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, Delta2=w.K2[0].Delta2), vk))
    # Alpha replaced by Beta, Beta2 by G2
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, Alpha=tr.Beta), vk))
    assert not _check(ps_api, ctx, w, (_with(ps_api, tr, Beta2=co.G2.to_b(co.G2.mul(1))), vk))
    # a key array one point short: no error, a rejection
    for name in PROVER_ARRAYS + ("IoLP",):
        pts = _points_of(w.K1, name)
        assert not _check(ps_api, ctx, w, _key_with_array(ps_api, w.K1, name, pts.slice(0, len(pts) - 1))), name


@pytest.mark.parametrize("which", ("left", "right", "out"))
def test_rejects_the_key_of_a_circuit_that_differs_in_one_coefficient(ps_api, ctx, world, which):
    from oracle import restate as rs

    w = world
    rows = {m: [list(r) for r in getattr(w.c, m)] for m in ("left", "right", "out")}
    gate = w.n // 2
    col, v = rows[which][gate][0]
    rows[which][gate][0] = (col, v + 1)
    c2 = rs.SparseR1CS(w.c.nbVars, w.c.nbIO, rows["left"], rows["right"], rows["out"])
    q2 = ps_api.QAP(ctx, c2.nbVars, c2.nbIO, c2.left, c2.right, c2.out)
    other = ps_api.NewGroth16TrustedSetup(q2, w.tw["alpha"], w.tw["beta"], 1, w.tw["x"], 1)
    assert ps_api.Groth16CheckFromSRS(ctx, q2, w.srs, other, w.rhos)  # the other circuit's key, against the other circuit
    assert not _check(ps_api, ctx, w, other)


def test_rejects_the_key_of_a_string_with_another_x(ps_api, ctx, pr, world):
    w = world
    other = ps_api.NewGroth16TrustedSetup(w.q, w.tw["alpha"], w.tw["beta"], 1, (w.tw["x"] + 1) % pr.R, 1)
    assert not _check(ps_api, ctx, w, other)


def test_long_rows_inside_the_check(ps_api, ctx, co, pr):
    """1 025 gates with rows of up to 8 193 entries: the workgroup-per-row SpMV kernel computes L rho_S inside the check."""
    import quotient_cases as qc

    c = qc.transposed_long_circuit().circuit()
    assert max(len(r) for r in c.left) > 512
    w = _world(ps_api, ctx, co, pr, c.nbGates, circuit=c)
    assert _check(ps_api, ctx, w, w.K0, check_subgroup=False)
    bad = _key_with_array(ps_api, w.K0, "NioLP", _replaced(ps_api, ctx, co, w.K0[0].NioLP, len(w.K0[0].NioLP) // 2))
    assert not _check(ps_api, ctx, w, bad, check_subgroup=False)


def test_errors(ps_api, ctx, co, pr):
    from playsnark_amd import _lib

    n = 4
    w = _world(ps_api, ctx, co, pr, n)
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        with pytest.raises(ps_api.LengthMismatch):
            ps_api.Groth16CheckFromSRS(ctx, w.q, _srs(ps_api, ctx, co, pr, n, w.tw, short=name), w.K0, w.rhos)
    with pytest.raises(ps_api.LengthMismatch):  # max(nbVars, n) = 6 weights are needed
        ps_api.Groth16CheckFromSRS(ctx, w.q, w.srs, w.K0, w.rhos[:5])
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16CheckFromSRS(ctx, w.q, w.srs, w.K0, w.rhos[:5] + [pr.R])
    assert e.value.code == _lib.PS_ERR_ENCODING
    tr = w.K0[0]
    sc = ps_api.Poly.upload(ctx, w.rhos[:n])
    assert _lib.lib.ps_msm_launch(ctx._h, tr.Xi._h, sc._h) == 0  # a sum left pending on the context
    try:
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.Groth16CheckFromSRS(ctx, w.q, w.srs, w.K0, w.rhos)
        assert e.value.code == _lib.PS_ERR_ARG
        with pytest.raises(ps_api.PlaysnarkError) as e:
            tr.Xi.lagrange_check(w.q, tr.LXi, w.rhos)
        assert e.value.code == _lib.PS_ERR_ARG
    finally:
        import ctypes

        assert _lib.lib.ps_msm_finish(ctx._h, ctypes.create_string_buffer(96)) == 0
    assert ps_api.Groth16CheckFromSRS(ctx, w.q, w.srs, w.K0, w.rhos)


def test_lagrange_check_both_groups_and_both_node_sets(ps_api, ctx, co, world):
    w = world
    tr, _ = w.K1
    pairs = ((tr.Xi, tr.LXi, 0), (tr.Xi2, tr.LXi2, 0), (tr.XiT, tr.LXiT, 1))
    for mono, lagr, nodes in pairs:
        assert mono.lagrange_check(w.q, lagr, w.rhos, nodes)
        for index in (0, -1):
            assert not mono.lagrange_check(w.q, _replaced(ps_api, ctx, co, lagr, index), w.rhos, nodes)
            assert not _replaced(ps_api, ctx, co, mono, index).lagrange_check(w.q, lagr, w.rhos, nodes)
    # the form on 1..n is not the form on n+1..2n-1 of the same powers
    mono = tr.Xi.slice(0, w.n - 1)
    assert not mono.lagrange_check(w.q, tr.LXi.slice(0, w.n - 1), w.rhos, 1)
    # lengths, groups, weights
    with pytest.raises(ps_api.LengthMismatch):
        tr.Xi.lagrange_check(w.q, tr.LXi, w.rhos, 1)
    with pytest.raises(ps_api.LengthMismatch):
        tr.Xi.lagrange_check(w.q, tr.LXi, w.rhos[:w.n - 1], 0)
    with pytest.raises(ps_api.PlaysnarkError):
        tr.Xi.lagrange_check(w.q, tr.LXi2, w.rhos, 0)
    with pytest.raises(ps_api.PlaysnarkError):
        tr.Xi.lagrange_check(w.q, tr.LXi, [ps_api.R_ORDER] + w.rhos[1:], 0)


@pytest.mark.parametrize("n", (4, 5, 68))
def test_lagrange_check_of_a_converted_array_and_of_the_phgr13_pair(ps_api, ctx, co, pr, n):
    """The arrays ps_points_monomial_to_lagrange itself makes (a conversion over group elements: the smaller sizes), and PHGR13's
    gsi / lgsi pair from ps_phgr13_setup."""
    w = _shared_world(ps_api, ctx, co, pr, n)
    tr, _ = w.K0
    assert tr.Xi.lagrange_check(w.q, tr.Xi.to_lagrange(w.q, 0), w.rhos, 0)
    assert tr.XiT.lagrange_check(w.q, tr.XiT.to_lagrange(w.q, 1), w.rhos, 1)
    rng = pr.SplitMix64(13)
    ek, _ = ps_api.NewPHGR13TrustedSetup(w.q, *[rng.fr() for _ in range(8)])
    assert ek.gsi.lagrange_check(w.q, ek.lgsi, w.rhos, 1)
    assert not ek.gsi.lagrange_check(w.q, _replaced(ps_api, ctx, co, ek.lgsi, 1), w.rhos, 1)
