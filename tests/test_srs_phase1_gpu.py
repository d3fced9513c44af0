"""GPU: phase 1 of a Groth16 ceremony -- the power sequence (ps_scalars_powers), a fold into a powers-of-tau string
(ps_groth16_srs_contribute), the check that a string is well formed (ps_groth16_srs_check) and the check of a fold
(ps_groth16_srs_check_update).

Strings are made here from fixed values held in the clear -- {x^i}, {alpha x^i}, {beta x^i} in Python integers, committed
with Points.from_scalars -- so that a contributed string can be compared byte for byte with the string of the products, and so
that every tampered point lies in the subgroup: it is made by changing ONE scalar before the commitment.  Sizes n = 2 (sums of
one and two terms), 4 (the toy circuit), 40 (79 G1 points: past one wave), 200 (399 points: past a 256-thread block in G1 and,
with lane pairs, in G2).  Weights are 128 bits from SplitMix64, as in test_srs_setup_gpu.py."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = (2, 4, 40, 200)
ARRAYS = ("TauG1", "TauG2", "AlphaTauG1", "BetaTauG1")


def _values(pr):
    rng = pr.SplitMix64(20161017)
    return {k: rng.fr() for k in ("x", "alpha", "beta", "t1", "a1", "b1", "t2", "a2", "b2", "other")}


def _scalars(pr, x, alpha, beta, lens):
    """The exponents of a string: one list per array, and beta"""
    R = pr.R
    pw = [pow(x, i, R) for i in range(max(lens))]
    return {"TauG1": pw[: lens[0]], "TauG2": pw[: lens[1]], "AlphaTauG1": [alpha * p % R for p in pw[: lens[2]]],
            "BetaTauG1": [beta * p % R for p in pw[: lens[3]]], "BetaG2": beta}


def _commit(api, ctx, co, sc):
    mk = lambda g, v: api.Points.from_scalars(ctx, g, api.Poly.upload(ctx, v))
    return api.Groth16SRS(mk(api.G1, sc["TauG1"]), mk(api.G2, sc["TauG2"]), mk(api.G1, sc["AlphaTauG1"]), mk(api.G1, sc["BetaTauG1"]),
                          co.G2.to_b(co.G2.mul(sc["BetaG2"])))


def _lens(n):
    return (2 * n - 1, n, n, n)


def _string(api, ctx, co, pr, x, alpha, beta, lens):
    return _commit(api, ctx, co, _scalars(pr, x, alpha, beta, lens))


def _bytes(srs):
    return {f: getattr(srs, f).download() for f in ARRAYS} | {"BetaG2": srs.BetaG2}


def _assert_same_string(got, want, what):
    gb, wb = _bytes(got), _bytes(want)
    for f in wb:
        assert len(gb[f]) == len(wb[f]), (what, f, len(gb[f]), len(wb[f]))
        assert gb[f] == wb[f], (what, f)


def _rhos(pr, seed, count):
    rng = pr.SplitMix64(seed)
    return [(rng.next() << 64 | rng.next()) or 1 for _ in range(count)]


class World:
    pass


_worlds = {}


def _world(ps_api, ctx, co, pr, n):
    """Per size, made once: the clear string S0 for (x, alpha, beta), S1 = S0 with (t1, a1, b1) folded in, S2 = S1 with
    (t2, a2, b2), their shares, and the weights."""
    if n not in _worlds:
        w = World()
        w.n, w.v = n, _values(pr)
        v = w.v
        w.S0 = _string(ps_api, ctx, co, pr, v["x"], v["alpha"], v["beta"], _lens(n))
        w.S1, w.sh1 = ps_api.Groth16SRSContribute(ctx, w.S0, v["t1"], v["a1"], v["b1"])
        w.S2, w.sh2 = ps_api.Groth16SRSContribute(ctx, w.S1, v["t2"], v["a2"], v["b2"])
        w.rhos = _rhos(pr, n, 2 * n - 2)
        _worlds[n] = w
    return _worlds[n]


@pytest.fixture(params=SIZES)
def world(request, ps_api, ctx, co, pr):
    return _world(ps_api, ctx, co, pr, request.param)


# ---- the power sequence ----

_pow_ref = {}


def _powers_ref(pr, s, n):
    """[s^i mod r], i < n, by Python's pow; computed once per s at the longest n of the test and sliced"""
    if s not in _pow_ref:
        _pow_ref[s] = [pow(s, i, pr.R) for i in range(65537)]
    return _pow_ref[s][:n]


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 65537])
def test_powers_equal_python_pow(ps_api, ctx, pr, n):
    rng = pr.SplitMix64(31)
    s_rand, c_rand = rng.fr(), rng.fr()
    for s in (0, 1, pr.R - 1, s_rand):
        ref = _powers_ref(pr, s, n)
        if n:
            assert ref[0] == 1  # s^0 = 1, also for s = 0
        for c in (1, c_rand):
            got = ps_api.Poly.powers(ctx, s, n, c)
            assert len(got) == n
            vals = got.download()
            assert len(vals) == n
            bad = [i for i in range(n) if vals[i] != c * ref[i] % pr.R]
            assert not bad, (s, c, n, bad[:5])


def test_powers_reject_non_canonical_scalars(ps_api, ctx, pr):
    for s, c in ((pr.R, 1), (2**256 - 1, 1), (3, pr.R)):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.Poly.powers(ctx, s, 4, c)
        assert e.value.code == -3


# ---- contribute ----

def test_contribution_equals_the_string_of_the_products(ps_api, ctx, co, pr, world):
    w, v, R = world, world.v, pr.R
    want1 = _string(ps_api, ctx, co, pr, v["x"] * v["t1"] % R, v["alpha"] * v["a1"] % R, v["beta"] * v["b1"] % R, _lens(w.n))
    _assert_same_string(w.S1, want1, "one fold")
    want2 = _string(ps_api, ctx, co, pr, v["x"] * v["t1"] * v["t2"] % R, v["alpha"] * v["a1"] * v["a2"] % R,
                    v["beta"] * v["b1"] * v["b2"] % R, _lens(w.n))
    _assert_same_string(w.S2, want2, "two folds")
    for f in ARRAYS:  # as long as the input's
        assert len(getattr(w.S1, f)) == len(getattr(w.S0, f))


def test_every_output_point_against_the_oracle_at_4_gates(ps_api, ctx, co, pr):
    n, v, R = 4, _values(pr), pr.R
    S0 = _string(ps_api, ctx, co, pr, v["x"], v["alpha"], v["beta"], _lens(n))
    S1, _ = ps_api.Groth16SRSContribute(ctx, S0, v["t1"], v["a1"], v["b1"])
    for f, grp, lead in (("TauG1", co.G1, 1), ("TauG2", co.G2, 1), ("AlphaTauG1", co.G1, v["a1"]), ("BetaTauG1", co.G1, v["b1"])):
        was, got = grp.unpack(getattr(S0, f).download()), grp.unpack(getattr(S1, f).download())
        assert len(was) == len(got)
        for i, (p, q) in enumerate(zip(was, got)):
            assert q == grp.mul(lead * pow(v["t1"], i, R) % R, p), (f, i)
    assert S1.BetaG2 == co.G2.to_b(co.G2.mul(v["b1"], co.G2.from_b(S0.BetaG2)))


def test_share_holds_the_public_values(ps_api, co, world):
    w, v = world, world.v
    assert w.sh1 == {"T2": co.G2.to_b(co.G2.mul(v["t1"])), "A2": co.G2.to_b(co.G2.mul(v["a1"])), "B2": co.G2.to_b(co.G2.mul(v["b1"]))}
    assert w.sh2 == {"T2": co.G2.to_b(co.G2.mul(v["t2"])), "A2": co.G2.to_b(co.G2.mul(v["a2"])), "B2": co.G2.to_b(co.G2.mul(v["b2"]))}


def test_contribution_to_a_string_longer_than_any_circuit_shape(ps_api, ctx, co, pr):
    """Arrays of lengths that are no (2n-1, n, n, n): a ceremony string, with the scaled arrays of different lengths"""
    v, R, lens = _values(pr), pr.R, (300, 259, 81, 70)
    S0 = _string(ps_api, ctx, co, pr, v["x"], v["alpha"], v["beta"], lens)
    S1, _ = ps_api.Groth16SRSContribute(ctx, S0, v["t1"], v["a1"], v["b1"])
    assert tuple(len(getattr(S1, f)) for f in ARRAYS) == lens
    _assert_same_string(S1, _string(ps_api, ctx, co, pr, v["x"] * v["t1"] % R, v["alpha"] * v["a1"] % R, v["beta"] * v["b1"] % R, lens), "long")
    rhos = _rhos(pr, 300, 299)
    assert ps_api.Groth16SRSCheck(ctx, S1, rhos)
    cut = S1.truncate(70)  # views of the first 139, 70, 70, 70 points
    assert tuple(len(getattr(cut, f)) for f in ARRAYS) == (139, 70, 70, 70)
    assert ps_api.Groth16SRSCheck(ctx, cut, rhos[:138])


def test_contribution_keeps_identity_points(ps_api, ctx, co, pr):
    """Zero exponents in the input (the identity, stored as 0x40 00 ..): scaled to the identity, neighbours untouched"""
    n, v, R = 40, _values(pr), pr.R
    sc = _scalars(pr, v["x"], v["alpha"], v["beta"], _lens(n))
    for f, i in (("TauG1", 0), ("TauG1", 78), ("TauG2", 17), ("AlphaTauG1", 39), ("BetaTauG1", 1)):
        sc[f][i] = 0
    S1, _ = ps_api.Groth16SRSContribute(ctx, _commit(ps_api, ctx, co, sc), v["t1"], v["a1"], v["b1"])
    lead = {"TauG1": 1, "TauG2": 1, "AlphaTauG1": v["a1"], "BetaTauG1": v["b1"]}
    want = {f: [lead[f] * pow(v["t1"], i, R) * k % R for i, k in enumerate(sc[f])] for f in ARRAYS}
    want["BetaG2"] = v["beta"] * v["b1"] % R
    _assert_same_string(S1, _commit(ps_api, ctx, co, want), "identities")
    assert S1.TauG1.download(78, 1) == co.G1.to_b(None)


def test_contribution_errors(ps_api, ctx, co, pr):
    v = _values(pr)
    S0 = _string(ps_api, ctx, co, pr, v["x"], v["alpha"], v["beta"], _lens(4))
    for t, a, b in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.Groth16SRSContribute(ctx, S0, t, a, b)
        assert e.value.code == -5
    for t, a, b in ((pr.R, 5, 7), (5, pr.R + 1, 7), (5, 7, 2**256 - 1)):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.Groth16SRSContribute(ctx, S0, t, a, b)
        assert e.value.code == -3


# ---- check ----

def test_check_accepts_honest_strings(ps_api, ctx, world):
    w = world
    for s in (w.S0, w.S1, w.S2):
        assert ps_api.Groth16SRSCheck(ctx, s, w.rhos)
    assert ps_api.Groth16SRSCheck(ctx, w.S2, w.rhos, check_subgroup=False)
    assert ps_api.Groth16SRSCheck(ctx, w.S2, w.rhos + [5, 7])  # more weights than pairs


def test_check_accepts_the_initial_string(ps_api, ctx, co, world):
    w = world
    init = ps_api.Groth16SRS.initial(ctx, w.n)
    assert tuple(len(getattr(init, f)) for f in ARRAYS) == _lens(w.n)
    assert init.TauG1.download() == co.G1.to_b(co.G1.mul(1)) * (2 * w.n - 1)
    assert init.TauG2.download() == co.G2.to_b(co.G2.mul(1)) * w.n and init.BetaG2 == co.G2.to_b(co.G2.mul(1))
    assert ps_api.Groth16SRSCheck(ctx, init, w.rhos)


def _tampered(ps_api, ctx, co, pr, w, edit):
    sc = _scalars(pr, w.v["x"], w.v["alpha"], w.v["beta"], _lens(w.n))
    edit(sc)
    return _commit(ps_api, ctx, co, sc)


def test_check_rejects_one_replaced_point_anywhere(ps_api, ctx, co, pr, world):
    """The first, a middle and the LAST point of each array, replaced by another subgroup point"""
    w = world
    for f in ARRAYS:
        m = len(getattr(w.S0, f))
        for i in sorted({0, m // 2, m - 1}):
            def edit(sc, f=f, i=i):
                sc[f][i] = (sc[f][i] + 1) % pr.R
            assert not ps_api.Groth16SRSCheck(ctx, _tampered(ps_api, ctx, co, pr, w, edit), w.rhos), (f, i)


def test_check_rejects_structural_errors(ps_api, ctx, co, pr, world):
    w, v, R, n = world, world.v, pr.R, world.n
    other = _scalars(pr, v["other"], v["alpha"], v["beta"], _lens(n))

    def swap(sc):  # two neighbouring powers exchanged
        a = sc["TauG1"]
        a[-2], a[-1] = a[-1], a[-2]

    def tau_g2_of_another_tau(sc):
        sc["TauG2"] = other["TauG2"]

    def alpha_over_another_tau(sc):
        sc["AlphaTauG1"] = other["AlphaTauG1"]

    def beta_g2_of_another_beta(sc):
        sc["BetaG2"] = v["other"]

    def first_power_is_not_the_generator(sc):  # a consistent string over 2 G1: every pair equation holds
        sc["TauG1"] = [2 * k % R for k in sc["TauG1"]]

    for edit in (swap, tau_g2_of_another_tau, alpha_over_another_tau, beta_g2_of_another_beta, first_power_is_not_the_generator):
        assert not ps_api.Groth16SRSCheck(ctx, _tampered(ps_api, ctx, co, pr, w, edit), w.rhos), edit.__name__
    # tau = 0: T1 = (G1, O, O, ..), every pair equation holds with the identity on both sides
    zero = _string(ps_api, ctx, co, pr, 0, v["alpha"], v["beta"], _lens(n))
    assert zero.TauG1.download(1, 1) == co.G1.to_b(None)
    assert not ps_api.Groth16SRSCheck(ctx, zero, w.rhos)


def test_check_rejects_points_outside_the_subgroup(ps_api, ctx, co, world, off_subgroup):
    w = world
    raw = bytearray(w.S1.AlphaTauG1.download())
    raw[-96:] = co.G1.to_b(off_subgroup[0])
    bad = ps_api.Groth16SRS(w.S1.TauG1, w.S1.TauG2, ps_api.Points.upload(ctx, ps_api.G1, bytes(raw)), w.S1.BetaTauG1, w.S1.BetaG2)
    assert not ps_api.Groth16SRSCheck(ctx, bad, w.rhos)
    bad = ps_api.Groth16SRS(w.S1.TauG1, w.S1.TauG2, w.S1.AlphaTauG1, w.S1.BetaTauG1, co.G2.to_b(off_subgroup[1]))
    assert not ps_api.Groth16SRSCheck(ctx, bad, w.rhos)


def test_check_errors(ps_api, ctx, co, pr, world):
    w = world
    with pytest.raises(ps_api.LengthMismatch):  # one weight short of the 2n - 2 neighbouring pairs of tau_g1
        ps_api.Groth16SRSCheck(ctx, w.S1, w.rhos[:-1])
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.Groth16SRSCheck(ctx, w.S1, [pr.R] + w.rhos[1:])
    assert e.value.code == -3
    with pytest.raises(ps_api.PlaysnarkError) as e:  # tau_g2 of one point: no tau in G2
        ps_api.Groth16SRSCheck(ctx, ps_api.Groth16SRS(w.S1.TauG1, w.S1.TauG2.slice(0, 1), w.S1.AlphaTauG1, w.S1.BetaTauG1, w.S1.BetaG2), w.rhos)
    assert e.value.code == -5
    # alpha_tau_g1 and beta_tau_g1 of one point each are fine: nothing to pair
    assert ps_api.Groth16SRSCheck(ctx, ps_api.Groth16SRS(w.S1.TauG1, w.S1.TauG2, w.S1.AlphaTauG1.slice(0, 1), w.S1.BetaTauG1.slice(0, 1), w.S1.BetaG2),
                                  w.rhos)


# ---- check of a fold ----

def test_check_update_accepts_honest_folds(ps_api, ctx, world):
    w = world
    assert ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S1, w.sh1, w.rhos)
    assert ps_api.Groth16SRSCheckUpdate(ctx, w.S1, w.S2, w.sh2, w.rhos)


def test_check_update_rejects_what_is_no_fold_of_the_share(ps_api, ctx, co, pr, world):
    w, v, R, n = world, world.v, pr.R, world.n
    g2 = lambda k: co.G2.to_b(co.G2.mul(k))
    for key, k in (("T2", v["t2"]), ("A2", v["a2"]), ("B2", v["b2"])):  # a share with another t, a or b
        assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S1, dict(w.sh1, **{key: g2(k)}), w.rhos), key
    for key in ("T2", "A2", "B2"):  # the identity as share
        assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S1, dict(w.sh1, **{key: co.G2.to_b(None)}), w.rhos), key
    # a well-formed `after` that builds on a different `before`
    assert ps_api.Groth16SRSCheck(ctx, w.S2, w.rhos)
    assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S2, w.sh2, w.rhos)
    elsewhere = _string(ps_api, ctx, co, pr, v["other"], v["alpha"], v["beta"], _lens(n))
    assert not ps_api.Groth16SRSCheckUpdate(ctx, elsewhere, w.S1, w.sh1, w.rhos)
    # an `after` of another length: well formed, one gate longer
    longer = _string(ps_api, ctx, co, pr, v["x"] * v["t1"] % R, v["alpha"] * v["a1"] % R, v["beta"] * v["b1"] % R, _lens(n + 1))
    rhos = _rhos(pr, 7, 2 * n)
    assert ps_api.Groth16SRSCheck(ctx, longer, rhos)
    assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, longer, w.sh1, rhos)
    # an `after` that is not well formed, though its heads match the share
    def edit(sc):
        sc["TauG1"][-1] = (sc["TauG1"][-1] + 1) % R
    sc = _scalars(pr, v["x"] * v["t1"] % R, v["alpha"] * v["a1"] % R, v["beta"] * v["b1"] % R, _lens(n))
    edit(sc)
    assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, _commit(ps_api, ctx, co, sc), w.sh1, w.rhos)
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S1, w.sh1, w.rhos[:-1])


def test_check_update_rejects_a_share_outside_the_subgroup(ps_api, ctx, co, pr, off_subgroup):
    w = _world(ps_api, ctx, co, pr, 4)
    assert not ps_api.Groth16SRSCheckUpdate(ctx, w.S0, w.S1, dict(w.sh1, T2=co.G2.to_b(off_subgroup[1])), w.rhos)


# ---- end to end ----

def test_ceremony_end_to_end_at_40_gates(ps_api, ctx, pr):
    """The trivial string, two folds each accepted by the check, truncation, the circuit's key from it -- byte-identical to the
    toxic-waste setup for (alpha, beta, delta, x, gamma) = (a1 a2, b1 b2, 1, t1 t2, 1) -- and a proof under it that verifies."""
    from oracle import restate as rs

    n, m, v, R = 40, 48, _values(pr), pr.R  # the ceremony serves circuits of up to 48 gates
    rhos = _rhos(pr, 40, 2 * m - 2)
    S0 = ps_api.Groth16SRS.initial(ctx, m)
    S1, sh1 = ps_api.Groth16SRSContribute(ctx, S0, v["t1"], v["a1"], v["b1"])
    assert ps_api.Groth16SRSCheckUpdate(ctx, S0, S1, sh1, rhos)
    S2, sh2 = ps_api.Groth16SRSContribute(ctx, S1, v["t2"], v["a2"], v["b2"])
    assert ps_api.Groth16SRSCheckUpdate(ctx, S1, S2, sh2, rhos)
    c, sol_v = rs.synthetic_circuit(n)
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, vk = ps_api.NewGroth16SetupFromSRS(q, S2.truncate(n))
    want, want_vk = ps_api.NewGroth16TrustedSetup(q, v["a1"] * v["a2"] % R, v["b1"] * v["b2"] % R, 1, v["t1"] * v["t2"] % R, 1)
    for f in ("Alpha", "Beta", "Delta", "Beta2", "Delta2"):
        assert getattr(tr, f) == getattr(want, f), f
    for f in ("Xi", "Xi2", "NioLP", "XiT", "LXi", "LXi2", "LXiT"):
        assert getattr(tr, f).download() == getattr(want, f).download(), f
    assert vk["Gamma"] == want_vk["Gamma"] and vk["IoLP"].download() == want_vk["IoLP"].download()
    diff = c.nbVars - c.nbIO
    proof = ps_api.Groth16Prove(tr, q, ps_api.Poly.upload(ctx, sol_v), 0x1F2E3D4C5B6A7988, 0x0123456789ABCDEF0FEDCBA987654321)
    assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], proof, ps_api.Poly.upload(ctx, sol_v[:diff]))
