"""GPU: ONE KZG proof for a set of points of one polynomial -- KZGOpenSet (ps_kzg_open_set) and KZGVerifySet
(ps_kzg_verify_set) -- over a powers-of-tau string held in the clear (tau known, as tests/test_kzg_gpu.py makes it: 2T + 1 + 3
points of G1, and 66 of G2 made the same way).  The proof is compared byte for byte with the oracle's scalar multiplication
[q(tau)] G1, with the lone sum over the uploaded oracle quotient (a route that touches no new kernel), with the weighted sum of
KZGOpen's k proofs, and at k = 1 with KZGOpen's proof; the verifier accepts what KZGOpenSet made and rejects each single change,
every changed point still in the subgroup."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
EXTRA = 3  # the string is longer than every polynomial
G2_POINTS = 66


def _tile():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_tile()


def _group():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_set_group()


T, G = _tile(), _group()
SIZES = [2, 5, 257, T + 1, 2 * T + 1]
SETS = sorted({1, 3, G + 1, 33})


@pytest.fixture(scope="module")
def string(ps_api, ctx, co):
    """tau_g1 (2T + 1 + EXTRA points) and tau_g2 (66 points) on the device, and tau G2 as bytes."""
    tau_g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.powers(ctx, TAU, 2 * T + 1 + EXTRA))
    tau_g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, G2_POINTS))
    return tau_g1, tau_g2, co.G2.to_b(co.G2.mul(TAU))


def _g1(co, k):
    return co.G1.to_b(co.G1.mul(k))


def _vanishing(pr, zs):
    zp = [1]
    for z in zs:
        zp = pr.poly_mul(zp, [(-z) % pr.R, 1])
    return zp


def _quotient(pr, p, zs):
    if len(p) <= len(zs):
        return []
    q, _ = pr.poly_div(p[::-1], _vanishing(pr, zs)[::-1])
    return q[::-1]


def _weights(pr, zs):
    ws = []
    for j, zj in enumerate(zs):
        d = 1
        for l, zl in enumerate(zs):
            if l != j:
                d = d * (zj - zl) % pr.R
        ws.append(pr.fr_inv(d))
    return ws


@pytest.mark.parametrize("n", SIZES)
def test_the_proof_is_the_oracles_point_and_the_composed_routes(ps_api, ctx, co, pr, string, n):
    tau_g1, _, _ = string
    rng = pr.SplitMix64(0x5E70 + n)
    p = [rng.fr() for _ in range(n)]
    poly = ps_api.Poly.upload(ctx, p)
    tau_n = tau_g1.slice(0, n + EXTRA)  # longer than p
    for k in SETS:
        zs = [rng.fr() for _ in range(k)]
        ys, proof = ps_api.KZGOpenSet(tau_n, poly, zs)
        assert ys == [pr.poly_eval(p, z) for z in zs], (n, k)
        q = _quotient(pr, p, zs)
        assert len(q) == max(n - k, 0)
        assert proof == _g1(co, pr.poly_eval(q, TAU)), (n, k)  # the identity for n <= k
        if n <= k:
            assert proof == _g1(co, 0)
            continue
        # the lone sum over the uploaded oracle quotient: no new kernel on this route
        assert ps_api.Poly.upload(ctx, q).BlindEval(tau_g1.slice(0, n - k)) == proof, (n, k)
        # the weighted sum of the k single-point proofs
        ys1, proofs = ps_api.KZGOpen(tau_n, poly, zs)
        assert ys1 == ys
        assert ps_api.points_lincomb(ps_api.G1, b"".join(proofs), _weights(pr, zs)) == proof, (n, k)
        if k == 1:
            assert proofs == [proof]


class _Opened:
    pass


@pytest.fixture(scope="module")
def opened(ps_api, ctx, pr, string):
    """One polynomial of 257 coefficients opened at G + 1 points and at one point, with its commitment"""
    tau_g1, _, _ = string
    o = _Opened()
    rng = pr.SplitMix64(0x0FE3)
    o.p = [rng.fr() for _ in range(257)]
    o.poly = ps_api.Poly.upload(ctx, o.p)
    o.commit = ps_api.KZGCommit(tau_g1, o.poly)
    o.zs = [rng.fr() for _ in range(G + 1)]
    o.ys, o.proof = ps_api.KZGOpenSet(tau_g1, o.poly, o.zs)
    o.z1 = [rng.fr()]
    o.y1, o.proof1 = ps_api.KZGOpenSet(tau_g1, o.poly, o.z1)
    o.p2 = [rng.fr() for _ in range(257)]
    o.commit2 = ps_api.KZGCommit(tau_g1, ps_api.Poly.upload(ctx, o.p2))  # a commitment of another polynomial
    return o


def test_verify_accepts_what_open_made(ps_api, ctx, pr, string, opened):
    tau_g1, tau_g2, _ = string
    o = opened
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, o.zs, o.ys, o.proof)
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, o.zs, o.ys, o.proof, check_subgroup=False)
    assert ps_api.KZGVerifySet(ctx, tau_g1.slice(0, G + 1), tau_g2.slice(0, G + 2), o.commit, o.zs, o.ys, o.proof)  # exactly k and k + 1
    # the points in another order: the same set, the values permuted with them, the same proof
    order = list(range(len(o.zs)))[::-1]
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, [o.zs[i] for i in order], [o.ys[i] for i in order], o.proof)
    # the largest set the G2 string of this file allows, and a polynomial shorter than the set (identity proof)
    rng = pr.SplitMix64(0x0FE4)
    zs = [rng.fr() for _ in range(G2_POINTS - 1)]
    ys, proof = ps_api.KZGOpenSet(tau_g1, o.poly, zs)
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, zs, ys, proof)
    short = ps_api.Poly.upload(ctx, o.p[:5])
    ys, proof = ps_api.KZGOpenSet(tau_g1, short, zs[:9])
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, ps_api.KZGCommit(tau_g1, short), zs[:9], ys, proof)


def test_verify_rejects_every_single_change(ps_api, ctx, pr, string, opened):
    tau_g1, tau_g2, _ = string
    o = opened
    R = pr.R
    ys_plus = list(o.ys)
    ys_plus[2] = (ys_plus[2] + 1) % R
    zs_plus = list(o.zs)
    zs_plus[G] = (zs_plus[G] + 1) % R
    ys_swapped = [o.ys[1], o.ys[0]] + o.ys[2:]
    other_zs = o.zs[:-1] + [(o.zs[-1] + 1) % R]
    _, other_proof = ps_api.KZGOpenSet(tau_g1, o.poly, other_zs)  # a proof of another set of the SAME polynomial
    changes = {
        "one y": (o.commit, o.zs, ys_plus, o.proof),
        "one z": (o.commit, zs_plus, o.ys, o.proof),
        "two y's swapped": (o.commit, o.zs, ys_swapped, o.proof),
        "the proof of another set": (o.commit, o.zs, o.ys, other_proof),
        "the commitment of another polynomial": (o.commit2, o.zs, o.ys, o.proof),
    }
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, o.zs, o.ys, o.proof)
    for what, (c, zs, ys, pi) in changes.items():
        assert not ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, c, zs, ys, pi), what
        assert not ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, c, zs, ys, pi, check_subgroup=False), what


def test_off_subgroup_malformed_and_short_strings(ps_api, ctx, pr, string, opened, off_subgroup):
    tau_g1, tau_g2, _ = string
    o = opened
    k = len(o.zs)
    bad = pr.g1_to_bytes(off_subgroup[0])
    assert not ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, bad, o.zs, o.ys, o.proof)
    assert not ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, o.zs, o.ys, bad)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # not on the curve at all
        ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, bad[:95] + bytes([bad[95] ^ 1]), o.zs, o.ys, o.proof)
    assert e.value.code == -3
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, o.zs, o.ys, o.proof[:95] + bytes([o.proof[95] ^ 1]))
    assert e.value.code == -3
    with pytest.raises(ps_api.LengthMismatch):  # k - 1 points of G1
        ps_api.KZGVerifySet(ctx, tau_g1.slice(0, k - 1), tau_g2, o.commit, o.zs, o.ys, o.proof)
    with pytest.raises(ps_api.LengthMismatch):  # k points of G2 where k + 1 are needed
        ps_api.KZGVerifySet(ctx, tau_g1, tau_g2.slice(0, k), o.commit, o.zs, o.ys, o.proof)
    for zs, ys, code in ((o.zs[:-1] + [pr.R], o.ys, -3), (o.zs, o.ys[:-1] + [pr.R], -3), (o.zs[:-1] + [o.zs[0]], o.ys, -5), ([], [], -5)):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, o.commit, zs, ys, o.proof)
        assert e.value.code == code
    with pytest.raises(ps_api.PlaysnarkError) as e:  # the two strings the other way round
        ps_api.KZGVerifySet(ctx, tau_g2, tau_g1, o.commit, o.zs, o.ys, o.proof)
    assert e.value.code == -5


def test_at_one_point_the_verdicts_are_kzg_verifys(ps_api, ctx, co, pr, string, opened):
    tau_g1, tau_g2, t2 = string
    o = opened
    (z,), (y,) = o.z1, o.y1
    _, (pi,) = ps_api.KZGOpen(tau_g1, o.poly, [z])
    assert pi == o.proof1
    _, other = ps_api.KZGOpenSet(tau_g1, o.poly, [(z + 1) % pr.R])
    cases = {
        "as made": (o.commit, z, y, o.proof1),
        "y + 1": (o.commit, z, (y + 1) % pr.R, o.proof1),
        "z + 1": (o.commit, (z + 1) % pr.R, y, o.proof1),
        "a proof of another point": (o.commit, z, y, other),
        "a commitment of another polynomial": (o.commit2, z, y, o.proof1),
    }
    for what, (c, zz, yy, pp) in cases.items():
        single = ps_api.KZGVerify(t2, c, zz, yy, pp)
        assert single == (what == "as made"), what
        assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, c, [zz], [yy], pp) == single, what


def test_open_set_argument_checks(ps_api, ctx, pr, string, opened):
    tau_g1, _, _ = string
    o = opened
    with pytest.raises(ps_api.PlaysnarkError) as e:  # two equal points: both indices are named
        ps_api.KZGOpenSet(tau_g1, o.poly, [5, 6, 5])
    assert e.value.code == -5 and "z[0]" in str(e.value) and "z[2]" in str(e.value)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.KZGOpenSet(tau_g1, o.poly, [5, pr.R])
    assert e.value.code == -3
    for zs in ([], list(range(1025))):
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGOpenSet(tau_g1, o.poly, zs)
        assert e.value.code == -5
    with pytest.raises(ps_api.LengthMismatch):  # the string is shorter than the polynomial
        ps_api.KZGOpenSet(tau_g1.slice(0, 256), o.poly, o.zs)
    with pytest.raises(ps_api.LengthMismatch):  # an empty polynomial
        ps_api.KZGOpenSet(tau_g1, o.poly.slice(0, 0), o.zs)
    ps_api.msm_launch(ctx, tau_g1.slice(0, 5), o.poly.slice(0, 5))  # a sum pending on the context
    try:
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGOpenSet(tau_g1, o.poly, o.zs)
        assert e.value.code == -5
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGVerifySet(ctx, tau_g1, string[1], o.commit, o.zs, o.ys, o.proof)
        assert e.value.code == -5
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
