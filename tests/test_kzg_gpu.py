"""GPU: KZG commitments over a powers-of-tau string held in the clear (tau known, as tests/test_srs_phase1_gpu.py makes its
strings): KZGCommit, KZGOpen, KZGVerify and KZGVerifyBatch.  Commitments and proofs are compared byte for byte with the
oracle's scalar multiplications [p(tau)] G1 and [q_j(tau)] G1 and with the composed route (Poly.DivLinear, then BlindEval);
the verifiers accept what KZGOpen made and reject each single change -- every changed point still in the subgroup, made by
changing one scalar before committing -- a cancelling pair of errors under random weights, and an off-subgroup commitment."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
EXTRA = 3  # the string is longer than every polynomial


def _tile():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_scan_tile()


def _sizes():
    return [1, 2, 5, 257, _tile() + 1]


@pytest.fixture(scope="module")
def string(ps_api, ctx, co):
    """tau_g1 (T + 1 + EXTRA points) on the device and tau G2 as bytes."""
    n = _tile() + 1 + EXTRA
    tau_g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.powers(ctx, TAU, n))
    return tau_g1, co.G2.to_b(co.G2.mul(TAU))


def _g1(co, k):
    return co.G1.to_b(co.G1.mul(k))


def _quotient(pr, p, z):
    q, rem = pr.poly_div(p[::-1], [1, (-z) % pr.R])
    return q[::-1], rem[0]


@pytest.mark.parametrize("n", _sizes())
def test_commitment_and_openings_are_the_oracles_points(ps_api, ctx, co, pr, string, n):
    tau_g1, _ = string
    rng = pr.SplitMix64(0xC0 + n)
    p = [rng.fr() for _ in range(n)]
    poly = ps_api.Poly.upload(ctx, p)
    tau_n = tau_g1.slice(0, n + EXTRA)  # longer than p
    assert ps_api.KZGCommit(tau_n, poly) == _g1(co, pr.poly_eval(p, TAU))
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.KZGCommit(tau_g1.slice(0, n - 1), poly)
    for k in (1, 3):
        zs = [rng.fr() for _ in range(k)]
        ys, proofs = ps_api.KZGOpen(tau_n, poly, zs)
        assert ys == [pr.poly_eval(p, z) for z in zs]
        for j, z in enumerate(zs):
            q, rem = (_quotient(pr, p, z) if n >= 2 else ([], p[0]))
            assert rem == ys[j]
            assert proofs[j] == _g1(co, pr.poly_eval(q, TAU)), (n, k, j)  # the identity for a constant
            if n >= 2:  # the composed route: one division, one sum
                qd, _ = poly.DivLinear([z])
                assert qd.BlindEval(tau_g1.slice(0, n - 1)) == proofs[j]


class _Items(list):
    """the openings, and the coefficients of the polynomial of 5 (for the test that opens it at another point)"""


@pytest.fixture(scope="module")
def opened(ps_api, ctx, co, pr, string):
    """Seventeen openings of one polynomial of 257 coefficients, and two openings of two other polynomials (5 and 2
    coefficients): (commit, z, y, proof) each."""
    tau_g1, _ = string
    rng = pr.SplitMix64(0x0FE2)
    out = _Items()
    for n, k in ((257, 17), (5, 1), (2, 1)):
        p = [rng.fr() for _ in range(n)]
        poly = ps_api.Poly.upload(ctx, p)
        commit = ps_api.KZGCommit(tau_g1, poly)
        zs = [rng.fr() for _ in range(k)]
        ys, proofs = ps_api.KZGOpen(tau_g1, poly, zs)
        out += [(commit, z, y, pi) for z, y, pi in zip(zs, ys, proofs)]
        if n == 5:
            out.coeffs5 = p
    return out


def _weights(pr, k, seed=0xBA7C4):
    rng = pr.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(k)]  # 128 bits each


def _batch(ps_api, ctx, t2, items, rhos, check_subgroup=True):
    return ps_api.KZGVerifyBatch(ctx, t2, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], rhos,
                                 check_subgroup)


def test_verifiers_accept_what_open_made(ps_api, ctx, pr, string, opened):
    _, t2 = string
    for commit, z, y, pi in opened:
        assert ps_api.KZGVerify(t2, commit, z, y, pi)
    for k in (1, 2, 17):
        assert _batch(ps_api, ctx, t2, opened[:k], _weights(pr, k))
    # polynomials and points all different, and a constant polynomial's identity proof among them
    mixed = [opened[0], opened[17], opened[18]]
    assert _batch(ps_api, ctx, t2, mixed, _weights(pr, 3))
    assert _batch(ps_api, ctx, t2, opened, _weights(pr, len(opened)), check_subgroup=False)
    assert _batch(ps_api, ctx, t2, [], [])


def test_verifiers_reject_every_single_change(ps_api, ctx, co, pr, string, opened):
    tau_g1, t2 = string
    commit, z, y, pi = opened[17]  # the polynomial of 5 coefficients
    other = opened[0]
    rng = pr.SplitMix64(0x5EED)
    p2 = [rng.fr() for _ in range(5)]
    commit2 = ps_api.KZGCommit(tau_g1, ps_api.Poly.upload(ctx, p2))  # a commitment of another polynomial
    z2 = (z + 1) % pr.R
    # a proof of another point of the SAME polynomial: open it again at z + 1
    _, (pi2,) = ps_api.KZGOpen(tau_g1, ps_api.Poly.upload(ctx, opened.coeffs5), [z2])
    t2_other = co.G2.to_b(co.G2.mul((TAU + 1) % pr.R))  # tau_g2_1 of another tau
    changes = {
        "y + 1": (t2, commit, z, (y + 1) % pr.R, pi),
        "z + 1": (t2, commit, z2, y, pi),
        "a proof of another point": (t2, commit, z, y, pi2),
        "a commitment of another polynomial": (t2, commit2, z, y, pi),
        "tau_g2_1 of another tau": (t2_other, commit, z, y, pi),
    }
    assert ps_api.KZGVerify(t2, commit, z, y, pi)
    rhos = _weights(pr, 2)
    for what, (tt, c, zz, yy, pp) in changes.items():
        assert not ps_api.KZGVerify(tt, c, zz, yy, pp), what
        for items in ([other, (c, zz, yy, pp)], [(c, zz, yy, pp), other]):
            assert not _batch(ps_api, ctx, tt, items, rhos), what
        assert not _batch(ps_api, ctx, tt, [(c, zz, yy, pp)], rhos[:1]), what


def test_a_cancelling_pair_passes_equal_weights_and_fails_random_ones(ps_api, ctx, pr, string, opened):
    """y_1 + d with y_2 - d leaves sum_j y_j alone: with all weights 1 the combined equation holds (so this test is sharp), with
    weights drawn after the fact it does not."""
    _, t2 = string
    d = 0x1234567
    a, b = opened[0], opened[17]
    pair = [(a[0], a[1], (a[2] + d) % pr.R, a[3]), (b[0], b[1], (b[2] - d) % pr.R, b[3])]
    assert not ps_api.KZGVerify(t2, *pair[0]) and not ps_api.KZGVerify(t2, *pair[1])
    assert _batch(ps_api, ctx, t2, pair, [1, 1])
    assert not _batch(ps_api, ctx, t2, pair, _weights(pr, 2))


def test_an_off_subgroup_commitment_is_rejected(ps_api, ctx, pr, string, opened, off_subgroup):
    _, t2 = string
    bad = pr.g1_to_bytes(off_subgroup[0])
    commit, z, y, pi = opened[17]
    assert not ps_api.KZGVerify(t2, bad, z, y, pi)
    assert not _batch(ps_api, ctx, t2, [opened[0], (bad, z, y, pi)], _weights(pr, 2), check_subgroup=True)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # not on the curve at all
        _batch(ps_api, ctx, t2, [(bad[:95] + bytes([bad[95] ^ 1]), z, y, pi)], [1])
    assert e.value.code == -3
    with pytest.raises(ps_api.PlaysnarkError) as e:  # a zero weight would skip an opening
        _batch(ps_api, ctx, t2, opened[:2], [1, 0])
    assert e.value.code == -5
