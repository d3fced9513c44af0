"""ps_pairing_product_is_one: prod_i e(P_i, Q_i) == 1 with the Miller loops and their product on the device
(csrc/pairing_dev.hpp) and one final exponentiation on the host.  Points P_i = a_i G1, Q_i = b_i G2 with host-known
scalars: the product is one iff sum a_i b_i = 0 (mod r).  Every compared quantity is a verdict or an error code."""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x70616972


def _upload(ps_api, ctx, a, b):
    g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, a))
    g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.upload(ctx, b))
    return g1, g2


def _scalars(pr, n, seed, identities=()):
    """a_i, b_i with sum a_i b_i = 0 (mod r).  identities: (index, slot) pairs, slot 1 = the G1 point is the identity
    (a_i = 0), slot 2 = the G2 point.  The sum is closed at an index that holds no identity."""
    rng = pr.SplitMix64(SEED + seed)
    a = [rng.fr() or 1 for _ in range(n)]
    b = [rng.fr() or 1 for _ in range(n)]
    for i, slot in identities:
        if slot == 1:
            a[i] = 0
        else:
            b[i] = 0
    free = [i for i in range(n) if i not in {k for k, _ in identities}]
    if free:
        k = free[-1]
        rest = sum(x * y for i, (x, y) in enumerate(zip(a, b)) if i != k) % pr.R
        a[k] = (-rest) * pow(b[k], pr.R - 2, pr.R) % pr.R
    return a, b, free


def _pairs(ps_api, ctx, pr, n, seed, break_one=False):
    a, b, free = _scalars(pr, n, seed)
    if break_one:
        a[n // 2] = (a[n // 2] + 1) % pr.R
    return _upload(ps_api, ctx, a, b)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 1000, 4097])
def test_product_is_one_iff_the_exponents_cancel(ps_api, ctx, pr, n):
    g1, g2 = _pairs(ps_api, ctx, pr, n, n)
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=False) is True
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=True) is True
    if n:
        g1, g2 = _pairs(ps_api, ctx, pr, n, n, break_one=True)
        assert ps_api.pairing_product_is_one(ctx, g1, g2, check=False) is False


@pytest.mark.parametrize("n", [3, 65, 1000])
@pytest.mark.parametrize("slot", [1, 2])
@pytest.mark.parametrize("place", ["first", "middle", "last", "all three"])
def test_identities_in_either_slot_do_not_change_the_verdict(ps_api, ctx, pr, n, slot, place):
    """An identity as the G1 point (slot 1) or as the G2 point (slot 2) of the first, a middle and the last pair contributes
    one: the verdict is that of the other pairs -- one when their exponents cancel, not one when one of them is off by 1."""
    index = {"first": [0], "middle": [n // 2], "last": [n - 1], "all three": [0, n // 2, n - 1]}[place]
    if place == "all three" and n == 3:
        index = [0, 2]  # leave one pair that is not an identity
    ids = [(i, slot if place != "all three" else 1 + (slot + k) % 2) for k, i in enumerate(index)]
    a, b, free = _scalars(pr, n, 100 + n, identities=ids)
    assert free and all((a[i] == 0) != (b[i] == 0) for i, _ in ids)
    g1, g2 = _upload(ps_api, ctx, a, b)
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=True) is True
    a[free[0]] = (a[free[0]] + 1) % pr.R
    g1, g2 = _upload(ps_api, ctx, a, b)
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=True) is False


def test_two_pairs_agree_with_pairing_equal_and_the_oracle(ps_api, ctx, co, pr):
    from oracle import pairing as pg

    rng = pr.SplitMix64(SEED + 2)
    a, b = rng.fr(), rng.fr()
    for c, d in ((b, a), ((a * b + 1) % pr.R, 1)):
        # e(aG1, bG2) * e(-cG1, dG2) == 1  <=>  e(aG1, bG2) == e(cG1, dG2)
        g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, [a, pr.R - c]))
        g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.upload(ctx, [b, d]))
        got = ps_api.pairing_product_is_one(ctx, g1, g2)
        P = [co.G1.to_b(co.G1.mul(a)), co.G1.to_b(co.G1.mul(c))]
        Q = [co.G2.to_b(co.G2.mul(b)), co.G2.to_b(co.G2.mul(d))]
        assert got == ps_api.pairing_equal(P[0], Q[0], P[1], Q[1])
        assert got == (pg.pair(pr.G1.mul(a), pr.G2.mul(b)) == pg.pair(pr.G1.mul(c), pr.G2.mul(d)))


def test_errors(ps_api, ctx, co, pr, off_subgroup):
    from playsnark_amd import _lib

    g1, g2 = _pairs(ps_api, ctx, pr, 4, 9)
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.pairing_product_is_one(ctx, g1.slice(0, 3), g2)
    bad1 = ps_api.Points.upload(ctx, ps_api.G1, co.G1.to_b(co.G1.mul(5)) + co.G1.to_b(off_subgroup[0]))
    ok2 = ps_api.Points.upload(ctx, ps_api.G2, co.G2.to_b(co.G2.mul(5)) + co.G2.to_b(co.G2.mul(6)))
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.pairing_product_is_one(ctx, bad1, ok2, check=True)
    assert e.value.code == _lib.PS_ERR_ENCODING
    ok1 = ps_api.Points.upload(ctx, ps_api.G1, co.G1.to_b(co.G1.mul(5)) + co.G1.to_b(co.G1.mul(6)))
    bad2 = ps_api.Points.upload(ctx, ps_api.G2, co.G2.to_b(off_subgroup[1]) + co.G2.to_b(co.G2.mul(6)))
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.pairing_product_is_one(ctx, ok1, bad2, check=True)
    assert e.value.code == _lib.PS_ERR_ENCODING
    with pytest.raises(ps_api.PlaysnarkError) as e:  # the groups the wrong way round
        ps_api.pairing_product_is_one(ctx, ok2, ok1)
    assert e.value.code == _lib.PS_ERR_ARG


def _device_simds():
    """SIMDs of device 0 (four per compute unit on CDNA, as verify_batch.inc counts them), asked in a child process"""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=300, check=True).stdout
    return 4 * int(out.split()[-1])


def _spread_lanes(n, simds):  # pairing_dev.hpp, restated
    return min(64, max(1, -(-n // max(simds, 1))))


@pytest.mark.parametrize("ragged", [False, True], ids=["full-waves", "ragged-last-wave"])
def test_full_waves_and_a_ragged_last_wave(ps_api, ctx, pr, ragged):
    """65 536 pairs fill every lane of 1 024 waves on 1 024 SIMDs, 70 001 leave a last wave of 49: the only shapes where
    k_miller_batch runs lpw = 64 through the API.  The device's SIMD count is read, and n grows with it."""
    simds = _device_simds()
    n = max(65536, 64 * simds) + (4465 if ragged else 0)
    assert _spread_lanes(n, simds) == 64 and (n % 64 != 0) == ragged
    a, b, free = _scalars(pr, n, 7000 + ragged)
    assert free[-1] == n - 1
    g1, g2 = _upload(ps_api, ctx, a, b)
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=False) is True
    last_wave = range((n - 1) // 64 * 64, n)
    k = last_wave[len(last_wave) // 2]  # one pair of the last wave
    a[k] = (a[k] + 1) % pr.R
    g1, g2 = _upload(ps_api, ctx, a, b)
    assert ps_api.pairing_product_is_one(ctx, g1, g2, check=False) is False
