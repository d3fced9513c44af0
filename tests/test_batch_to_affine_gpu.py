"""k_batch_to_affine (Montgomery's trick over T = max(1, n / 16) strided chains, one thread per chain) with identities where
the chains are sensitive to them, through Points.from_scalars: a zero scalar gives the identity, whose key (ZZ * ZZZ) is zero
and must be skipped by the running product, not multiplied into it.

n = 1, 15 (one chain, shorter than 16), 16, 17 (one chain of 16 / 17), 33 (two chains: 17 and 16 points), 300 (18 chains,
unequal lengths), 4112 (257 chains: the 257th is thread 0 of a second block).  Every point against the C oracle's Mul."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 33, 300, 4112]
PATTERNS = ["all", "chain0", "last", "first", "odd"]


def _is_zero(pattern, i, n):
    T = max(1, n // 16)
    return {"all": True, "chain0": i % T == 0, "last": i == n - 1, "first": i == 0, "odd": i % 2 == 1}[pattern]


@pytest.fixture(scope="module")
def products(co, pr):
    """{(group, n): (scalars, [k_i G])}: non-zero scalars, most below 2^16 (a quick oracle), every 37th full width; made once
    per size and shared by the patterns, which only put zeros in"""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            rng = pr.SplitMix64(0xBA7C4 + n + (1 << 20) * (name == "g2"))
            ks = [rng.fr() if i % 37 == 5 else 1 + rng.next() % 0xFFFF for i in range(n)]
            og = co.G1 if name == "g1" else co.G2
            cache[name, n] = (ks, [og.to_b(og.mul(k)) for k in ks])
        return cache[name, n]

    return get


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_fixed_base_points_with_identities_in_the_chains(ps_api, ctx, co, products, name, n, pattern):
    gid, og = (ps_api.G1, co.G1) if name == "g1" else (ps_api.G2, co.G2)
    ks, want = products(name, n)
    zero = [_is_zero(pattern, i, n) for i in range(n)]
    if pattern == "chain0" and n >= 32:
        T = n // 16
        assert all(zero[i] for i in range(0, n, T)) and not any(zero[i] for i in range(n) if i % T)  # chain 0, nothing else
    pts = ps_api.Points.from_scalars(ctx, gid, ps_api.Poly.upload(ctx, [0 if z else k for k, z in zip(ks, zero)]))
    got = pts.download()
    ident = og.to_b(None)
    bad = [i for i in range(n) if got[i * og.nb:(i + 1) * og.nb] != (ident if zero[i] else want[i])]
    assert not bad, bad[:20]
