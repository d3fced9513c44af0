"""GPU: the KZG proofs of EVERY node of the domain in one call -- KZGAllKeyLagrange (ps_kzg_all_key_lagrange) and
KZGOpenAllLagrange (ps_kzg_open_all_lagrange) -- with tau held in the clear, as the other KZG tests hold it.  Byte for byte
against (a) the oracle's scalar multiplication [(p(tau) - v_m) / (tau - m)] G1 with p(tau) = sum_i v_i l_i(tau) in Python
integers, (b) KZGOpenLagrange at the same nodes, which runs none of the new kernels, and (c), for the key table,
[sum_i l_i(tau) / (m - i)] G1.  A table read backwards would give the NEGATED points (kappa is antisymmetric): (a) and (c) are
signed values, so that is caught.

Sizes: n in {1, 2, 3, 5, 64, 65, 128, 129, 256, 257, 1025, 4097} -- both sides of the transform size S = 2^p >= 2n - 1 doubling,
the one-pass / two-pass edge of the scalar transform at p = 9 / 10, and p = 14.  Every node is checked for n <= 257; beyond, 64
nodes: 1, n and a fixed multiplicative-hash sample.  Further: all_key = None gives the bytes of the tabled call, two calls in a
row give the same bytes, a slice view as `values` gives the same bytes; value vectors at n = 5, 65, 257 (all zero and constant,
where every proof is the identity; the values of aX + b, where every proof is [a] G1; one-hot at node 1 and at node n; every
value r - 1); a string with identity entries; KZGVerifyBatch over all n openings at n = 257; every error rule a device can
reach (the limit n <= 2^30 is beyond any device's memory: tests/test_kzg_all_plan_host.py holds it)."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
SIZES = [1, 2, 3, 5, 64, 65, 128, 129, 256, 257, 1025, 4097]
VECTOR_SIZES = [5, 65, 257]


def _g1(co, k):
    return co.G1.to_b(co.G1.mul(k))


def _sample(n):
    if n <= 257:
        return list(range(1, n + 1))
    want, i = [1, n], 0
    while len(set(want)) < 64:
        want.append(1 + (i * 2654435761) % n)
        i += 1
    return sorted(set(want))


def _split(points):
    raw = points.download()
    assert len(raw) == 96 * len(points)
    return [raw[96 * m : 96 * m + 96] for m in range(len(points))]


def _proof_scalars(pr, v, lag, tau, nodes):
    """(p(tau) - v_m) / (tau - m) for m in nodes, p(tau) = sum_i v_i l_i(tau); tau is no node"""
    pt = sum(a * b for a, b in zip(v, lag)) % pr.R
    return [(pt - v[m - 1]) * pr.fr_inv((tau - m) % pr.R) % pr.R for m in nodes]


class _Case:
    pass


_CASES = {}


@pytest.fixture(scope="module")
def case(ps_api, ctx, pr, co):
    """n -> the identity QAP, random values, the Lagrange-form string in the clear and on the device, the key table and the
    proofs of the tabled call; made once per n and left unchanged."""
    from oracle import restate as rs

    def make(n):
        if n in _CASES:
            return _CASES[n]
        c = _Case()
        rng = pr.SplitMix64(0xA77 + n)
        c.n = n
        c.v = [rng.fr() for _ in range(n)]
        ident = [[(i, 1)] for i in range(n)]
        const = [[(0, 1)] for _ in range(n)]
        c.qap = ps_api.QAP(ctx, n, 1, ident, const, const)
        c.values = ps_api.Poly.upload(ctx, c.v)
        c.lag = rs.lagrange_at(n, TAU)[0]
        c.lag_g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, c.lag))
        c.key = ps_api.KZGAllKeyLagrange(c.qap, c.lag_g1)
        c.proofs = ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, c.values, c.key)
        c.nodes = _sample(n)
        _CASES[n] = c
        return c

    yield make
    _CASES.clear()


@pytest.mark.parametrize("n", SIZES)
def test_proofs_against_the_oracle_and_the_single_point_openings(ps_api, ctx, co, pr, case, n):
    c = case(n)
    assert len(c.proofs) == n and c.proofs.group == ps_api.G1
    got = _split(c.proofs)
    want = _proof_scalars(pr, c.v, c.lag, TAU, c.nodes)
    for m, k in zip(c.nodes, want):
        assert got[m - 1] == _g1(co, k), (n, m)  # (a)
    ys, single = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, c.nodes)  # (b)
    assert ys == [c.v[m - 1] for m in c.nodes]
    assert [got[m - 1] for m in c.nodes] == single, n
    if n == 1:
        assert got == [_g1(co, 0)]


@pytest.mark.parametrize("n", SIZES)
def test_key_table_against_the_signed_sums(ps_api, co, pr, case, n):
    c = case(n)
    assert len(c.key) == n and c.key.group == ps_api.G1
    got = _split(c.key)
    inv = [0] + [pr.fr_inv(d) for d in range(1, n)]
    for m in c.nodes:
        k = sum((inv[m - i] if m > i else -inv[i - m]) * c.lag[i - 1] for i in range(1, n + 1) if i != m) % pr.R
        assert got[m - 1] == _g1(co, k), (n, m)  # (c)
        if n > 1:
            assert got[m - 1] != _g1(co, (-k) % pr.R)


@pytest.mark.parametrize("n", SIZES)
def test_without_the_table_twice_in_a_row_and_from_a_slice_view(ps_api, ctx, case, n):
    c = case(n)
    want = c.proofs.download()
    assert ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, c.values).download() == want  # all_key = NULL
    assert ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, c.values, c.key).download() == want  # again
    assert ps_api.KZGAllKeyLagrange(c.qap, c.lag_g1).download() == c.key.download()
    wide = ps_api.Poly.upload(ctx, [7] + c.v + [9])
    view = wide.slice(1, n)
    assert ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, view, c.key).download() == want


@pytest.mark.parametrize("n", VECTOR_SIZES)
def test_value_vectors_at_the_edges(ps_api, ctx, co, pr, case, n):
    c = case(n)
    R = pr.R
    rng = pr.SplitMix64(0xA78 + n)
    a, b = rng.fr(), rng.fr()
    spike1, spiken = [0] * n, [0] * n
    spike1[0], spiken[n - 1] = rng.fr(), rng.fr()
    vectors = {
        "zero": [0] * n,
        "constant": [b] * n,
        "line": [(a * i + b) % R for i in range(1, n + 1)],
        "one-hot at 1": spike1,
        "one-hot at n": spiken,
        "all r - 1": [R - 1] * n,
    }
    ident = _g1(co, 0)
    for name, v in vectors.items():
        got = _split(ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, ps_api.Poly.upload(ctx, v), c.key))
        want = _proof_scalars(pr, v, c.lag, TAU, range(1, n + 1))
        if name in ("zero", "constant", "all r - 1"):
            assert want == [0] * n and got == [ident] * n, (n, name)  # the additions cancel to the identity
        elif name == "line":
            assert want == [a] * n and got == [_g1(co, a)] * n, (n, name)
        else:
            assert got == [_g1(co, k) for k in want], (n, name)


def test_a_string_with_identity_entries(ps_api, ctx, co, pr, case):
    """tau = 3 is a node of the domain 1..5: l_i(3) is 1 at i = 3 and 0 elsewhere, so four of the five points are the identity"""
    n, tau = 5, 3
    c = case(n)
    R = pr.R
    lag = [0, 0, 1, 0, 0]
    lag_g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, lag))
    assert _split(lag_g1)[0] == _g1(co, 0) and _split(lag_g1)[2] == _g1(co, 1)
    p = (pr.interpolate(c.v) + [0] * n)[:n]
    deriv = sum(k * p[k] * pow(tau, k - 1, R) for k in range(1, n)) % R
    want = [deriv if m == tau else (c.v[tau - 1] - c.v[m - 1]) * pr.fr_inv((tau - m) % R) % R for m in range(1, n + 1)]
    key = ps_api.KZGAllKeyLagrange(c.qap, lag_g1)
    assert _split(key) == [_g1(co, pr.fr_inv((m - tau) % R) if m != tau else 0) for m in range(1, n + 1)]
    for k in (key, None):
        assert _split(ps_api.KZGOpenAllLagrange(c.qap, lag_g1, c.values, k)) == [_g1(co, s) for s in want]


def test_the_batch_verifier_accepts_all_openings_and_rejects_a_changed_value(ps_api, ctx, pr, case):
    n = 257
    c = case(n)
    tau_g2_1 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, 2)).download(1, 1)
    commit = ps_api.KZGCommitLagrange(c.lag_g1, c.values)
    proofs = _split(c.proofs)
    rng = pr.SplitMix64(0xA79)
    rhos = [1 + rng.fr() % ((1 << 128) - 1) for _ in range(n)]
    zs = list(range(1, n + 1))
    assert ps_api.KZGVerifyBatch(ctx, tau_g2_1, [commit] * n, zs, c.v, proofs, rhos)
    bad = list(c.v)
    bad[n // 2] = (bad[n // 2] + 1) % pr.R
    assert not ps_api.KZGVerifyBatch(ctx, tau_g2_1, [commit] * n, zs, bad, proofs, rhos)
    assert ps_api.KZGVerify(tau_g2_1, commit, n, c.v[n - 1], proofs[n - 1])


def test_each_error_rule_returns_its_code_and_names_the_entry(ps_api, ctx, pr, case):
    import ctypes as C

    from playsnark_amd import _lib

    lib = _lib.lib
    n = 5
    c = case(n)
    g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, n))
    short_v, long_v = c.values.slice(0, n - 1), ps_api.Poly.upload(ctx, c.v + [1])
    short_l, short_k = c.lag_g1.slice(0, n - 1), c.key.slice(0, n - 1)  # (held: a temporary would be freed before the call)
    long_l = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, c.lag + [1]))
    h = C.c_void_p()

    def key(q=c.qap._h, lag=c.lag_g1._h, out=C.byref(h), cx=ctx._h):
        return lambda: lib.ps_kzg_all_key_lagrange(cx, q, lag, out)

    def opn(q=c.qap._h, lag=c.lag_g1._h, k=c.key._h, v=c.values._h, out=C.byref(h), cx=ctx._h):
        return lambda: lib.ps_kzg_open_all_lagrange(cx, q, lag, k, v, out)

    def expect(call, name, code):
        h.value = 0xDEAD
        assert call() == code, name
        assert name in lib.ps_last_error().decode(), (name, lib.ps_last_error())

    K, O = "ps_kzg_all_key_lagrange", "ps_kzg_open_all_lagrange"
    # lengths: values, lag_g1 and all_key hold exactly n elements
    for v in (short_v, long_v):
        expect(opn(v=v._h), O, _lib.PS_ERR_LENGTH)
    for lag in (short_l, long_l):
        expect(opn(lag=lag._h), O, _lib.PS_ERR_LENGTH)
        expect(key(lag=lag._h), K, _lib.PS_ERR_LENGTH)
    expect(opn(k=short_k._h), O, _lib.PS_ERR_LENGTH)
    assert h.value is None  # the output is nulled on an error
    # a G2 array
    expect(opn(lag=g2._h), O, _lib.PS_ERR_ARG)
    expect(opn(k=g2._h), O, _lib.PS_ERR_ARG)
    expect(key(lag=g2._h), K, _lib.PS_ERR_ARG)
    # NULL arguments (all_key alone may be NULL)
    for call in (opn(cx=None), opn(q=None), opn(lag=None), opn(v=None), opn(out=None)):
        expect(call, O, _lib.PS_ERR_ARG)
        assert "NULL argument" in lib.ps_last_error().decode()
    for call in (key(cx=None), key(q=None), key(lag=None), key(out=None)):
        expect(call, K, _lib.PS_ERR_ARG)
        assert "NULL argument" in lib.ps_last_error().decode()
    # the Python surface maps the codes
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, short_v, c.key)
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.KZGAllKeyLagrange(c.qap, short_l)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.KZGOpenAllLagrange(c.qap, g2, c.values)
    assert e.value.code == _lib.PS_ERR_ARG and O in str(e.value)
    # and a good call still works afterwards
    assert ps_api.KZGOpenAllLagrange(c.qap, c.lag_g1, c.values, c.key).download() == c.proofs.download()
