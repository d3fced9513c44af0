"""GPU: ONE KZG proof for a set of points of a polynomial given by its VALUES on the domain 1..n -- Poly.DivRootsLagrange
(ps_poly_div_roots_lagrange) and KZGOpenSetLagrange (ps_kzg_open_set_lagrange) -- against a route that touches none of the new
kernels: the identity-matrix QAP of tests/test_kzg_lagrange_gpu.py, whose ps_qap_interpolate coefficients are pinned by the
oracle as there, divided by Z_S with the oracle's Poly.Div.  Checked: the values against the oracle's Horner; the row of
quotient values against the oracle quotient evaluated at the nodes (every node for n <= 257; beyond, 64 nodes that hold every
hit, both sides of every tile edge, 1 and n); the remainder; the proof byte for byte against KZGOpenSet of the coefficients AND
against the oracle's scalar multiplication [q(tau)] G1, the string being held in the clear; KZGVerifySet accepts it and rejects
it with one value changed.

Sizes, with T = ps_poly_lagrange_tile() and G = ps_poly_lagrange_set_group(): n in {1, 2, 5, 257, T - 1, T, T + 1, 2T + 1} and
k in {1, 2, G - 1, G, G + 1, 2G + 1} where k <= n + 2 -- and k = n - 1, n, n + 1 at n = 5 whatever G is.  Point sets of every
(n, k): all off the domain (0, r - 1 and n + 1 among them), all nodes, mixed with hits at 1, n, T and T + 1 where they exist, a
hit in every group, and a group made of hits only."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61


def _consts():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_lagrange_tile(), _lib.lib.ps_poly_lagrange_set_group()


T, G = _consts()
SIZES = [1, 2, 5, 257, T - 1, T, T + 1, 2 * T + 1]
KS = sorted({1, 2, G - 1, G, G + 1, 2 * G + 1} - {0})
KMAX = max(KS + [6])


def _ks(n):
    return [k for k in sorted(set(KS) | ({n - 1, n, n + 1} if n == 5 else set())) if 1 <= k <= n + 2]


def _g1(co, k):
    return co.G1.to_b(co.G1.mul(k))


def _nodes_pool(n):
    """distinct nodes of the domain, the tile edges first"""
    pool = []
    for m in [1, n, T, T + 1, 2, n - 1, 2 * T, 2 * T + 1] + [1 + (i * 2654435761) % n for i in range(4 * KMAX)]:
        if 1 <= m <= n and m not in pool:
            pool.append(m)
    return pool


def _off_pool(pr, n, seed):
    rng = pr.SplitMix64(seed)
    return [0, pr.R - 1, n + 1] + [rng.fr() for _ in range(KMAX)]


def _fill(k, is_node, nodes, off):
    """k distinct points: position i takes the next node where is_node(i) and one is left, else the next off-domain point"""
    nodes, off, zs = list(nodes), list(off), []
    for i in range(k):
        zs.append(nodes.pop(0) if is_node(i) and nodes else off.pop(0))
    assert len(set(zs)) == k
    return zs


def _point_sets(pr, n, k):
    nodes, off = _nodes_pool(n), _off_pool(pr, n, 0x5E7 + 31 * n + k)
    hits_group = 1 if k > G else 0
    sets = {
        "off": _fill(k, lambda i: False, nodes, off[k % 3 :] + off[: k % 3] if k < 3 else off),
        "nodes": _fill(k, lambda i: True, nodes, off),
        "mixed": _fill(k, lambda i: i % 2 == 1, nodes, off),
        "hit per group": _fill(k, lambda i: i % G == (i // G) % G, nodes, off),
        "group of hits": _fill(k, lambda i: i // G == hits_group, nodes, off),
    }
    return sets


def _vanishing(pr, zs):
    zp = [1]
    for z in zs:
        zp = pr.poly_mul(zp, [(-z) % pr.R, 1])
    return zp


def _divide(pr, p, zs):
    """(q, rem), lowest degree first: p = q Z_S + rem, q of len(p) - len(zs) coefficients and rem of len(zs) -- the oracle's
    Poly.Div, which works highest degree first; a polynomial no longer than the set is its own remainder"""
    if len(p) <= len(zs):
        return [], p + [0] * (len(zs) - len(p))
    q, rem = pr.poly_div(p[::-1], _vanishing(pr, zs)[::-1])
    return q[::-1], rem[::-1]


def _sample(n, zs):
    if n <= 257:
        return list(range(1, n + 1))
    want = [1, n] + [z for z in zs if 1 <= z <= n] + [m for b in range(1, n // T + 1) for m in (b * T, b * T + 1) if m <= n]
    i = 0
    while len(set(want)) < 64:
        want.append(1 + (i * 2654435761) % n)
        i += 1
    return sorted(set(want))


class _Case:
    pass


_CASES = {}


@pytest.fixture(scope="module")
def string(ps_api, ctx):
    """tau_g1 (2T + 1 powers of tau in G1) and tau_g2 (KMAX + 1 in G2), on the device"""
    return (ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.powers(ctx, TAU, 2 * T + 1)),
            ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, KMAX + 1)))


@pytest.fixture(scope="module")
def case(ps_api, ctx, pr, string):
    """n -> the values, the identity QAP, the interpolated coefficients (device route without a new kernel, pinned by the
    oracle) and the Lagrange-form string in the clear; made once per n."""
    from oracle import restate as rs

    def make(n):
        if n in _CASES:
            return _CASES[n]
        c = _Case()
        rng = pr.SplitMix64(0x7C1 + n)
        c.n = n
        c.v = [rng.fr() for _ in range(n)]
        ident = [[(i, 1)] for i in range(n)]
        const = [[(0, 1)] for _ in range(n)]
        c.qap = ps_api.QAP(ctx, n, 1, ident, const, const)
        c.values = ps_api.Poly.upload(ctx, c.v)
        c.poly = c.qap.interpolate(c.values, 0)
        c.p = c.poly.download()
        assert len(c.p) == n
        nodes = sorted({1, 2, n, n - 1, T, T + 1, 2 * T} | {1 + (i * 2654435761) % n for i in range(9)})
        for i in [m for m in nodes if 1 <= m <= n][:16]:
            assert pr.poly_eval(c.p, i) == c.v[i - 1], (n, i)
        if n <= 9:
            assert c.p == (pr.interpolate(c.v) + [0] * n)[:n]
        c.lag_g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, rs.lagrange_at(n, TAU)[0]))
        c.tau_g1 = string[0].slice(0, n)
        c.commit = ps_api.KZGCommitLagrange(c.lag_g1, c.values)
        _CASES[n] = c
        return c

    yield make
    _CASES.clear()


def _check(ps_api, ctx, co, pr, string, c, values, p, commit, zs, what):
    n, k = c.n, len(zs)
    q, rem = _divide(pr, p, zs)
    want_y = [pr.poly_eval(p, z) for z in zs]
    qv, ys, got_rem = values.DivRootsLagrange(c.qap, zs)
    assert ys == want_y, what
    assert got_rem == rem, what
    assert len(qv) == n
    at = _sample(n, zs)
    row = qv.download()
    assert [row[i - 1] for i in at] == [pr.poly_eval(q, i) for i in at], what
    if k >= n:
        assert row == [0] * n, what
    assert values.DivRootsLagrange(c.qap, zs, remainder=False)[2] is None
    ys2, proof = ps_api.KZGOpenSetLagrange(c.qap, c.lag_g1, values, zs)
    assert ys2 == want_y, what
    assert proof == _g1(co, pr.poly_eval(q, TAU)), what
    assert (ys2, proof) == ps_api.KZGOpenSet(c.tau_g1, ps_api.Poly.upload(ctx, p), zs), what
    tau_g1, tau_g2 = string
    assert ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, commit, zs, ys2, proof), what
    bad = list(ys2)
    bad[k // 2] = (bad[k // 2] + 1) % pr.R
    assert not ps_api.KZGVerifySet(ctx, tau_g1, tau_g2, commit, zs, bad, proof), what
    return ys2, proof


@pytest.mark.parametrize("n,k", [(n, k) for n in SIZES for k in _ks(n)])
def test_values_row_remainder_and_proof_against_the_coefficient_route(ps_api, ctx, co, pr, string, case, n, k):
    c = case(n)
    for name, zs in _point_sets(pr, n, k).items():
        ys, proof = _check(ps_api, ctx, co, pr, string, c, c.values, c.p, c.commit, zs, (n, k, name))
        if k == 1:  # one point: the single-point opening's bytes
            assert ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, zs) == (ys, [proof]), (n, name)


@pytest.mark.parametrize("n", [5, T + 1])
def test_range_edges_every_value_r_minus_1_and_every_value_zero(ps_api, ctx, co, pr, string, case, n):
    c = case(n)
    zs = _point_sets(pr, n, G + 1)["mixed"]
    k = len(zs)
    for const in (pr.R - 1, 0):  # a constant polynomial: its own value everywhere, quotient zero
        values = ps_api.Poly.upload(ctx, [const] * n)
        qv, ys, rem = values.DivRootsLagrange(c.qap, zs)
        assert ys == [const] * k and qv.download() == [0] * n and rem == [const] + [0] * (k - 1)
        assert ps_api.KZGOpenSetLagrange(c.qap, c.lag_g1, values, zs) == ([const] * k, _g1(co, 0))
    # every value r - 1 but one: a polynomial of full degree with values at the edge of the range
    v = [pr.R - 1] * n
    v[n // 2] = 0
    spike = ps_api.Poly.upload(ctx, v)
    p = c.qap.interpolate(spike, 0).download()
    _check(ps_api, ctx, co, pr, string, c, spike, p, ps_api.KZGCommitLagrange(c.lag_g1, spike), zs, (n, "spike"))


def test_each_error_rule_returns_its_code_and_names_the_entry(ps_api, ctx, pr, case):
    import ctypes as C

    from playsnark_amd import _lib

    lib = _lib.lib
    n = 5
    c = case(n)
    g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, n))
    short, long_ = c.values.slice(0, n - 1), ps_api.Poly.upload(ctx, c.v + [1])
    zb = lambda zs: b"".join(int(z).to_bytes(32, "big") for z in zs)
    y, rem, pf = C.create_string_buffer(32 * 4), C.create_string_buffer(32 * 4), C.create_string_buffer(96)
    h = C.c_void_p()

    def calls(values, lag, z, k, q=c.qap._h):
        return {
            "ps_poly_div_roots_lagrange": lambda: lib.ps_poly_div_roots_lagrange(ctx._h, q, values, z, k, C.byref(h), y, rem),
            "ps_kzg_open_set_lagrange": lambda: lib.ps_kzg_open_set_lagrange(ctx._h, q, lag, values, z, k, y, pf),
        }

    def expect(call, name, code):
        assert call() == code, name
        assert name in lib.ps_last_error().decode(), (name, lib.ps_last_error())

    two = zb([7, 3])
    for name, call in calls(c.values._h, c.lag_g1._h, zb([7, 3, 7]), 3).items():  # repeated points: both indices named
        expect(call, name, _lib.PS_ERR_ARG)
        assert "z[0]" in lib.ps_last_error().decode() and "z[2]" in lib.ps_last_error().decode()
    for name, call in calls(c.values._h, c.lag_g1._h, zb([2, 9, 2]), 3).items():  # ... on the domain too
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, two, 0).items():  # an empty set
        expect(call, name, _lib.PS_ERR_ARG)
    for vals in (short, long_):  # values not exactly n long
        for name, call in calls(vals._h, c.lag_g1._h, two, 2).items():
            expect(call, name, _lib.PS_ERR_LENGTH)
    head = c.lag_g1.slice(0, n - 1)  # (held: a temporary would be freed before the call)
    expect(lambda: lib.ps_kzg_open_set_lagrange(ctx._h, c.qap._h, head._h, c.values._h, two, 2, y, pf), "ps_kzg_open_set_lagrange", _lib.PS_ERR_LENGTH)
    for name, call in calls(c.values._h, c.lag_g1._h, zb([7, pr.R]), 2).items():  # z not below r
        expect(call, name, _lib.PS_ERR_ENCODING)
        assert "z[1]" in lib.ps_last_error().decode()
    expect(lambda: lib.ps_kzg_open_set_lagrange(ctx._h, c.qap._h, g2._h, c.values._h, two, 2, y, pf), "ps_kzg_open_set_lagrange", _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, None, 2).items():  # NULL points
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(None, c.lag_g1._h, two, 2).items():  # NULL values
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, two, 2, q=None).items():  # NULL domain
        expect(call, name, _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_poly_div_roots_lagrange(ctx._h, c.qap._h, c.values._h, two, 2, None, y, rem), "ps_poly_div_roots_lagrange", _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_kzg_open_set_lagrange(ctx._h, c.qap._h, c.lag_g1._h, c.values._h, two, 2, y, None), "ps_kzg_open_set_lagrange", _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, two, 1025).items():  # more than 1024 points, before z is read
        expect(call, name, _lib.PS_ERR_ARG)
        assert "1024" in lib.ps_last_error().decode()
    # a sum pending on the context
    ps_api.msm_launch(ctx, c.lag_g1, c.values)
    try:
        expect(lambda: lib.ps_kzg_open_set_lagrange(ctx._h, c.qap._h, c.lag_g1._h, c.values._h, two, 2, y, pf), "ps_kzg_open_set_lagrange", _lib.PS_ERR_ARG)
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    # the Python surface maps the codes
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.KZGOpenSetLagrange(c.qap, c.lag_g1, short, [7])
    with pytest.raises(ps_api.PlaysnarkError) as e:
        c.values.DivRootsLagrange(c.qap, [pr.R])
    assert e.value.code == -3 and "ps_poly_div_roots_lagrange" in str(e.value)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.KZGOpenSetLagrange(c.qap, c.lag_g1, c.values, [3, 3])
    assert e.value.code == -5
