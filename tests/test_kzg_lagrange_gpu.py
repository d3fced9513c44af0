"""GPU: KZG commitments and openings of polynomials given by their VALUES on the domain 1..n -- QAP.gate_values
(ps_qap_gate_values), Poly.EvalLagrange, Poly.DivLinearLagrange, KZGCommitLagrange, KZGOpenLagrange -- against routes that touch
none of the new kernels: the coefficients ps_qap_interpolate gives for the same values (a QAP whose left matrix is the identity
interpolates any vector; the coefficients are pinned by the oracle at sixteen nodes, and outright for n <= 9), the oracle's
Horner value and synthetic division, KZGCommit and KZGOpen of those coefficients byte for byte, and the oracle's scalar
multiplication [q(tau)] G1.  The string is held in the clear (tau known), in monomial and in Lagrange form.

Sizes: the smallest that reach every branch -- n = 1 (no quotient), 2, 5, 257 (two waves' worth, one partial tile), and both
sides of one and two tiles.  Points of a call: two random ones, 0, r - 1, n + 1 (just off the domain), and the nodes 1, n, T and
T + 1 where they exist, one of them twice: on- and off-domain points share every call."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61


def _tile():
    from playsnark_amd import _lib

    return _lib.lib.ps_poly_lagrange_tile()


T = _tile()
SIZES = [1, 2, 5, 257, T - 1, T, T + 1, 2 * T + 1]


def _g1(co, k):
    return co.G1.to_b(co.G1.mul(k))


def _points(pr, n, seed):
    rng = pr.SplitMix64(seed)
    zs = [rng.fr(), rng.fr(), 0, pr.R - 1, n + 1] + [m for m in (1, n, T, T + 1) if 1 <= m <= n]
    return zs + [zs[-1], zs[0]]  # a node and an off-domain point twice


def _synthetic_division(pr, p, z):
    """(q, y): p = q (X - z) + y, lowest degree first -- the oracle's Poly.Div by (1, -z), which works highest degree first"""
    q, rem = pr.poly_div(p[::-1], [1, (-z) % pr.R])
    return q[::-1], rem[0]


class _Case:
    pass


_CASES = {}


@pytest.fixture(scope="module")
def string(ps_api, ctx):
    """tau_g1: the 2T + 1 powers of tau in G1, on the device"""
    return ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.powers(ctx, TAU, 2 * T + 1))


@pytest.fixture(scope="module")
def case(ps_api, ctx, pr, string):
    """n -> the values, the identity QAP, the interpolated coefficients (device route without a new kernel, pinned by the
    oracle) and the Lagrange-form string in the clear; made once per n."""
    from oracle import restate as rs

    def make(n):
        if n in _CASES:
            return _CASES[n]
        c = _Case()
        rng = pr.SplitMix64(0x1A6 + n)
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
        c.tau_g1 = string.slice(0, n)
        _CASES[n] = c
        return c

    yield make
    _CASES.clear()


@pytest.mark.parametrize("n", SIZES)
def test_gate_values_are_the_oracles_matrix_vector_products(ps_api, ctx, pr, n):
    from oracle import restate as rs

    circuits = [rs.synthetic_circuit(n)] + ([rs.toy_circuit()] if n == SIZES[0] else [])
    for c, sol in circuits:
        sol = [s % pr.R for s in sol]
        qap = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
        w = ps_api.Poly.upload(ctx, sol)
        for which, want in enumerate(c.values(sol)):
            got = qap.gate_values(w, which)
            assert len(got) == c.nbGates
            assert got.download() == want, (n, which)


@pytest.mark.parametrize("n", SIZES)
def test_values_rows_commitment_and_proofs_against_the_coefficient_route(ps_api, ctx, co, pr, case, n):
    c = case(n)
    zs = _points(pr, n, 0x2B7 + n)
    want_y = [pr.poly_eval(c.p, z) for z in zs]
    assert c.values.EvalLagrange(c.qap, zs) == want_y, n
    qv, ys = c.values.DivLinearLagrange(c.qap, zs)
    assert ys == want_y and len(qv) == len(zs) * n
    nodes = list(range(1, n + 1))
    divided = [_synthetic_division(pr, c.p, z) for z in zs]
    for j, z in enumerate(zs):
        q, y = divided[j]
        assert y == want_y[j]
        if n == 1:
            want_row = [0]
        elif n <= 257:
            want_row = [pr.poly_eval(q, i) for i in nodes]
        else:  # the oracle's quotient, evaluated at the nodes by the coefficient-form scan
            want_row = ps_api.Poly.upload(ctx, q).Eval(nodes)
        assert qv.download(j * n, n) == want_row, (n, j, z)
    # the commitment and the proofs: the same group elements as the coefficient route's, hence the same bytes
    commit = ps_api.KZGCommitLagrange(c.lag_g1, c.values)
    assert commit == ps_api.KZGCommit(c.tau_g1, c.poly) == _g1(co, pr.poly_eval(c.p, TAU))
    ys2, proofs = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, zs)
    ys1, proofs1 = ps_api.KZGOpen(c.tau_g1, c.poly, zs)
    assert ys2 == ys1 == want_y
    assert proofs == proofs1, n
    for j, (q, _) in enumerate(divided):
        assert proofs[j] == _g1(co, pr.poly_eval(q, TAU)), (n, j)
    # one point alone takes the lone sum: on the domain and off it
    for z in (zs[0], n):
        (y,), (pi,) = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, [z])
        assert (y, pi) == (want_y[zs.index(z)], proofs[zs.index(z)]), (n, z)


def test_the_string_from_monomial_to_lagrange_is_the_clear_one_and_opens_the_same(ps_api, ctx, pr, case, string):
    c = case(33)
    lag = c.tau_g1.to_lagrange(c.qap, 0)
    assert lag.download() == c.lag_g1.download()
    zs = _points(pr, 33, 0x3C8)
    assert ps_api.KZGOpenLagrange(c.qap, lag, c.values, zs) == ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, zs)
    assert ps_api.KZGOpenLagrange(c.qap, lag, c.values, zs) == ps_api.KZGOpen(c.tau_g1, c.poly, zs)
    assert ps_api.KZGCommitLagrange(lag, c.values) == ps_api.KZGCommit(c.tau_g1, c.poly)


def test_a_circuits_gate_vectors_open_as_its_aggregate_polynomials_do(ps_api, ctx, pr, case, string):
    from oracle import restate as rs

    n = 257
    circ, sol = rs.synthetic_circuit(n)
    qap = ps_api.QAP(ctx, circ.nbVars, circ.nbIO, circ.left, circ.right, circ.out)
    w = ps_api.Poly.upload(ctx, [s % pr.R for s in sol])
    lag_g1, tau_g1 = case(n).lag_g1, string.slice(0, n)
    zs = _points(pr, n, 0x4D9)
    for which in range(3):
        values, coeffs = qap.gate_values(w, which), qap.interpolate(w, which)
        assert ps_api.KZGCommitLagrange(lag_g1, values) == ps_api.KZGCommit(tau_g1, coeffs), which
        assert ps_api.KZGOpenLagrange(qap, lag_g1, values, zs) == ps_api.KZGOpen(tau_g1, coeffs, zs), which


@pytest.mark.parametrize("n", [5, T + 1])
def test_range_edges_every_value_r_minus_1_and_every_value_zero(ps_api, ctx, co, pr, case, n):
    c = case(n)
    zs = [pr.R - 1, 0, n]
    top = ps_api.Poly.upload(ctx, [pr.R - 1] * n)  # the constant polynomial r - 1: its own value everywhere, quotient zero
    assert top.EvalLagrange(c.qap, zs) == [pr.R - 1] * 3
    qv, ys = top.DivLinearLagrange(c.qap, zs)
    assert ys == [pr.R - 1] * 3 and qv.download() == [0] * (3 * n)
    ys, proofs = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, top, zs)
    assert ys == [pr.R - 1] * 3 and proofs == [_g1(co, 0)] * 3
    assert ps_api.KZGCommitLagrange(c.lag_g1, top) == _g1(co, pr.R - 1)
    zero = ps_api.Poly.upload(ctx, [0] * n)
    qv, ys = zero.DivLinearLagrange(c.qap, zs)
    assert ys == [0] * 3 and qv.download() == [0] * (3 * n)
    ys, proofs = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, zero, zs)
    assert ys == [0] * 3 and proofs == [_g1(co, 0)] * 3
    assert ps_api.KZGCommitLagrange(c.lag_g1, zero) == _g1(co, 0)
    # every value r - 1 but one: a polynomial of full degree with values at the edge of the range
    v = [pr.R - 1] * n
    v[n // 2] = 0
    spike = ps_api.Poly.upload(ctx, v)
    coeffs = c.qap.interpolate(spike, 0)
    assert ps_api.KZGOpenLagrange(c.qap, c.lag_g1, spike, zs) == ps_api.KZGOpen(c.tau_g1, coeffs, zs)


def test_the_verifier_accepts_each_opening_and_rejects_each_change(ps_api, ctx, co, pr, case):
    n = 257
    c = case(n)
    t2 = co.G2.to_b(co.G2.mul(TAU))
    zs = _points(pr, n, 0x5EA)
    commit = ps_api.KZGCommitLagrange(c.lag_g1, c.values)
    ys, proofs = ps_api.KZGOpenLagrange(c.qap, c.lag_g1, c.values, zs)
    for z, y, pi in zip(zs, ys, proofs):
        assert ps_api.KZGVerify(t2, commit, z, y, pi), z
    for j in (0, zs.index(1), zs.index(n)):  # off the domain, and both ends of it
        z, y, pi = zs[j], ys[j], proofs[j]
        assert not ps_api.KZGVerify(t2, commit, z, (y + 1) % pr.R, pi), z
        assert not ps_api.KZGVerify(t2, commit, (z + 1) % pr.R, y, pi), z
        assert not ps_api.KZGVerify(t2, commit, z, y, proofs[zs.index(0)]), z  # the proof of another point
    rng = pr.SplitMix64(0x6FB)
    rhos = [rng.fr() or 1 for _ in zs]
    assert ps_api.KZGVerifyBatch(ctx, t2, [commit] * len(zs), zs, ys, proofs, rhos)
    ys_bad = list(ys)
    ys_bad[zs.index(n)] = (ys_bad[zs.index(n)] + 1) % pr.R
    assert not ps_api.KZGVerifyBatch(ctx, t2, [commit] * len(zs), zs, ys_bad, proofs, rhos)


def test_each_error_rule_returns_its_code_and_names_the_entry(ps_api, ctx, pr, case):
    import ctypes as C

    from playsnark_amd import _lib

    lib = _lib.lib
    c = case(5)
    n = 5
    g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.powers(ctx, TAU, n))
    short, long_ = c.values.slice(0, n - 1), ps_api.Poly.upload(ctx, c.v + [1])
    zb = lambda zs: b"".join(int(z).to_bytes(32, "big") for z in zs)
    y, pf, out = C.create_string_buffer(64), C.create_string_buffer(192), C.create_string_buffer(96)
    h = C.c_void_p()

    def calls(values, lag, z, k, q=c.qap._h):
        return {
            "ps_poly_eval_lagrange": lambda: lib.ps_poly_eval_lagrange(ctx._h, q, values, z, k, y),
            "ps_poly_div_linear_lagrange": lambda: lib.ps_poly_div_linear_lagrange(ctx._h, q, values, z, k, C.byref(h), y),
            "ps_kzg_open_lagrange": lambda: lib.ps_kzg_open_lagrange(ctx._h, q, lag, values, z, k, y, pf),
        }

    def expect(call, name, code):
        assert call() == code, name
        assert name in lib.ps_last_error().decode(), (name, lib.ps_last_error())

    two = zb([7, 3])
    for vals in (short, long_):  # values not exactly n long
        for name, call in calls(vals._h, c.lag_g1._h, two, 2).items():
            expect(call, name, _lib.PS_ERR_LENGTH)
    head = c.lag_g1.slice(0, n - 1)  # (held: a temporary would be freed before the call)
    expect(lambda: lib.ps_kzg_open_lagrange(ctx._h, c.qap._h, head._h, c.values._h, two, 2, y, pf), "ps_kzg_open_lagrange", _lib.PS_ERR_LENGTH)
    expect(lambda: lib.ps_kzg_commit_lagrange(ctx._h, c.lag_g1._h, short._h, out), "ps_kzg_commit_lagrange", _lib.PS_ERR_LENGTH)
    expect(lambda: lib.ps_kzg_commit_lagrange(ctx._h, g2._h, c.values._h, out), "ps_kzg_commit_lagrange", _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_kzg_open_lagrange(ctx._h, c.qap._h, g2._h, c.values._h, two, 2, y, pf), "ps_kzg_open_lagrange", _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, None, 2).items():  # NULL points
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(None, c.lag_g1._h, two, 2).items():  # NULL values
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, two, 2, q=None).items():  # NULL domain
        expect(call, name, _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_kzg_commit_lagrange(ctx._h, c.lag_g1._h, c.values._h, None), "ps_kzg_commit_lagrange", _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_qap_gate_values(ctx._h, c.qap._h, c.values._h, 3, C.byref(h)), "ps_qap_gate_values", _lib.PS_ERR_ARG)
    expect(lambda: lib.ps_qap_gate_values(ctx._h, c.qap._h, None, 0, C.byref(h)), "ps_qap_gate_values", _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, None, (1 << 32) // n + 1).items():  # the NULL check comes first ...
        expect(call, name, _lib.PS_ERR_ARG)
    for name, call in calls(c.values._h, c.lag_g1._h, two, (1 << 32) // n + 1).items():  # ... then k * n >= 2^32, before z is read
        expect(call, name, _lib.PS_ERR_ARG)
        assert "2^32" in lib.ps_last_error().decode()
    for name, call in calls(c.values._h, c.lag_g1._h, zb([7, pr.R]), 2).items():  # z not below r
        expect(call, name, _lib.PS_ERR_ENCODING)
        assert "z[1]" in lib.ps_last_error().decode()
    # k = 0: PS_OK and nothing written
    y.raw = b"\xAA" * 64
    pf.raw = b"\xBB" * 192
    assert lib.ps_poly_eval_lagrange(ctx._h, c.qap._h, c.values._h, None, 0, None) == _lib.PS_OK
    assert lib.ps_kzg_open_lagrange(ctx._h, c.qap._h, c.lag_g1._h, c.values._h, None, 0, y, pf) == _lib.PS_OK
    assert y.raw == b"\xAA" * 64 and pf.raw == b"\xBB" * 192
    qv, ys = c.values.DivLinearLagrange(c.qap, [])
    assert len(qv) == 0 and ys == []
    # a sum pending on the context
    ps_api.msm_launch(ctx, c.lag_g1, c.values)
    try:
        expect(lambda: lib.ps_kzg_commit_lagrange(ctx._h, c.lag_g1._h, c.values._h, out), "ps_kzg_commit_lagrange", _lib.PS_ERR_ARG)
        expect(lambda: lib.ps_kzg_open_lagrange(ctx._h, c.qap._h, c.lag_g1._h, c.values._h, two, 2, y, pf), "ps_kzg_open_lagrange", _lib.PS_ERR_ARG)
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)
    # the Python surface maps the codes
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.KZGOpenLagrange(c.qap, c.lag_g1, short, [7])
    with pytest.raises(ps_api.PlaysnarkError) as e:
        c.values.EvalLagrange(c.qap, [pr.R])
    assert e.value.code == -3 and "ps_poly_eval_lagrange" in str(e.value)
