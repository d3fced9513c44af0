"""GPU: many polynomials at shared points -- Poly.LinComb / Add / Sub (ps_scalars_lincomb), KZGOpenMulti and KZGVerifyMulti --
over the in-the-clear string of tests/test_kzg_gpu.py (tau known, T + 1 + 3 points).  Linear combinations are compared word for
word with Python integers mod r; proofs byte for byte with the oracle's [q_j(tau)] G1 and with the composed route (LinComb,
DivLinear, BlindEval); the verifier accepts what KZGOpenMulti made and rejects each single change, every changed point still
in the subgroup."""
import pytest

pytestmark = pytest.mark.gpu

TAU = 0x1F3D5B79A2C4E6F81B3D5F7092B4D6F8A1C3E5079B2D4F6183A5C7E90B2D4F61
EXTRA = 3  # the string is longer than every polynomial
ROWS = 4   # FR_LINCOMB_ROWS: rows per workgroup row of k_fr_lincomb (tests/test_fr_lincomb_plan_host.py reads it from the header)


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


def _lincomb(pr, vs, coef):
    """rows[j][i] = sum_l coef[l][j] vs[l][i] mod r, every v zero-extended to the longest: Python integers"""
    N, t = max(len(v) for v in vs), len(coef[0])
    rows = [[0] * N for _ in range(t)]
    for l, v in enumerate(vs):
        for j in range(t):
            c = coef[l][j]
            if c:
                row = rows[j]
                for i, a in enumerate(v):
                    row[i] = (row[i] + c * a) % pr.R
    return rows


def _check_lincomb(ps_api, pr, polys, vs, coef):
    N, t = max(len(v) for v in vs), len(coef[0])
    got = ps_api.Poly.LinComb(polys, coef)
    assert len(got) == t * N
    words = got.download()
    want = _lincomb(pr, vs, coef)
    for j in range(t):
        assert words[j * N : (j + 1) * N] == want[j], j
    return got


def test_rows_per_group_is_what_the_header_says():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "playsnark_amd", "csrc", "fr_lincomb_plan.hpp")).read()
    assert int(re.search(r"FR_LINCOMB_ROWS\s*=\s*(\d+)\s*;", src).group(1)) == ROWS


@pytest.mark.parametrize("m", [1, 2, 33])
@pytest.mark.parametrize("t", [1, 2, ROWS + 1])
def test_lincomb_is_the_sum_in_python_integers(ps_api, ctx, pr, m, t):
    """Lengths mixed from {1, 2, 5, 257, T + 1}: zero extension, a partial last workgroup, rows longer than a scan tile; m = 33
    crosses the reduce-every-32 step; t = R + 1 leaves a partial row group."""
    rng = pr.SplitMix64(0x11C0 + 64 * m + t)
    sizes = _sizes()
    lens = [sizes[(l + m + t) % 5] for l in range(m)]
    vs = [[rng.fr() for _ in range(n)] for n in lens]
    coef = [[rng.fr() for _ in range(t)] for _ in range(m)]
    _check_lincomb(ps_api, pr, [ps_api.Poly.upload(ctx, v) for v in vs], vs, coef)


def test_lincomb_at_the_top_of_the_lazy_ranges(ps_api, ctx, pr):
    """Every input word and every weight r - 1: the largest products, 33 of them in a row."""
    m, t = 33, ROWS + 1
    vs = [[pr.R - 1] * 257 for _ in range(m)]
    p = ps_api.Poly.upload(ctx, vs[0])
    _check_lincomb(ps_api, pr, [p] * m, vs, [[pr.R - 1] * t for _ in range(m)])


def test_lincomb_with_a_sparse_matrix_a_view_and_a_repeated_input(ps_api, ctx, pr):
    rng = pr.SplitMix64(0x5BA25E)
    # each polynomial used in ONE row only, as in PLONK's opening matrices
    lens = [5, 257, 2, 257, 1]
    vs = [[rng.fr() for _ in range(n)] for n in lens]
    polys = [ps_api.Poly.upload(ctx, v) for v in vs]
    coef = [[rng.fr() if j == l % 2 else 0 for j in range(2)] for l in range(5)]
    _check_lincomb(ps_api, pr, polys, vs, coef)
    # a view into a longer vector, and the same vector twice
    view = polys[1].slice(3, 250)
    _check_lincomb(ps_api, pr, [view, polys[0]], [vs[1][3:253], vs[0]], [[rng.fr(), 1], [rng.fr(), 0]])
    _check_lincomb(ps_api, pr, [polys[3], polys[3], view], [vs[3], vs[3], vs[1][3:253]], [[rng.fr()] * 3, [rng.fr()] * 3, [1, 2, 3]])


def test_add_and_sub_are_the_references_up_to_normalisation(ps_api, ctx, pr):
    rng = pr.SplitMix64(0xADD5)
    a = [rng.fr() for _ in range(257)]
    b = [rng.fr() for _ in range(5)]
    c = [rng.fr() for _ in range(250)] + a[250:]  # a - c loses its seven leading terms
    pa, pb, pc = (ps_api.Poly.upload(ctx, v) for v in (a, b, c))
    norm = pr.poly_normalize
    for x, y, px, py in ((a, b, pa, pb), (b, a, pb, pa), (a, c, pa, pc), (a, a, pa, pa)):
        assert norm(px.Add(py).download()) == norm(pr.poly_add(x, y))
        assert norm(px.Sub(py).download()) == norm(pr.poly_sub(x, y))
    assert len(pa.Sub(pc)) == 257 and len(norm(pa.Sub(pc).download())) == 250  # the longer operand's length: not normalised


def test_lincomb_argument_checks(ps_api, ctx, pr):
    p = ps_api.Poly.upload(ctx, [1, 2, 3])
    with pytest.raises(ps_api.PlaysnarkError) as e:  # a coefficient that is not below r
        ps_api.Poly.LinComb([p, p], [[1], [pr.R]])
    assert e.value.code == -3
    with pytest.raises(ps_api.LengthMismatch):  # an empty input
        ps_api.Poly.LinComb([p, p.slice(1, 0)], [[1], [1]])
    empty = ps_api.Poly.LinComb([p], [[]])  # t = 0
    assert len(empty) == 0
    ones = [1] * (1 << 20)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # m * t = 2^20 + 1
        ps_api.Poly.LinComb([p], [ones + [1]])
    assert e.value.code == -5
    long = ps_api.Poly.powers(ctx, 3, 4096)
    with pytest.raises(ps_api.PlaysnarkError) as e:  # t * N = 2^32
        ps_api.Poly.LinComb([long], [ones])
    assert e.value.code == -5


class _Opened:
    """three polynomials (5, 257, T + 1 coefficients) opened at two points under a matrix with one zero"""


@pytest.fixture(scope="module")
def opened(ps_api, ctx, co, pr, string):
    tau_g1, _ = string
    rng = pr.SplitMix64(0x0FE3)
    o = _Opened()
    o.vs = [[rng.fr() for _ in range(n)] for n in (5, 257, _tile() + 1)]
    o.polys = [ps_api.Poly.upload(ctx, v) for v in o.vs]
    o.zs = [rng.fr(), rng.fr()]
    o.coef = [[rng.fr(), 0], [rng.fr(), rng.fr()], [rng.fr(), rng.fr()]]
    o.commits = [ps_api.KZGCommit(tau_g1, p) for p in o.polys]
    o.ys, o.proofs = ps_api.KZGOpenMulti(tau_g1, o.polys, o.zs, o.coef)
    return o


def test_open_multi_gives_the_oracles_values_and_points(ps_api, ctx, co, pr, string, opened):
    tau_g1, _ = string
    o = opened
    N = max(len(v) for v in o.vs)
    assert o.ys == [[pr.poly_eval(v, z) if o.coef[i][j] else None for j, z in enumerate(o.zs)] for i, v in enumerate(o.vs)]
    rows = _lincomb(pr, o.vs, o.coef)
    f = ps_api.Poly.LinComb(o.polys, o.coef)
    for j, z in enumerate(o.zs):
        q, rem = _quotient(pr, rows[j], z)
        assert rem == sum(o.coef[i][j] * (o.ys[i][j] or 0) for i in range(3)) % pr.R
        assert o.proofs[j] == _g1(co, pr.poly_eval(q, TAU)), j
        qd, _ = f.slice(j * N, N).DivLinear([z])  # the composed route: one row, one division, one sum
        assert qd.BlindEval(tau_g1.slice(0, N - 1)) == o.proofs[j], j


@pytest.mark.parametrize("n", _sizes())
def test_one_polynomial_with_weight_one_is_kzg_open(ps_api, ctx, co, pr, string, n):
    tau_g1, _ = string
    rng = pr.SplitMix64(0xC1 + n)
    p = [rng.fr() for _ in range(n)]
    poly = ps_api.Poly.upload(ctx, p)
    zs = [rng.fr() for _ in range(3)]
    ys, proofs = ps_api.KZGOpen(tau_g1, poly, zs)
    ys_m, proofs_m = ps_api.KZGOpenMulti(tau_g1, [poly], zs, [[1, 1, 1]])
    assert ys_m == [ys] and proofs_m == proofs


def test_constants_open_to_themselves_with_identity_proofs(ps_api, ctx, co, pr, string):
    tau_g1, _ = string
    polys = [ps_api.Poly.upload(ctx, [v]) for v in (7, pr.R - 1)]
    ys, proofs = ps_api.KZGOpenMulti(tau_g1, polys, [3, 4], [[1, 0], [5, 6]])
    assert ys == [[7, None], [pr.R - 1, pr.R - 1]]
    assert proofs == [_g1(co, 0)] * 2


def test_open_multi_argument_checks(ps_api, ctx, pr, string, opened):
    tau_g1, _ = string
    o = opened
    with pytest.raises(ps_api.PlaysnarkError) as e:  # nothing is opened at the second point
        ps_api.KZGOpenMulti(tau_g1, o.polys, o.zs, [[1, 0], [1, 0], [1, 0]])
    assert e.value.code == -5 and "z[1]" in str(e.value)
    with pytest.raises(ps_api.LengthMismatch):  # the string is shorter than the longest polynomial
        ps_api.KZGOpenMulti(tau_g1.slice(0, _tile()), o.polys, o.zs, o.coef)
    with pytest.raises(ps_api.LengthMismatch):  # an empty polynomial
        ps_api.KZGOpenMulti(tau_g1, [o.polys[0], o.polys[0].slice(0, 0)], o.zs, o.coef[:2])
    for bad in ({"zs": [o.zs[0], pr.R]}, {"coef": [[1, pr.R], [1, 1], [1, 1]]}):  # a point or a weight that is not below r
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGOpenMulti(tau_g1, o.polys, bad.get("zs", o.zs), bad.get("coef", o.coef))
        assert e.value.code == -3
    assert ps_api.KZGOpenMulti(tau_g1, o.polys, [], [[], [], []]) == ([[], [], []], [])  # t = 0
    ps_api.msm_launch(ctx, tau_g1.slice(0, 5), o.polys[0])  # a sum pending on the context
    try:
        with pytest.raises(ps_api.PlaysnarkError) as e:
            ps_api.KZGOpenMulti(tau_g1, o.polys, o.zs, o.coef)
        assert e.value.code == -5
    finally:
        ps_api.msm_finish(ctx, ps_api.G1)


def _weights(pr, k, seed=0xBA7C5):
    rng = pr.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(k)]  # 128 bits each


def _verify(ps_api, ctx, t2, o, rhos, check_subgroup=True, **changed):
    get = lambda name: changed.get(name, getattr(o, name))
    return ps_api.KZGVerifyMulti(ctx, t2, get("commits"), get("zs"), get("coef"), get("ys"), get("proofs"), rhos, check_subgroup)


def test_verify_multi_accepts_what_open_multi_made(ps_api, ctx, pr, string, opened):
    _, t2 = string
    rhos = _weights(pr, 2)
    assert _verify(ps_api, ctx, t2, opened, rhos)
    assert _verify(ps_api, ctx, t2, opened, rhos, check_subgroup=False)
    assert _verify(ps_api, ctx, t2, opened, [1, 1])
    assert ps_api.KZGVerifyMulti(ctx, t2, opened.commits, [], [[], [], []], [[], [], []], [], [])  # t = 0
    # the value at the entry with weight zero is not read
    ys = [list(row) for row in opened.ys]
    assert ys[0][1] is None
    ys[0][1] = 12345
    assert _verify(ps_api, ctx, t2, opened, rhos, ys=ys)
    ys[0][1] = pr.R  # not even decoded
    assert _verify(ps_api, ctx, t2, opened, rhos, ys=ys)


def test_verify_multi_rejects_every_single_change(ps_api, ctx, co, pr, string, opened):
    tau_g1, t2 = string
    o = opened
    rhos = _weights(pr, 2)
    bump = lambda rows, i, j: [[(v + 1) % pr.R if (a, b) == (i, j) else v for b, v in enumerate(row)] for a, row in enumerate(rows)]
    rng = pr.SplitMix64(0x5EEE)
    other = ps_api.KZGCommit(tau_g1, ps_api.Poly.upload(ctx, [rng.fr() for _ in range(257)]))  # of another polynomial
    changes = {
        "one y + 1": {"ys": bump(o.ys, 1, 1)},
        "one z + 1": {"zs": [o.zs[0], (o.zs[1] + 1) % pr.R]},
        "one c + 1": {"coef": bump(o.coef, 2, 0)},
        "the proofs of the two points swapped": {"proofs": o.proofs[::-1]},
        "a commitment of another polynomial": {"commits": [o.commits[0], other, o.commits[2]]},
    }
    assert _verify(ps_api, ctx, t2, o, rhos)
    for what, ch in changes.items():
        assert not _verify(ps_api, ctx, t2, o, rhos, **ch), what
        assert not _verify(ps_api, ctx, t2, o, rhos, check_subgroup=False, **ch), what
    t2_other = co.G2.to_b(co.G2.mul((TAU + 1) % pr.R))  # tau_g2_1 of another tau
    assert not _verify(ps_api, ctx, t2_other, o, rhos)


def test_the_identity_matrix_is_verify_batch(ps_api, ctx, pr, string, opened):
    tau_g1, t2 = string
    o = opened
    zs = [o.zs[0], o.zs[1]]
    items = []
    for p, z in zip(o.polys[:2], zs):
        (y,), (pi,) = ps_api.KZGOpen(tau_g1, p, [z])
        items.append((y, pi))
    rhos = _weights(pr, 2)
    eye = [[1, 0], [0, 1]]
    for delta in (0, 1):  # an accepted and a rejected input
        y0 = (items[0][0] + delta) % pr.R
        batch = ps_api.KZGVerifyBatch(ctx, t2, o.commits[:2], zs, [y0, items[1][0]], [items[0][1], items[1][1]], rhos)
        multi = ps_api.KZGVerifyMulti(ctx, t2, o.commits[:2], zs, eye, [[y0, None], [None, items[1][0]]], [items[0][1], items[1][1]], rhos)
        assert batch == multi == (delta == 0)


def test_verify_multi_argument_checks(ps_api, ctx, pr, string, opened):
    _, t2 = string
    o = opened
    with pytest.raises(ps_api.PlaysnarkError) as e:  # a zero weight would skip a point
        _verify(ps_api, ctx, t2, o, [1, 0])
    assert e.value.code == -5
    bad = o.commits[1][:95] + bytes([o.commits[1][95] ^ 1])  # not on the curve
    with pytest.raises(ps_api.PlaysnarkError) as e:
        _verify(ps_api, ctx, t2, o, [1, 1], commits=[o.commits[0], bad, o.commits[2]])
    assert e.value.code == -3
    with pytest.raises(ps_api.PlaysnarkError) as e:  # a column of weights that opens nothing
        _verify(ps_api, ctx, t2, o, [1, 1], coef=[[1, 0], [1, 0], [1, 0]])
    assert e.value.code == -5
    with pytest.raises(ps_api.PlaysnarkError) as e:  # a value that is not below r where it is read
        _verify(ps_api, ctx, t2, o, [1, 1], ys=[[pr.R, None], o.ys[1], o.ys[2]])
    assert e.value.code == -3
