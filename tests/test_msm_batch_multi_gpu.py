"""GPU: ps_msm_batch_multi -- K scalar vectors over A point arrays, one digit sort per pass shared by all arrays and one bucket
problem per array (csrc/msm_batch.inc) -- byte for byte against ps_msm over slices: entry (i, j) is
scalars[j*stride + first : +n].BlindEval(points[i]).  The expected bytes never come from the code under test.  The reference
statement is computeSolCommit (pinochio.go:222-241) for K solutions over the arrays of one evaluation key.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x6D626D756C7469 & 0xFFFFFFFFFFFFFFFF

SHAPES = {"g1": ["g1"], "g1g2": ["g1", "g2"], "seven": ["g1", "g2", "g1", "g1", "g1", "g1", "g1"]}

_RAW = {}


def _raw(co, pr, name, n, idx):
    """n points of the group for array `idx` of a call, made once per (group, n, idx) and shared by the tests."""
    if (name, n, idx) not in _RAW:
        og = co.G1 if name == "g1" else co.G2
        rng = pr.SplitMix64(SEED + 131 * n + 7 * idx + (name == "g2"))
        _RAW[name, n, idx] = og.gen_points(rng.fr(), rng.fr(), n)
    return _RAW[name, n, idx]


def _gid(ps_api, name):
    return ps_api.G1 if name == "g1" else ps_api.G2


def _arrays(ps_api, ctx, co, pr, names, n):
    return [ps_api.Points.upload(ctx, _gid(ps_api, nm), _raw(co, pr, nm, n, i)) for i, nm in enumerate(names)]


def _loop(arrays, sc, n, k, stride, first):
    """The parent's behaviour: one ps_msm per (array, member)."""
    views = [sc.slice(j * stride + first, n) for j in range(k)]
    return [[v.BlindEval(p) for v in views] for p in arrays]


def _layout(members, stride, first, fill):
    """The scalar vector of a call: member j at [j*stride + first, +n), `fill()` everywhere else."""
    flat = []
    for m in members:
        row = [fill() for _ in range(stride)]
        row[first : first + len(m)] = m
        flat += row
    return flat


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("shape", ["g1", "g1g2", "seven"])
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("n", [1, 5, 33, 300])
def test_batch_multi_equals_single_sums(ps_api, ctx, co, pr, n, k, shape, strided):
    names = SHAPES[shape]
    stride, first = (n + 9, 4) if strided else (n, 0)
    rng = pr.SplitMix64(SEED + 31 * n + k + 1000 * len(names) + strided)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    arrays = _arrays(ps_api, ctx, co, pr, names, n)
    sc = ps_api.Poly.upload(ctx, _layout(members, stride, first, rng.fr))
    got = ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first)
    want = _loop(arrays, sc, n, k, stride, first)
    assert [len(g) for g in got] == [k] * len(names)
    for i in range(len(names)):
        for j in range(k):
            assert got[i][j] == want[i][j], (shape, n, k, i, j)
    if strided:  # the scalars outside the members' ranges are never read: other values there, the same bytes
        other = ps_api.Poly.upload(ctx, _layout(members, stride, first, lambda: pr.R - 1 - rng.next() % 1000))
        assert ps_api.msm_batch_multi(ctx, arrays, other, k, stride, first) == got


def test_batch_multi_members_straddle_workgroups(ps_api, ctx, co, pr):
    """n = 1100, K = 9: 9 900 virtual entries -- more than one 8 192-entry workgroup of k_sort_partition_batch and five
    2 048-entry workgroups of k_sort_count_batch; a member boundary lies inside a workgroup and a workgroup boundary inside a
    member, under a stride that is not n."""
    n, k, stride, first = 1100, 9, 1109, 4
    names = ["g1", "g2", "g1"]
    rng = pr.SplitMix64(SEED + 1100)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    arrays = _arrays(ps_api, ctx, co, pr, names, n)
    sc = ps_api.Poly.upload(ctx, _layout(members, stride, first, rng.fr))
    got = ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first)
    assert got == _loop(arrays, sc, n, k, stride, first)
    other = ps_api.Poly.upload(ctx, _layout(members, stride, first, lambda: 0))
    assert ps_api.msm_batch_multi(ctx, arrays, other, k, stride, first) == got
    # member 3 against the oracle's own MSM, so that the chain of trust does not end in ps_msm alone
    assert got[0][3] == co.G1.to_b(co.G1.msm_pippenger(co.pack_fr(members[3]), _raw(co, pr, "g1", n, 0), n, 4))


def test_batch_multi_member_and_point_contents(ps_api, ctx, co, pr):
    """n = 33 over a G1 and a G2 array that hold identity points, a repeated point and a pair P, -P; members: all zero (the
    identity encoding), all r - 1, two identical members, the negation of a member (the opposite sums), and one whose scalars
    on the P / -P pair are equal (the pair cancels)."""
    from oracle import restate as rs

    n = 33
    rng = pr.SplitMix64(SEED + 33)
    arrays, raws = [], []
    for i, (nm, og) in enumerate((("g1", co.G1), ("g2", co.G2))):
        pts = og.unpack(_raw(co, pr, nm, n, i))
        pts[2] = None  # identity points
        pts[17] = None
        pts[5] = pts[4]  # a repeated point
        pts[9] = rs._neg(pts[8])  # P and -P
        raws.append(og.pack(pts))
        arrays.append(ps_api.Points.upload(ctx, _gid(ps_api, nm), raws[-1]))
    a = [rng.fr() for _ in range(n)]
    pair = [rng.fr() for _ in range(n)]
    pair[9] = pair[8]
    members = [[0] * n, [pr.R - 1] * n, a, list(a), [(pr.R - v) % pr.R for v in a], pair]
    k = len(members)
    sc = ps_api.Poly.upload(ctx, [v for m in members for v in m])
    got = ps_api.msm_batch_multi(ctx, arrays, sc, k)
    assert got == _loop(arrays, sc, n, k, n, 0)
    for i, og in enumerate((co.G1, co.G2)):
        assert got[i][0] == og.to_b(None)
        assert got[i][2] == got[i][3] and got[i][2] != got[i][4]
        assert og.add(og.from_b(got[i][2]), og.from_b(got[i][4])) is None
        for j in range(k):
            assert got[i][j] == og.to_b(og.msm_pippenger(co.pack_fr(members[j]), raws[i], n, 4)), (i, j)


def test_batch_multi_of_int64_vectors_with_negative_values(ps_api, ctx, co, pr):
    """An int64-uploaded vector (short-scalar plan, negatives folded onto the negated point), strided."""
    n, k, stride, first = 33, 3, 40, 5
    names = ["g1", "g2"]
    rng = pr.SplitMix64(SEED + 64)
    vals = [0, 1, -1, (1 << 63) - 1, -(1 << 63)] + [int(rng.next() % 2001) - 1000 for _ in range(stride * k - 5)]
    arrays = _arrays(ps_api, ctx, co, pr, names, n)
    sc = ps_api.Poly.from_values(ctx, vals)
    got = ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first)
    assert ctx.last_msm_info()["windows"] * ctx.last_msm_info()["window_bits"] < 128
    assert got == _loop(arrays, sc, n, k, stride, first)
    for i, (nm, og) in enumerate((("g1", co.G1), ("g2", co.G2))):
        for j in range(k):
            member = vals[j * stride + first : j * stride + first + n]
            assert got[i][j] == og.to_b(og.blind_eval_i64(member, _raw(co, pr, nm, n, i))), (i, j)


def test_batch_multi_passes_windows_and_reuse(ps_api, ctx, co, pr):
    """Seven arrays -- more than the four workspaces, so workspaces and their fold buffers are reused within a pass -- and
    K = 5 under set_batch_chunk(2): passes of 2, 2 and 1, every buffer reused by the next pass.  A window of 4, a forced
    window of 17 (16 * 2^16 buckets per member: exactly what the sort takes, so every pass holds one member) and one of 18
    (15 * 2^17 buckets: more than the sort takes, so the sums fall back to ps_msm per array and member) change nothing in
    the bytes; nor does a window table on an array.  Two calls in a row, then ps_msm and ps_msm_multi on the same context: nothing is
    left pending."""
    n, k, stride, first = 33, 5, 42, 4
    names = SHAPES["seven"]
    rng = pr.SplitMix64(SEED + 5)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    arrays = _arrays(ps_api, ctx, co, pr, names, n)
    sc = ps_api.Poly.upload(ctx, _layout(members, stride, first, rng.fr))
    want = _loop(arrays, sc, n, k, stride, first)
    assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
    try:
        ctx.set_batch_chunk(2)
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        one = sc.slice(first, n)
        assert one.BlindEval(arrays[1]) == want[1][0]
        assert ps_api.msm_multi(ctx, arrays, one) == [w[0] for w in want]
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        ctx.set_batch_chunk(0)
        ctx.set_window(4)
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        assert ctx.last_msm_info()["window_bits"] == 4
        ctx.set_window(17)
        assert ps_api.msm_batch_multi(ctx, arrays[:3], sc, k, stride, first) == want[:3]
        ctx.set_window(18)
        assert ps_api.msm_batch_multi(ctx, arrays[:2], sc, k, stride, first) == want[:2]
        ctx.set_window(0)
        arrays[0].precompute()
        assert arrays[0].table_window > 0
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
    finally:
        ctx.set_batch_chunk(0)
        ctx.set_window(0)
        arrays[0].drop_table()


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_one_array_packed_is_msm_batch(ps_api, ctx, co, pr, name):
    n, k = 33, 4
    rng = pr.SplitMix64(SEED + 1 + (name == "g2"))
    (pts,) = _arrays(ps_api, ctx, co, pr, [name], n)
    sc = ps_api.Poly.upload(ctx, [rng.fr() for _ in range(n * k)])
    assert ps_api.msm_batch_multi(ctx, [pts], sc, k) == [ps_api.msm_batch(ctx, pts, sc, k)]


def test_batch_multi_semantics(ps_api, ctx, co, pr):
    """Every error and empty case of the header comment, with its code; a refused call leaves the context usable."""
    C, lib = ps_api.C, ps_api.lib
    n, k = 10, 3
    rng = pr.SplitMix64(SEED + 99)
    g1, g2 = _arrays(ps_api, ctx, co, pr, ["g1", "g2"], n)
    sc = ps_api.Poly.upload(ctx, [rng.fr() for _ in range(n * k)])
    want = _loop([g1, g2], sc, n, k, n, 0)
    none = ps_api.Poly.upload(ctx, [])
    assert ps_api.msm_batch_multi(ctx, [], sc, k) == []  # a == 0
    assert ps_api.msm_batch_multi(ctx, [g1, g2], none, 0) == [[], []]  # k == 0
    e1, e2 = ps_api.Points.upload(ctx, ps_api.G1, b""), ps_api.Points.upload(ctx, ps_api.G2, b"")
    assert ps_api.msm_batch_multi(ctx, [e1, e2], none, 4) == [[co.G1.to_b(None)] * 4, [co.G2.to_b(None)] * 4]  # n == 0
    assert ps_api.msm_batch_multi(ctx, [e1], sc, k, stride=n, first=3) == [[co.G1.to_b(None)] * k]  # n == 0 inside a stride
    shorter = ps_api.Points.upload(ctx, ps_api.G1, _raw(co, pr, "g1", n, 0)[: 96 * (n - 1)])
    with pytest.raises(ps_api.LengthMismatch) as e:  # arrays of different lengths: the reference's text
        ps_api.msm_batch_multi(ctx, [g1, shorter], sc, k)
    assert "mismatch of length between poly %d and blinded eval points %d" % (n, n - 1) in str(e.value)
    with pytest.raises(ps_api.LengthMismatch):  # first + n > stride
        ps_api.msm_batch_multi(ctx, [g1], sc, k, stride=n, first=1)
    with pytest.raises(ps_api.LengthMismatch):  # len(scalars) != k * stride
        ps_api.msm_batch_multi(ctx, [g1], sc, k + 1)
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.msm_batch_multi(ctx, [g1], sc, k, stride=n + 1)
    # through the raw entry point: too many arrays, a NULL array, a NULL out[i]
    out1 = C.create_string_buffer(96 * k)
    many = (C.c_void_p * 17)(*[g1._h] * 17)
    outs = (C.c_void_p * 17)(*[C.cast(out1, C.c_void_p)] * 17)
    assert lib.ps_msm_batch_multi(ctx._h, many, 17, sc._h, k, n, 0, outs) == -5
    two = (C.c_void_p * 2)(g1._h, None)
    assert lib.ps_msm_batch_multi(ctx._h, two, 2, sc._h, k, n, 0, outs) == -5
    two = (C.c_void_p * 2)(g1._h, g1._h)
    nulls = (C.c_void_p * 2)(C.cast(out1, C.c_void_p), None)
    assert lib.ps_msm_batch_multi(ctx._h, two, 2, sc._h, k, n, 0, nulls) == -5
    assert lib.ps_msm_batch_multi(None, two, 2, sc._h, k, n, 0, outs) == -5
    # a pending sum on the context
    ps_api.msm_launch(ctx, g1, sc.slice(0, n))
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.msm_batch_multi(ctx, [g1, g2], sc, k)
    assert e.value.code == -5
    assert ps_api.msm_finish(ctx, ps_api.G1) == want[0][0]
    assert ps_api.msm_batch_multi(ctx, [g1, g2], sc, k) == want
