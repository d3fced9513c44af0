"""GPU: ps_msm_batch and ps_msm_batch_multi over the window tables of their points (csrc/msm_batch.hpp: k_sort_count_batch_tab,
k_sort_partition_batch_tab; msm_batch.inc) -- one bucket set per member, no fold -- byte for byte against the loop of ps_msm
over slices, computed BEFORE the points get their table (so the expected bytes come from the plain single sum), and against
the oracle's own MSM where K * n <= 4096.  ps_msm_batch_set_table: 0 automatic, 1 never, 2 wherever a table is usable.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x6D736D5F62746162 & 0xFFFFFFFFFFFFFFFF
MAX_BITS = 255

_POINTS = {}
_WANT = {}


def _grp(ps_api, co, name):
    return (ps_api.G1, co.G1) if name == "g1" else (ps_api.G2, co.G2)


def _raw_points(co, pr, name, n):
    """n points of the group, made once per (group, n) and shared by the tests."""
    if (name, n) not in _POINTS:
        og = co.G1 if name == "g1" else co.G2
        rng = pr.SplitMix64(SEED + n)
        _POINTS[name, n] = og.gen_points(rng.fr(), rng.fr(), n)
    return _POINTS[name, n]


def _loop(pts, sc, n, k):
    """The parent's behaviour: one ps_msm per member."""
    return [sc.slice(j * n, n).BlindEval(pts) for j in range(k)]


def _restore(ctx, *points):
    ctx.set_batch_table(0)
    ctx.set_batch_chunk(0)
    ctx.set_window(0)
    for p in points:
        p.drop_table()


def _tabled(ps_api, ctx, pts, sc, k, c, members_last=None):
    """msm_batch over a table the caller has built, with the route it took checked on last_msm_info."""
    got = ps_api.msm_batch(ctx, pts, sc, k)
    info = ctx.last_msm_info()
    assert info["window_table"] == 1 and info["window_bits"] == c, info
    assert info["windows"] == sc_bits(sc) // c + 1, info
    assert info["buckets"] == (k if members_last is None else members_last) << (c - 1), info
    return got


def sc_bits(sc):
    return getattr(sc, "_max_bits", MAX_BITS)


def _reference(ps_api, ctx, co, pr, name, n, members, key):
    """(points without a table, scalars, the loop's bytes): the loop runs once per `key`, against the oracle where K * n <= 4096."""
    gid, og = _grp(ps_api, co, name)
    raw = _raw_points(co, pr, name, n)
    pts = ps_api.Points.upload(ctx, gid, raw)
    sc = ps_api.Poly.upload(ctx, [v for m in members for v in m])
    k = len(members)
    if key not in _WANT:
        want = _loop(pts, sc, n, k)
        assert ctx.last_msm_info()["window_table"] == 0
        if k * n <= 4096:
            for j in range(k):
                assert want[j] == og.to_b(og.msm_pippenger(co.pack_fr(members[j]), raw, n, 4)), (name, n, k, j, "oracle")
        _WANT[key] = want
    return pts, sc, _WANT[key]


@pytest.mark.parametrize("c", [8, 13])
@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("n,k", [(1, 1), (1, 5), (2, 3), (63, 4), (64, 4), (65, 17), (3000, 7), (8192, 2)])
def test_tabled_batch_equals_the_loop_of_single_sums(ps_api, ctx, co, pr, name, n, k, c):
    """c = 8: W = 32 windows, the window tag of an entry reaches 31, the top of its five bits.  (3000, 7): members straddle the
    2 048-scalar count blocks and the 8 192-scalar partition chunks mid-member; (8192, 2): a member boundary on a chunk
    boundary."""
    rng = pr.SplitMix64(SEED + 31 * n + k + (name == "g2"))
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    pts, sc, want = _reference(ps_api, ctx, co, pr, name, n, members, ("uniform", name, n, k))
    try:
        pts.precompute(c)
        ctx.set_batch_table(2)
        got = _tabled(ps_api, ctx, pts, sc, k, c)
        for j in range(k):
            assert got[j] == want[j], (name, n, k, c, j)
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_tabled_batch_member_contents(ps_api, ctx, co, pr, name):
    """n = 65 over an 8-bit table: an all-zero member (the identity encoding), a member of all r - 1, two identical members, a
    member that is the negation of another (the opposite point)."""
    gid, og = _grp(ps_api, co, name)
    n = 65
    rng = pr.SplitMix64(SEED + 65 + (name == "g2"))
    a = [rng.fr() for _ in range(n)]
    members = [[0] * n, [pr.R - 1] * n, a, list(a), [(pr.R - v) % pr.R for v in a]]
    pts, sc, want = _reference(ps_api, ctx, co, pr, name, n, members, ("contents", name))
    try:
        pts.precompute(8)
        ctx.set_batch_table(2)
        got = _tabled(ps_api, ctx, pts, sc, len(members), 8)
        assert got == want
        assert got[0] == og.to_b(None)
        assert got[2] == got[3] and got[2] != got[4]
        assert og.add(og.from_b(got[2]), og.from_b(got[4])) is None
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_tabled_batch_over_one_repeated_point(ps_api, ctx, co, pr, name):
    """65 copies of ONE point: every row of the table holds one point 65 times, so a bucket that takes two entries of a window
    adds P + P (and P - P where the digits' signs differ).  Expected: (sum of the member's scalars) * P from the oracle."""
    gid, og = _grp(ps_api, co, name)
    n, k = 65, 4
    rng = pr.SplitMix64(SEED + 66 + (name == "g2"))
    one = og.unpack(_raw_points(co, pr, name, 1))[0]
    raw = og.pack([one] * n)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    pts = ps_api.Points.upload(ctx, gid, raw)
    sc = ps_api.Poly.upload(ctx, [v for m in members for v in m])
    want = _loop(pts, sc, n, k)
    for j in range(k):
        assert want[j] == og.to_b(og.mul(sum(members[j]) % pr.R, one)), j
    try:
        pts.precompute(8)
        ctx.set_batch_table(2)
        assert _tabled(ps_api, ctx, pts, sc, k, 8) == want
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_tabled_batch_of_int64_vectors_with_negative_values(ps_api, ctx, co, pr, name):
    """An int64-uploaded vector over a 10-bit table: short max_bits (fewer windows than the table has rows), negatives folded
    onto the negated point."""
    gid, og = _grp(ps_api, co, name)
    n, k = 65, 3
    rng = pr.SplitMix64(SEED + 64 + (name == "g2"))
    vals = [0, 1, -1, (1 << 63) - 1, -(1 << 63)] + [int(rng.next() % 2001) - 1000 for _ in range(n * k - 5)]
    raw = _raw_points(co, pr, name, n)
    pts = ps_api.Points.upload(ctx, gid, raw)
    sc = ps_api.Poly.from_values(ctx, vals)
    want = _loop(pts, sc, n, k)
    for j in range(k):
        assert want[j] == og.to_b(og.blind_eval_i64(vals[j * n : (j + 1) * n], raw)), j
    try:
        pts.precompute(10)
        ctx.set_batch_table(2)
        assert ps_api.msm_batch(ctx, pts, sc, k) == want
        info = ctx.last_msm_info()
        assert info["window_table"] == 1 and info["window_bits"] == 10 and info["buckets"] == k << 9, info
        assert info["windows"] * 10 < 128 and info["windows"] < 255 // 10 + 1, info
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_tabled_batch_passes_and_reuse(ps_api, ctx, co, pr, name):
    """set_batch_chunk(2) with K = 5: passes of 2, 2 and 1 (the last pass holds one member's buckets); calling twice gives the
    same bytes (the context's buffers are reused)."""
    n, k = 65, 5
    rng = pr.SplitMix64(SEED + 5 + (name == "g2"))
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    pts, sc, want = _reference(ps_api, ctx, co, pr, name, n, members, ("passes", name))
    try:
        pts.precompute(13)
        ctx.set_batch_table(2)
        assert _tabled(ps_api, ctx, pts, sc, k, 13) == want
        assert _tabled(ps_api, ctx, pts, sc, k, 13) == want
        ctx.set_batch_chunk(2)
        assert _tabled(ps_api, ctx, pts, sc, k, 13, members_last=1) == want
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("c,k,last", [(16, 33, 1), (16, 32, 32), (20, 3, 1)])
def test_tabled_batch_hits_the_bucket_limit(ps_api, ctx, co, pr, c, k, last):
    """n = 64 (G1).  A 16-bit table: 32 members of 2^15 buckets fill the sort's 2^20 bucket keys, so K = 32 is one pass and
    K = 33 leaves a last pass of one member.  A 20-bit table: two members of 2^19 buckets per pass, K = 3 runs 2 and 1."""
    n = 64
    rng = pr.SplitMix64(SEED + 64 + c + k)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    pts, sc, want = _reference(ps_api, ctx, co, pr, "g1", n, members, ("limit", c, k))
    try:
        pts.precompute(c)
        ctx.set_batch_table(2)
        assert _tabled(ps_api, ctx, pts, sc, k, c, members_last=last) == want
    finally:
        _restore(ctx, pts)


def test_tabled_batch_hot_bucket_takes_the_tiled_sort(ps_api, ctx, co, pr):
    """n = 70 000, K = 2, member 0 all ones and member 1 uniform (G1, 13-bit table): the ones put 70 000 entries into ONE bucket
    of member 0 -- a coarse bin over SORT_BIG entries, walked by the k_sort_big_* kernels under a tabled batch key."""
    n = 70000
    rng = pr.SplitMix64(SEED + 70000)
    members = [[1] * n, [rng.fr() for _ in range(n)]]
    pts, sc, want = _reference(ps_api, ctx, co, pr, "g1", n, members, ("hot",))
    try:
        pts.precompute(13)
        ctx.set_batch_table(2)
        assert _tabled(ps_api, ctx, pts, sc, 2, 13) == want
    finally:
        _restore(ctx, pts)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_tabled_batch_over_a_view(ps_api, ctx, co, pr, name):
    """pts.slice(5, 65) of a tabled array of 80 points: the table's base is offset by the view's first point and its rows keep
    the stride of the whole array."""
    gid, og = _grp(ps_api, co, name)
    n, k = 65, 4
    rng = pr.SplitMix64(SEED + 80 + (name == "g2"))
    raw = _raw_points(co, pr, name, 80)
    wb = len(raw) // 80
    whole = ps_api.Points.upload(ctx, gid, raw)
    view = whole.slice(5, n)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    sc = ps_api.Poly.upload(ctx, [v for m in members for v in m])
    want = _loop(view, sc, n, k)
    for j in range(k):
        assert want[j] == og.to_b(og.msm_pippenger(co.pack_fr(members[j]), raw[5 * wb : (5 + n) * wb], n, 4)), j
    try:
        whole.precompute(13)
        ctx.set_batch_table(2)
        assert _tabled(ps_api, ctx, view, sc, k, 13) == want
    finally:
        _restore(ctx, whole)


def test_automatic_mode_follows_the_floor_the_model_and_the_forced_window(ps_api, ctx, co, pr):
    """n = 1026 (at least PS_BATCH_TABLE_MIN_POINTS), K = 4, uniform 255-bit scalars over the automatic table: the tabled pass;
    set_batch_table(1): the plain pass, the same bytes; an int64 vector over a 20-bit table stays plain by the cost model (2^19
    buckets to reduce for a handful of windows); set_window(13) means the plain plan with 13-bit windows."""
    n, k = 1026, 4
    rng = pr.SplitMix64(SEED + 1026)
    members = [[rng.fr() for _ in range(n)] for _ in range(k)]
    pts, sc, want = _reference(ps_api, ctx, co, pr, "g1", n, members, ("auto",))
    try:
        pts.precompute()
        c = pts.table_window
        assert c > 0
        assert _tabled(ps_api, ctx, pts, sc, k, c) == want
        ctx.set_batch_table(1)
        assert ps_api.msm_batch(ctx, pts, sc, k) == want
        assert ctx.last_msm_info()["window_table"] == 0
        ctx.set_batch_table(0)
        ctx.set_window(13)
        assert ps_api.msm_batch(ctx, pts, sc, k) == want
        info = ctx.last_msm_info()
        assert info["window_table"] == 0 and info["window_bits"] == 13, info
        ctx.set_window(0)
        vals = [int(rng.next() % 2001) - 1000 for _ in range(n * k)]
        small = ps_api.Poly.from_values(ctx, vals)
        pts.drop_table()
        want_small = _loop(pts, small, n, k)
        pts.precompute(20)
        assert ps_api.msm_batch(ctx, pts, small, k) == want_small
        assert ctx.last_msm_info()["window_table"] == 0
    finally:
        _restore(ctx, pts)


def test_tabled_batch_multi_needs_one_window_on_every_array(ps_api, ctx, co, pr):
    """msm_batch_multi over a G1 and a G2 array, stride > n and first > 0, mode 2: both with 13-bit tables -> the tabled pass;
    only one of the two tabled, or tables of different windows -> the plain pass.  The bytes equal the loops either way."""
    n, k, stride, first = 65, 5, 74, 4
    rng = pr.SplitMix64(SEED + 7400)
    arrays = [ps_api.Points.upload(ctx, ps_api.G1, _raw_points(co, pr, "g1", n)), ps_api.Points.upload(ctx, ps_api.G2, _raw_points(co, pr, "g2", n))]
    flat = [rng.fr() for _ in range(k * stride)]
    sc = ps_api.Poly.upload(ctx, flat)
    views = [sc.slice(j * stride + first, n) for j in range(k)]
    want = [[v.BlindEval(p) for v in views] for p in arrays]
    for og, raw, row in ((co.G1, _raw_points(co, pr, "g1", n), want[0]), (co.G2, _raw_points(co, pr, "g2", n), want[1])):
        for j in range(k):
            assert row[j] == og.to_b(og.msm_pippenger(co.pack_fr(flat[j * stride + first : j * stride + first + n]), raw, n, 4)), j
    try:
        ctx.set_batch_table(2)
        arrays[0].precompute(13)
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        assert ctx.last_msm_info()["window_table"] == 0
        arrays[1].precompute(10)
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        assert ctx.last_msm_info()["window_table"] == 0
        arrays[1].precompute(13)
        assert ps_api.msm_batch_multi(ctx, arrays, sc, k, stride, first) == want
        info = ctx.last_msm_info()
        assert info["window_table"] == 1 and info["window_bits"] == 13 and info["windows"] == 20 and info["buckets"] == k << 12, info
    finally:
        _restore(ctx, *arrays)
