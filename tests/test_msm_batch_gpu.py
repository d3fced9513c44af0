"""GPU: ps_msm_batch -- K scalar vectors over ONE point array as one bucket problem of K * W bucket sets (csrc/msm_batch.hpp,
msm_batch.inc) -- byte for byte against K calls of ps_msm on slices of the same vector, and against the oracle's own MSM
where K * n <= 4096.  The reference statement is Poly.BlindEval (algebra.go:348-359), K times over one blindedPoint.
"""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x6D736D5F6261746368 & 0xFFFFFFFFFFFFFFFF


def _grp(ps_api, co, name):
    return (ps_api.G1, co.G1) if name == "g1" else (ps_api.G2, co.G2)


_POINTS = {}


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


def _check(ps_api, ctx, co, pr, name, n, members, oracle=None):
    """members: K lists of n scalars.  Batch == loop of ps_msm; with `oracle` (default: K * n <= 4096) == the oracle's MSM."""
    gid, og = _grp(ps_api, co, name)
    k = len(members)
    raw = _raw_points(co, pr, name, n)
    pts = ps_api.Points.upload(ctx, gid, raw)
    sc = ps_api.Poly.upload(ctx, [v for m in members for v in m])
    got = ps_api.msm_batch(ctx, pts, sc, k)
    assert len(got) == k
    want = _loop(pts, sc, n, k)
    for j in range(k):
        assert got[j] == want[j], (name, n, k, j)
    if oracle if oracle is not None else k * n <= 4096:
        for j in range(k):
            assert got[j] == og.to_b(og.msm_pippenger(co.pack_fr(members[j]), raw, n, 4)), (name, n, k, j, "oracle")
    return got, pts, sc


@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("n,k", [(1, 1), (1, 5), (2, 3), (63, 4), (64, 4), (65, 17), (1000, 3), (3000, 7), (8192, 2)])
def test_batch_equals_the_loop_of_single_sums(ps_api, ctx, co, pr, name, n, k):
    """(3000, 7): members straddle the 2 048-scalar count blocks and the 8 192-scalar partition chunks mid-member; (8192, 2): a
    member boundary exactly on a chunk boundary."""
    rng = pr.SplitMix64(SEED + 31 * n + k + (name == "g2"))
    _check(ps_api, ctx, co, pr, name, n, [[rng.fr() for _ in range(n)] for _ in range(k)])


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_batch_member_contents(ps_api, ctx, co, pr, name):
    """n = 65: an all-zero member (the identity encoding), a member of all r - 1, two identical members, a member that is the
    negation of another (the opposite point)."""
    gid, og = _grp(ps_api, co, name)
    n = 65
    rng = pr.SplitMix64(SEED + 65 + (name == "g2"))
    a = [rng.fr() for _ in range(n)]
    neg = [(pr.R - v) % pr.R for v in a]
    members = [[0] * n, [pr.R - 1] * n, a, list(a), neg]
    got, _, _ = _check(ps_api, ctx, co, pr, name, n, members)
    assert got[0] == og.to_b(None)
    assert got[2] == got[3]
    P, Q = og.from_b(got[2]), og.from_b(got[4])
    assert og.add(P, Q) is None and got[2] != got[4]


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_batch_of_int64_vectors_with_negative_values(ps_api, ctx, co, pr, name):
    """An int64-uploaded vector (short-scalar plan, negatives folded onto the negated point: max_bits and neg_small of the
    vector are respected as in msm_sort)."""
    gid, og = _grp(ps_api, co, name)
    n, k = 65, 3
    rng = pr.SplitMix64(SEED + 64 + (name == "g2"))
    vals = [0, 1, -1, (1 << 63) - 1, -(1 << 63)] + [int(rng.next() % 2001) - 1000 for _ in range(n * k - 5)]
    raw = _raw_points(co, pr, name, n)
    pts = ps_api.Points.upload(ctx, gid, raw)
    sc = ps_api.Poly.from_values(ctx, vals)
    got = ps_api.msm_batch(ctx, pts, sc, k)
    assert ctx.last_msm_info()["windows"] * ctx.last_msm_info()["window_bits"] < 128
    assert got == _loop(pts, sc, n, k)
    for j in range(k):
        assert got[j] == og.to_b(og.blind_eval_i64(vals[j * n : (j + 1) * n], raw)), j


def test_batch_hot_bucket_takes_the_tiled_sort(ps_api, ctx, co, pr):
    """n = 70 000, K = 2, member 0 all ones and member 1 uniform (G1): the ones put 70 000 entries into one bucket of member 0's
    lowest window -- a coarse bin over SORT_BIG entries, walked by the k_sort_big_* kernels under a batch key."""
    n = 70000
    rng = pr.SplitMix64(SEED + 70000)
    _check(ps_api, ctx, co, pr, "g1", n, [[1] * n, [rng.fr() for _ in range(n)]])


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_batch_passes_windows_tables_and_reuse(ps_api, ctx, co, pr, name):
    """The split into passes (set_chunk(2), K = 5: passes of 2, 2 and 1), the window size (4 and 13) and a window table on the
    points change nothing in the bytes; nor does calling twice (the context's buffers are reused)."""
    gid, og = _grp(ps_api, co, name)
    n, k = 65, 5
    rng = pr.SplitMix64(SEED + 5 + (name == "g2"))
    got, pts, sc = _check(ps_api, ctx, co, pr, name, n, [[rng.fr() for _ in range(n)] for _ in range(k)])
    assert ps_api.msm_batch(ctx, pts, sc, k) == got
    try:
        ctx.set_batch_chunk(2)
        assert ps_api.msm_batch(ctx, pts, sc, k) == got
        ctx.set_batch_chunk(0)
        for c in (4, 13):
            ctx.set_window(c)
            assert ps_api.msm_batch(ctx, pts, sc, k) == got, c
            assert ctx.last_msm_info()["window_bits"] == c
        ctx.set_window(0)
        pts.precompute()
        assert pts.table_window > 0
        assert ps_api.msm_batch(ctx, pts, sc, k) == got
        assert ctx.last_msm_info()["window_table"] == 0
    finally:
        ctx.set_batch_chunk(0)
        ctx.set_window(0)
        pts.drop_table()


def test_batch_semantics(ps_api, ctx, co, pr):
    """K = 0 and n = 0; a wrong length is BlindEval's panic; a pending ps_msm_launch is an error that leaves the context
    usable."""
    rng = pr.SplitMix64(SEED + 99)
    n, k = 10, 3
    raw = _raw_points(co, pr, "g1", n)
    pts = ps_api.Points.upload(ctx, ps_api.G1, raw)
    vals = [rng.fr() for _ in range(n * k)]
    sc = ps_api.Poly.upload(ctx, vals)
    assert ps_api.msm_batch(ctx, pts, ps_api.Poly.upload(ctx, []), 0) == []
    empty = ps_api.Points.upload(ctx, ps_api.G1, b"")
    assert ps_api.msm_batch(ctx, empty, ps_api.Poly.upload(ctx, []), 4) == [co.G1.to_b(None)] * 4
    with pytest.raises(ps_api.LengthMismatch):
        ps_api.msm_batch(ctx, pts, sc, k + 1)
    want = _loop(pts, sc, n, k)
    one = sc.slice(0, n)
    ps_api.msm_launch(ctx, pts, one)
    with pytest.raises(ps_api.PlaysnarkError) as e:
        ps_api.msm_batch(ctx, pts, sc, k)
    assert e.value.code == -5
    assert ps_api.msm_finish(ctx, ps_api.G1) == want[0]
    assert ps_api.msm_batch(ctx, pts, sc, k) == want
