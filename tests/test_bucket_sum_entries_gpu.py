"""GPU: the whole-bucket point pass (msm.hpp section 4b, k_bucket_sum behind k_bo_count / k_bo_scan / k_bo_place) through every
entry point it is wired into, not only the lone ps_msm of tests/test_bucket_sum_gpu.py: ps_msm_multi (one sort, one perm[], one
verdict word, up to 16 point passes on rotating workspaces, both groups), ps_msm_launch / ps_msm_finish (sums in flight, each
with its own verdict word; ps_msm_last_accumulate reports the sum just finished), index-range views with and without window
tables (idx_mask / w_stride / pstride of the point loads), int64-uploaded scalars (sign bit in the entry, short-scalar plans,
the qtail reduction over the buckets the pass wrote), the tail knobs, both provers, and the batch entries, which keep the
slices whatever the knob says.

Every result is compared, byte for byte, with the CPU oracle and with the same call under set_accumulate(1); the path taken is
asserted with last_accumulate_path() wherever the entry reports one.  ctx.set_accumulate(2) forces the pass for any shape, so
the shapes are the smallest at which the plumbing can go wrong.  The automatic choice is checked at the smallest shape the
host condition admits (2^17 points, 16-bit windows, as in test_bucket_sum_gpu.py), with sums of both verdicts in flight
together; its inputs and CPU sums are made once, in a module fixture.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bucket_sum_cases import BUCKETS, SEED, SLICES, _base_points, _case, _grp, _neg, _uniform_be32  # noqa: E402

pytestmark = pytest.mark.gpu

AUTO = 0


def _reset(ctx):
    ctx.set_accumulate(0)
    ctx.set_window(0)
    ctx.set_slice(0)
    ctx.set_tail(0)
    ctx.set_batch_chunk(0)


def _ints(sc):
    return [int.from_bytes(sc[i : i + 32], "big") for i in range(0, len(sc), 32)]


def _oracle(og, sc, raw):
    """The CPU sum of scalar bytes over point bytes: the serial Mul + Add loop up to 64 points, Pippenger beyond."""
    n = len(sc) // 32
    assert len(raw) == n * og.nb
    if n <= 64:
        return og.to_b(og.blind_eval(_ints(sc), raw))
    return og.to_b(og.msm_pippenger(sc, raw, n, 4))


def _points(og, name, first, n):
    """n of the group's 4 097 base points, from `first` on."""
    assert first + n <= 4097
    return _base_points(og, name)[first * og.nb : (first + n) * og.nb]


def _special(og, pr, raw, n):
    """The array with identity points (first and later), one point three times in a row and a P / -P pair."""
    if n < 7:
        return raw
    nb = og.nb
    ident = og.to_b(None)
    P, Q = raw[nb : 2 * nb], raw[4 * nb : 5 * nb]
    negQ = og.to_b(_neg(pr, "g1", og.from_b(Q)))
    return ident + P * 3 + Q + negQ + ident + raw[7 * nb :]


def _scalars(kind, n, seed):
    """uniform: with sc[1] = sc[2] = sc[3] and sc[4] = sc[5], so that the repeated point and the P / -P pair of _special meet
    in one bucket of every window; zero; equal."""
    sc = _uniform_be32(n, seed)
    if kind == "zero":
        return bytes(32 * n)
    if kind == "equal":
        return sc[:32] * n
    assert kind == "uniform"
    if n >= 7:
        sc = sc[:64] + sc[32:64] * 2 + sc[128:160] * 2 + sc[192:]
    return sc


# ---- 1. ps_msm_multi ----------------------------------------------------------------------------------------------------------
MULTI_KINDS = ["g1", "g2", "g1", "g1"]


@pytest.mark.parametrize("kind", ["uniform", "zero", "equal"])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_multi_sum_over_both_groups_takes_whole_buckets(ps_api, ctx, co, pr, n, kind):
    """[G1, G2, G1, G1] over one scalar vector: one sort, one perm[] and one verdict word on workspace 0, four point passes on
    four workspaces with their own buckets, the G2 one in lane pairs.  Array 2 carries identity points, a point three times and
    a P / -P pair.  All-zero scalars: every bucket of every pass is empty and must still be written."""
    raws, pts = [], []
    for j, name in enumerate(MULTI_KINDS):
        gid, og = _grp(ps_api, co, name)
        raw = _points(og, name, 1000 * j if name == "g1" else 0, n)
        if j == 2:
            raw = _special(og, pr, raw, n)
        raws.append(raw)
        pts.append(ps_api.Points.upload(ctx, gid, raw))
    sc = _scalars(kind, n, SEED + 100 + n)
    dsc = ps_api.Poly.upload(ctx, sc)
    want = [_oracle(_grp(ps_api, co, name)[1], sc, raw) for name, raw in zip(MULTI_KINDS, raws)]
    plans = [(4, False), (8, False)] + ([(0, True)] if n == 300 else [])
    try:
        for window, table in plans:
            ctx.set_window(window)
            if table:
                for p in pts:
                    p.precompute()
            got = {}
            for mode in (SLICES, BUCKETS):
                ctx.set_accumulate(mode)
                got[mode] = ps_api.msm_multi(ctx, pts, dsc)
                assert ctx.last_accumulate_path() == mode, (n, kind, window, table)
                info = ctx.last_msm_info()
                assert info["window_table"] == int(table), info
                if not table:
                    assert info["window_bits"] == window and info["buckets"] == info["windows"] << (window - 1), info
            assert got[BUCKETS] == want, (n, kind, window, table)
            assert got[SLICES] == want, (n, kind, window, table)
            ctx.set_accumulate(BUCKETS)
            for p, w in zip(pts, want):  # the lone sum of each array, on the same plan
                assert dsc.BlindEval(p) == w, (n, kind, window, table)
                assert ctx.last_accumulate_path() == BUCKETS
    finally:
        _reset(ctx)


def test_multi_sum_of_sixteen_arrays_reuses_every_ring_workspace(ps_api, ctx, co, pr):
    """PS_MSM_MULTI_MAX = 16 arrays at n = 40: each of the four ring workspaces runs four point passes, one behind the other,
    over the one perm[] and verdict word of workspace 0; every fifth array is G2.  One array more is refused."""
    n = 40
    sc = _scalars("uniform", n, SEED + 140)
    dsc = ps_api.Poly.upload(ctx, sc)
    names = ["g2" if i % 5 == 1 else "g1" for i in range(16)]
    raws = [_points(_grp(ps_api, co, nm)[1], nm, 200 * i, n) for i, nm in enumerate(names)]
    raws[2] = _special(co.G1, pr, raws[2], n)
    pts = [ps_api.Points.upload(ctx, _grp(ps_api, co, nm)[0], raw) for nm, raw in zip(names, raws)]
    want = [_oracle(_grp(ps_api, co, nm)[1], sc, raw) for nm, raw in zip(names, raws)]
    assert len(set(want)) == 16
    try:
        for mode in (SLICES, BUCKETS, BUCKETS):
            ctx.set_accumulate(mode)
            assert ps_api.msm_multi(ctx, pts, dsc) == want, mode
            assert ctx.last_accumulate_path() == mode
        with pytest.raises(ps_api.PlaysnarkError):  # 16 is PS_MSM_MULTI_MAX
            ps_api.msm_multi(ctx, pts + [pts[0]], dsc)
    finally:
        _reset(ctx)


# ---- 2. sums in flight --------------------------------------------------------------------------------------------------------
_JOBS = {}


def _jobs(ps_api, ctx, co):
    """G1 n = 4 097, G2 n = 300, G1 n = 0, G1 n = 64: (group id, points, scalars, oracle bytes, n); the CPU sums are made once."""
    if not _JOBS:
        rows = []
        for name, n, first in (("g1", 4097, 0), ("g2", 300, 500), ("g1", 0, 0), ("g1", 64, 3000)):
            og = _grp(ps_api, co, name)[1]
            raw = _points(og, name, first, n)
            sc = _uniform_be32(n, SEED + 200 + n)
            rows.append((name, raw, sc, _oracle(og, sc, raw) if n else og.to_b(None)))
        _JOBS["rows"] = rows
    jobs = []
    for name, raw, sc, want in _JOBS["rows"]:
        gid = _grp(ps_api, co, name)[0]
        jobs.append((gid, ps_api.Points.upload(ctx, gid, raw), ps_api.Poly.upload(ctx, sc), want, len(sc) // 32))
    return jobs


def test_sums_in_flight_report_the_path_of_the_sum_just_finished(ps_api, ctx, co, pr):
    """PS_MSM_QUEUE launches fill the queue, set_accumulate called before each: the mode is fixed in the plan at launch, each
    sum has its own workspace, and ps_msm_last_accumulate after a finish is the path of THAT sum, not of the one launched
    last.  The empty sum launches nothing and reports nothing (the path read after it is the previous one's)."""
    from playsnark_amd import _lib

    assert _lib.PS_MSM_QUEUE == 4
    jobs = _jobs(ps_api, ctx, co)
    try:
        for modes in ((2, 1, 2, 1), (1, 2, 1, 2)):
            for (gid, pts, dsc, _, _), mode in zip(jobs, modes):
                ctx.set_accumulate(mode)
                ps_api.msm_launch(ctx, pts, dsc)
            ctx.set_accumulate(AUTO)  # whatever the knob says by now
            prev = None
            for (gid, pts, dsc, want, n), mode in zip(jobs, modes):
                assert ps_api.msm_finish(ctx, gid) == want, (modes, n)
                assert ctx.last_accumulate_path() == (mode if n else prev), (modes, n)
                prev = ctx.last_accumulate_path()
    finally:
        _reset(ctx)


def test_sums_in_flight_random_schedule_of_both_paths(ps_api, ctx, co, pr):
    """A seeded schedule of launches and finishes, the mode of each launch drawn from {slices, whole buckets}, with lone sums
    and multi-sums whenever the queue is empty: every result is the one-at-a-time bytes (the oracle's), every reported path the
    mode the sum was launched with."""
    from playsnark_amd import _lib

    jobs = _jobs(ps_api, ctx, co)
    rng = pr.SplitMix64(SEED + 9200)
    try:
        ctx.set_accumulate(SLICES)
        for gid, pts, dsc, want, n in jobs:  # one at a time
            assert dsc.BlindEval(pts) == want, n
        pending = []
        launches = finishes = lone = 0
        for step in range(40):
            r = rng.next() % 100
            if pending and (len(pending) == _lib.PS_MSM_QUEUE or r < 40):
                j, mode = pending.pop(0)
                assert ps_api.msm_finish(ctx, jobs[j][0]) == jobs[j][3], (step, j, mode)
                if jobs[j][4]:
                    assert ctx.last_accumulate_path() == mode, (step, j)
                finishes += 1
            elif not pending and r >= 70:
                j, mode = rng.next() % len(jobs), 1 + rng.next() % 2
                ctx.set_accumulate(mode)
                assert jobs[j][2].BlindEval(jobs[j][1]) == jobs[j][3], (step, j, mode)
                assert ps_api.msm_multi(ctx, [jobs[j][1], jobs[j][1]], jobs[j][2]) == [jobs[j][3]] * 2, (step, j, mode)
                if jobs[j][4]:
                    assert ctx.last_accumulate_path() == mode, (step, j)
                lone += 1
            else:
                j, mode = rng.next() % len(jobs), 1 + rng.next() % 2
                ctx.set_accumulate(mode)
                ps_api.msm_launch(ctx, jobs[j][1], jobs[j][2])
                pending.append((j, mode))
                launches += 1
        while pending:
            j, mode = pending.pop(0)
            assert ps_api.msm_finish(ctx, jobs[j][0]) == jobs[j][3], (j, mode)
            if jobs[j][4]:
                assert ctx.last_accumulate_path() == mode, j
        assert launches >= 15 and lone >= 1, (launches, finishes, lone)  # the seed's schedule does visit every kind of step
    finally:
        _reset(ctx)


# ---- 3. views and tables ------------------------------------------------------------------------------------------------------
RANGES = ((0, 1), (1, 63), (37, 300), (999, 1))


def _thirds(og, raw, n):
    """Every third point the identity (indices 2, 5, ..: the one-point ranges of RANGES keep a point)."""
    ident = og.to_b(None)
    return b"".join(ident if i % 3 == 2 else raw[i * og.nb : (i + 1) * og.nb] for i in range(n))


@pytest.mark.parametrize("config", ["none", "whole", "view"])
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_index_range_views_take_whole_buckets(ps_api, ctx, co, pr, name, config):
    """pts.slice(f, cnt) / poly.slice(f, cnt) of 1 000 points, every third the identity.  none: plain points at the view's
    offset.  whole: precompute(9) on the array; the view reads that table at its own offset (rows of 1 000 points).  view: the
    array carries the table of its own automatic window, as a prover's key does, and the sum is asked for through the view:
    views shorter than PS_VIEW_TABLE_MIN_POINTS = 1 024 points keep the array's table, so at these ranges the ViewTable route is
    NOT taken (window_bits stays the array's); test_a_view_table_is_read_by_whole_buckets below reaches it."""
    gid, og = _grp(ps_api, co, name)
    n = 1000
    raw = _thirds(og, _points(og, name, 0, n), n)
    sc = _uniform_be32(n, SEED + 300)
    pts = ps_api.Points.upload(ctx, gid, raw)
    poly = ps_api.Poly.upload(ctx, sc)
    if config != "none":
        pts.precompute(9 if config == "whole" else 0)
    try:
        for f, cnt in RANGES:
            want = _oracle(og, sc[32 * f : 32 * (f + cnt)], raw[og.nb * f : og.nb * (f + cnt)])
            got = {}
            for mode in (SLICES, BUCKETS):
                ctx.set_accumulate(mode)
                got[mode] = poly.slice(f, cnt).BlindEval(pts.slice(f, cnt))
                assert ctx.last_accumulate_path() == mode, (name, config, f, cnt)
                info = ctx.last_msm_info()
                assert info["window_table"] == int(config != "none"), (name, config, f, cnt, info)
                if config != "none":
                    assert info["window_bits"] == pts.table_window and info["buckets"] == 1 << (pts.table_window - 1), info
            assert got[SLICES] == got[BUCKETS], (name, config, f, cnt)
            assert got[BUCKETS] == want, (name, config, f, cnt)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_a_view_table_is_read_by_whole_buckets(ps_api, ctx, co, pr, name):
    """The ViewTable route (a table of the view's own length, rows of cnt points, read from its start) opens at 1 024 points:
    a 1 025-point view of a 4 097-point array whose own table has 16-bit windows gets 10-bit windows of its own on the first
    sum, as in test_index_range_views_get_a_window_table_of_their_own; both paths read it and give the oracle's bytes."""
    gid, og = _grp(ps_api, co, name)
    n, f, cnt = 4097, 37, 1025
    raw = _thirds(og, _points(og, name, 0, n), n)
    sc = _uniform_be32(cnt, SEED + 310)
    whole = ps_api.Points.upload(ctx, gid, raw).precompute(16)
    view = whole.slice(f, cnt)
    poly = ps_api.Poly.upload(ctx, sc)
    want = _oracle(og, sc, raw[og.nb * f : og.nb * (f + cnt)])
    try:
        for mode in (BUCKETS, SLICES, BUCKETS):  # built by the first sum, found by the others
            ctx.set_accumulate(mode)
            assert poly.BlindEval(view) == want, (name, mode)
            assert ctx.last_accumulate_path() == mode
            info = ctx.last_msm_info()
            assert info["window_table"] == 1 and info["window_bits"] < 16 and info["buckets"] == 1 << (info["window_bits"] - 1), info
    finally:
        _reset(ctx)
        whole.precompute(-1)


# ---- 4. int64 scalars ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 65, 300])
def test_int64_scalars_take_whole_buckets(ps_api, ctx, co, pr, n):
    """Poly.from_values: negative values are folded onto the negated point (the sign bit of the entry, which k_bucket_sum
    must honour at the first entry of a bucket, the copy, and at later ones), the plan is the short-scalar one, and its
    reduction reads the buckets the pass wrote.  Lone sums of both groups and one multi-sum over [G1, G2]."""
    rng = pr.SplitMix64(SEED + 400 + n)
    vals = [0, 1, -1, (1 << 63) - 1, -(1 << 63)] + [int(rng.next() % 2001) - 1000 for _ in range(n - 5)]
    poly = ps_api.Poly.from_values(ctx, vals)
    pts, want = [], []
    for name in ("g1", "g2"):
        gid, og = _grp(ps_api, co, name)
        raw = _points(og, name, 700, n)
        pts.append(ps_api.Points.upload(ctx, gid, raw))
        want.append(og.to_b(og.blind_eval_i64(vals, raw)))
    try:
        for mode in (SLICES, BUCKETS):
            ctx.set_accumulate(mode)
            for p, w in zip(pts, want):
                assert poly.BlindEval(p) == w, (n, mode)
                assert ctx.last_accumulate_path() == mode
                info = ctx.last_msm_info()
                assert info["windows"] * info["window_bits"] < 128, info
            assert ps_api.msm_multi(ctx, pts, poly) == want, (n, mode)
            assert ctx.last_accumulate_path() == mode
            info = ctx.last_msm_info()
            assert info["windows"] * info["window_bits"] < 128, info
    finally:
        _reset(ctx)


# ---- 5. tail knobs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 4097])
def test_tail_and_slice_knobs_do_not_change_whole_bucket_sums(ps_api, ctx, co, pr, n):
    """Chains and trees behind the pass, and every slice length: no slices are cut, so the length only sizes buffers the
    pass does not use.  The slices' bytes are taken once per tail mode, at the automatic slice length."""
    og = co.G1
    raw = _special(og, pr, _points(og, "g1", 0, n), n)
    sc = _scalars("uniform", n, SEED + 500 + n)
    pts, poly = ps_api.Points.upload(ctx, ps_api.G1, raw), ps_api.Poly.upload(ctx, sc)
    want = _oracle(og, sc, raw)
    try:
        for tail in (0, 1, 2):
            ctx.set_tail(tail)
            ctx.set_slice(0)
            ctx.set_accumulate(SLICES)
            assert poly.BlindEval(pts) == want, (n, tail)
            assert ctx.last_accumulate_path() == SLICES
            ctx.set_accumulate(BUCKETS)
            for sl in (0, 1, 5):
                ctx.set_slice(sl)
                assert poly.BlindEval(pts) == want, (n, tail, sl)
                assert ctx.last_accumulate_path() == BUCKETS
    finally:
        _reset(ctx)


# ---- 6. the provers -----------------------------------------------------------------------------------------------------------
def _abc(p):
    return (p.A, p.B, p.C)


@pytest.mark.parametrize("n", [7, 300])
def test_groth16_proofs_do_not_depend_on_the_point_pass(ps_api, ctx, co, pr, n):
    """Groth16Prove over the monomial key and over the Lagrange-form key: the sums go through msm_launch_impl(allow_self =
    false) on worker contexts and come back through ps_msm_finish, so the context does report a path after the call."""
    from oracle import restate as rs

    c, sol = rs.synthetic_circuit(n)
    rng = pr.SplitMix64(SEED + 600 + n)
    tox = [rng.fr() for _ in range(5)]
    r, s = rng.fr(), rng.fr()
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, vk = ps_api.NewGroth16TrustedSetup(q, *tox)
    io = ps_api.Poly.upload(ctx, sol[: c.nbVars - c.nbIO])
    try:
        for form, key in (("monomial", tr.monomial_only()), ("lagrange", tr.lagrange_only())):
            got = {}
            for mode in (SLICES, BUCKETS):
                ctx.set_accumulate(mode)
                got[mode] = ps_api.Groth16Prove(key, q, ps_api.Poly.upload(ctx, sol), r, s)
                assert ctx.last_accumulate_path() == mode, (n, form)
            assert _abc(got[BUCKETS]) == _abc(got[SLICES]), (n, form)
            assert ps_api.Groth16Verify(ctx, tr.Alpha, tr.Beta2, vk["Gamma"], tr.Delta2, vk["IoLP"], got[BUCKETS], io) is True, (n, form)
            if n == 7:
                o = rs.groth16_prove(rs.groth16_setup(c, *tox), c, sol, r, s)
                assert _abc(got[BUCKETS]) == (o.A, o.B, o.C), form
    finally:
        _reset(ctx)


@pytest.mark.parametrize("n", [7, 300])
def test_phgr13_proofs_do_not_depend_on_the_point_pass(ps_api, ctx, co, pr, n):
    """PHGR13Prove: the h(s) sum through msm_launch_impl and the seven solution sums (six G1, one G2) through the multi-sum
    helpers on worker contexts only (the sort on ring[0], not on the context); both set the reported path."""
    from oracle import restate as rs

    c, sol = rs.synthetic_circuit(n)
    rng = pr.SplitMix64(SEED + 650 + n)
    tox = [rng.fr() for _ in range(8)]
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *tox)
    fields = lambda p: tuple(getattr(p, f) for f in ps_api.PHGR13Proof.FIELDS)
    try:
        for form, key in (("lagrange", ek), ("monomial", ek.monomial_only())):
            got = {}
            for mode in (SLICES, BUCKETS):
                ctx.set_accumulate(mode)
                got[mode] = fields(ps_api.PHGR13Prove(key, q, ps_api.Poly.upload(ctx, sol)))
                assert ctx.last_accumulate_path() == mode, (n, form)
            assert got[BUCKETS] == got[SLICES], (n, form)
            if n == 7:
                o = rs.phgr13_prove(rs.phgr13_setup(c, *tox).EK, c, sol)
                assert got[BUCKETS] == tuple(getattr(o, f) for f in ps_api.PHGR13Proof.FIELDS), form
    finally:
        _reset(ctx)


# ---- 7. the batch entries keep the slices -------------------------------------------------------------------------------------
def _lone_takes_whole_buckets(ps_api, ctx, co):
    """A lone sum right after a batch entry, on the same context and with the knob still at whole buckets."""
    sc, raw = _uniform_be32(65, SEED + 700), _points(co.G1, "g1", 1500, 65)
    got = ps_api.Poly.upload(ctx, sc).BlindEval(ps_api.Points.upload(ctx, ps_api.G1, raw))
    assert ctx.last_accumulate_path() == BUCKETS
    assert got == _oracle(co.G1, sc, raw)


def test_msm_batch_entries_keep_the_slices(ps_api, ctx, co, pr):
    """msm_batch (n = 65, K = 5) and msm_batch_multi (one G1 and one G2 array, strided members) under mode 2: the bytes of
    mode 0, which are the oracle's member by member."""
    n, k = 65, 5
    raw1, raw2 = _points(co.G1, "g1", 100, n), _points(co.G2, "g2", 100, n)
    p1, p2 = ps_api.Points.upload(ctx, ps_api.G1, raw1), ps_api.Points.upload(ctx, ps_api.G2, raw2)
    members = [_uniform_be32(n, SEED + 710 + j) for j in range(k)]
    flat = ps_api.Poly.upload(ctx, b"".join(members))
    stride, first = n + 9, 4
    pad = _uniform_be32(stride, SEED + 720)
    strided = ps_api.Poly.upload(ctx, b"".join(pad[: 32 * first] + m + pad[32 * (first + n) :] for m in members))
    want1 = [_oracle(co.G1, m, raw1) for m in members]
    want2 = [_oracle(co.G2, m, raw2) for m in members]
    try:
        got = {}
        for mode in (AUTO, BUCKETS):
            ctx.set_accumulate(mode)
            got[mode] = (ps_api.msm_batch(ctx, p1, flat, k), ps_api.msm_batch_multi(ctx, [p1, p2], strided, k, stride, first))
        assert got[BUCKETS] == got[AUTO]
        assert got[BUCKETS] == (want1, [want1, want2])
        _lone_takes_whole_buckets(ps_api, ctx, co)
    finally:
        _reset(ctx)


def test_prover_batch_entries_keep_the_slices(ps_api, ctx, co, pr):
    """Groth16ProveBatch and PHGR13ProveBatch (n = 7, K = 3) under mode 2: the bytes of mode 0, which are the oracle's
    restatement proof by proof."""
    from oracle import restate as rs

    n, k = 7, 3
    made = [rs.synthetic_circuit(n, x0=3 + 2 * j) for j in range(k)]
    c = made[0][0]
    sols = [sol for _, sol in made]
    flat = [v for sol in sols for v in sol]
    rng = pr.SplitMix64(SEED + 750)
    tox16, tox13 = [rng.fr() for _ in range(5)], [rng.fr() for _ in range(8)]
    rr, ss = [rng.fr() for _ in range(k)], [rng.fr() for _ in range(k)]
    q = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
    tr, _ = ps_api.NewGroth16TrustedSetup(q, *tox16)
    ek, _ = ps_api.NewPHGR13TrustedSetup(q, *tox13)
    fields = lambda p: tuple(getattr(p, f) for f in ps_api.PHGR13Proof.FIELDS)
    try:
        g16, p13 = {}, {}
        for mode in (AUTO, BUCKETS):
            ctx.set_accumulate(mode)
            g16[mode] = [_abc(p) for p in ps_api.Groth16ProveBatch(tr, q, ps_api.Poly.upload(ctx, flat), rr, ss)]
            p13[mode] = [fields(p) for p in ps_api.PHGR13ProveBatch(ek, q, ps_api.Poly.upload(ctx, flat), k)]
        assert g16[BUCKETS] == g16[AUTO] and p13[BUCKETS] == p13[AUTO]
        ref16, ref13 = rs.groth16_setup(c, *tox16), rs.phgr13_setup(c, *tox13)
        for j in range(k):
            o = rs.groth16_prove(ref16, c, sols[j], rr[j], ss[j])
            assert g16[BUCKETS][j] == (o.A, o.B, o.C), j
            o = rs.phgr13_prove(ref13.EK, c, sols[j])
            assert p13[BUCKETS][j] == tuple(getattr(o, f) for f in ps_api.PHGR13Proof.FIELDS), j
        _lone_takes_whole_buckets(ps_api, ctx, co)
    finally:
        _reset(ctx)


# ---- 8, 9. the automatic choice with several sums sharing the chip ------------------------------------------------------------
class _Auto:
    pass


@pytest.fixture(scope="module")
def auto(ps_api, ctx, co):
    """2^17 points of each group, the uniform and the 0/1 scalar vector of test_bucket_sum_gpu.py, the two CPU sums over the G1
    array and the lone sums of both arrays on the slices: made once, read only."""
    a = _Auto()
    a.n = n = 1 << 17
    a.g1 = ps_api.Points.from_scalars(ctx, ps_api.G1, ps_api.Poly.upload(ctx, _uniform_be32(n, SEED + 1)))
    a.g2 = ps_api.Points.from_scalars(ctx, ps_api.G2, ps_api.Poly.upload(ctx, _uniform_be32(n, SEED + 4)))
    bits = np.zeros((n, 32), dtype=np.uint8)
    bits[:, 31] = np.random.RandomState(SEED + 3).randint(0, 2, size=n)
    a.sc = {"uniform": _uniform_be32(n, SEED + 2), "boolean": bits.tobytes()}
    a.poly = {k: ps_api.Poly.upload(ctx, v) for k, v in a.sc.items()}
    a.path = {"uniform": BUCKETS, "boolean": SLICES}  # the device's verdict for each vector
    raw = a.g1.download()
    a.want = {k: co.G1.to_b(co.G1.msm_pippenger(v, raw, n, 16)) for k, v in a.sc.items()}
    try:
        ctx.set_window(16)
        ctx.set_accumulate(SLICES)
        a.lone = {(g, k): a.poly[k].BlindEval(getattr(a, g)) for g in ("g1", "g2") for k in a.sc}
    finally:
        _reset(ctx)
    assert all(a.lone["g1", k] == a.want[k] for k in a.sc)
    return a


def test_automatic_choice_with_both_verdicts_in_flight(ps_api, ctx, auto):
    """[uniform, boolean, uniform, boolean] launched under mode 0 over one resident G1 array and finished in order: every sum
    sorts on its own workspace and carries its own verdict word, perm[] and heavy counts -- one of these shared between
    workspaces, or the verdict read from the wrong pinned buffer, shows as wrong bytes or as a path other than 2, 1, 2, 1."""
    order = ["uniform", "boolean", "uniform", "boolean"]
    try:
        ctx.set_window(16)
        ctx.set_accumulate(AUTO)
        for k in order:
            ps_api.msm_launch(ctx, auto.g1, auto.poly[k])
        for i, k in enumerate(order):
            assert ps_api.msm_finish(ctx, ps_api.G1) == auto.want[k], (i, k)
            assert ctx.last_accumulate_path() == auto.path[k], (i, k)
            info = ctx.last_msm_info()
            assert info["window_bits"] == 16 and info["buckets"] == 1 << 19, info
    finally:
        _reset(ctx)


def test_automatic_choice_in_a_multi_sum_over_both_groups(ps_api, ctx, auto):
    """msm_multi over [G1, G2, G1 again] under mode 0: one verdict for the three point passes.  Each result is the lone sum of
    its array on the slices (tied to the oracle by test_bucket_sum_gpu.py, and here for G1); the path is 2, then 1."""
    try:
        ctx.set_window(16)
        ctx.set_accumulate(AUTO)
        for k in ("uniform", "boolean"):
            got = ps_api.msm_multi(ctx, [auto.g1, auto.g2, auto.g1], auto.poly[k])
            assert ctx.last_accumulate_path() == auto.path[k], k
            info = ctx.last_msm_info()
            assert info["window_bits"] == 16 and info["buckets"] == 1 << 19, info
            assert got == [auto.lone["g1", k], auto.lone["g2", k], auto.lone["g1", k]], k
            assert got[0] == auto.want[k], k
    finally:
        _reset(ctx)
