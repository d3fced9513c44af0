"""The point codecs and the subgroup test at edge encodings, against the strict model of tests/wire_model.py.

Host (no device): ps_point_convert and ps_points_sum over every entry of the edge table.
Device (marked gpu): k_points_from_bytes_g1/_g2, k_points_decompress<Fp|Fp2>, k_points_to_bytes, k_points_compress and
k_points_subgroup through Points.upload / download / download_compressed / in_subgroup -- the accepted entries byte for byte,
every rejected entry alone in block 0 and in block 1 of an otherwise valid array, the count of bad points across blocks,
and an upload that works after each one that failed.  The rejected entries are enumerated, never sampled: a test walks its
whole list and reports every entry that went wrong."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wire_model as wm  # noqa: E402

CASES = [(g, f) for g in (wm.G1, wm.G2) for f in (wm.AFFINE, wm.COMPRESSED)]
IDS = ["%s-%s" % c for c in CASES]
N_REJ = 513  # two full blocks of 256 threads and one thread of a third


def _ids(ps_api, group, fmt):
    return (ps_api.G1 if group == wm.G1 else ps_api.G2), (ps_api.FMT_AFFINE if fmt == wm.AFFINE else ps_api.FMT_COMPRESSED)


def _message(err):
    return str(err).split(": ", 1)[1]


# ---------------------------------------------------------------------------------------
# the model and the table
# ---------------------------------------------------------------------------------------
def test_model_special_points(pr):
    """What the table relies on, so that it cannot silently lose it."""
    P = wm.P
    real, imag = wm.g2_special()
    for pt in (real, imag):
        assert wm.on_curve(wm.G2, pt) and not wm.in_subgroup(wm.G2, pt)
        assert pt[0][1] == 2 and wm.rhs(wm.G2, pt[0])[1] == 0  # x = (x0, 2), a real right-hand side
    assert real[0][0] == P - imag[0][0]
    # a square in Fp: y.c1 = 0, the sign bit is decided by c0
    assert wm.fp_is_square(wm.rhs(wm.G2, real[0])[0]) and real[1][1] == 0 and real[1][0] != 0
    assert wm.lex_larger(wm.G2, real[1]) == (real[1][0] > wm.HALF) != wm.lex_larger(wm.G2, wm.neg(wm.G2, real)[1])
    # a non-square in Fp: y.c0 = 0, and the complex method meets alpha = a^((p-1)/2) = -1
    a = wm.rhs(wm.G2, imag[0])
    assert not wm.fp_is_square(a[0]) and imag[1][0] == 0 and imag[1][1] != 0
    a1 = pr.f2_pow(a, (P - 3) // 4)
    assert pr.f2_mul(a1, pr.f2_mul(a1, a)) == (P - 1, 0)
    a = wm.rhs(wm.G2, real[0])
    a1 = pr.f2_pow(a, (P - 3) // 4)
    assert pr.f2_mul(a1, pr.f2_mul(a1, a)) == (1, 0)
    # (0, 2) has order 3
    for pt in wm.g1_order3():
        assert wm.on_curve(wm.G1, pt) and not wm.in_subgroup(wm.G1, pt)
        assert pr.G1.add(pr.G1.add(pt, pt), pt) is None and pr.G1.add(pt, pt) == wm.neg(wm.G1, pt)
    # the twist has no point with x = 0
    assert wm.fp2_sqrt(wm.rhs(wm.G2, (0, 0))) is None and pr.f2_sqrt((4, 4)) is None
    # no point of E(Fp) has y = (p-1)/2 or (p+1)/2: y^2 - 4 is not a cube (p = 1 mod 3)
    assert P % 3 == 1
    for y in (wm.HALF, wm.HALF + 1):
        assert pow((y * y - 4) % P, (P - 1) // 3, P) != 1
    # the model's square root agrees with the oracle's complex method on squares and non-squares
    rng = pr.SplitMix64(99)
    for _ in range(20):
        a = (rng.fr() * rng.fr() % P, rng.fr() * rng.fr() % P)
        s, t = wm.fp2_sqrt(a), pr.f2_sqrt(a)
        assert (s is None) == (t is None) and (s is None or pr.f2_sqr(s) == a)


def test_table_has_the_listed_kinds():
    for group, fmt in CASES:
        acc, rej = wm.split_table(group, fmt)
        assert len(acc) >= 5 and len(rej) >= 30, (group, fmt)
        for raw, _label, pt in acc:  # an accepted point encodes back; the compressed form is canonical
            assert wm.decode(group, wm.AFFINE, wm.encode_uncompressed(group, pt)) == pt
            assert wm.decode(group, wm.COMPRESSED, wm.encode_compressed(group, pt)) == pt
            assert wm.encode(group, fmt, pt) == raw
    verdict = {(g, f, label): wm.decode(g, f, raw) for g, f, raw, label in wm.edge_table()}
    gx = wm.GROUPS[wm.G1].gen[0]
    hx = wm.GROUPS[wm.G2].gen[0]
    R = wm.REJECT
    assert verdict[wm.G1, wm.COMPRESSED, "x=0x0 flag=0x80"] == (0, 2) and verdict[wm.G1, wm.COMPRESSED, "x=0x0 flag=0xa0"] == (0, wm.P - 2)
    assert verdict[wm.G1, wm.COMPRESSED, "x=%#x flag=0x80" % wm.P] is R          # x = p: the alias of x = 0
    assert verdict[wm.G1, wm.COMPRESSED, "x=0x1 flag=0x80"] is R                  # 5 is a non-residue
    assert verdict[wm.G1, wm.COMPRESSED, "x=%#x flag=0x00" % gx] is R             # 0x80 missing
    assert verdict[wm.G1, wm.COMPRESSED, "x=0x0 flag=0xe0"] is R                  # the identity with the sign bit
    assert verdict[wm.G2, wm.COMPRESSED, "x=(0x0, 0x0) flag=0x80"] is R           # 4 + 4u is a non-residue
    assert verdict[wm.G2, wm.COMPRESSED, "x=(%#x, %#x) flag=0x80" % (hx[0] + wm.P, hx[1])] is R
    assert verdict[wm.G2, wm.COMPRESSED, "x=(%#x, %#x) flag=0x80" % hx] in (wm.GROUPS[wm.G2].gen, wm.neg(wm.G2, wm.GROUPS[wm.G2].gen))
    assert verdict[wm.G1, wm.AFFINE, "(x, y+p) flag=0x00"] is R and verdict[wm.G1, wm.AFFINE, "(p, 2) flag=0x00"] is R
    assert verdict[wm.G1, wm.AFFINE, "(0, p+2) flag=0x00"] is R and verdict[wm.G1, wm.AFFINE, "(0, 0) flag=0x00"] is R
    assert verdict[wm.G1, wm.AFFINE, "(0, 0) flag=0x40"] is None and verdict[wm.G1, wm.AFFINE, "G flag=0x40"] is R
    for c in ("x.c0", "y.c1", "y.c0"):
        assert verdict[wm.G2, wm.AFFINE, "G with %s + p flag=0x00" % c] is R
    assert verdict[wm.G2, wm.AFFINE, "special, real root with y.c1 + p flag=0x00"] is R  # y.c1 = p, the alias of 0
    assert verdict[wm.G2, wm.AFFINE, "special, imaginary root with y.c0 + p flag=0x00"] is R


# ---------------------------------------------------------------------------------------
# host codec
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,fmt", CASES, ids=IDS)
def test_host_point_convert_matches_the_model(ps_api, group, fmt):
    gid, fid = _ids(ps_api, group, fmt)
    wrong = []
    for g, f, raw, label in wm.edge_table():
        if (g, f) != (group, fmt):
            continue
        want = wm.decode(g, f, raw)
        for out_fmt, out_id in ((wm.AFFINE, ps_api.FMT_AFFINE), (wm.COMPRESSED, ps_api.FMT_COMPRESSED)):
            try:
                got = ps_api.point_convert(gid, raw, fid, out_id)
            except ps_api.PlaysnarkError as e:
                got = e.code
            exp = -3 if want is wm.REJECT else wm.encode(g, out_fmt, want)
            if got != exp:
                wrong.append((label, out_fmt))
    assert not wrong, wrong


@pytest.mark.parametrize("group", [wm.G1, wm.G2])
def test_host_points_sum_over_the_uncompressed_entries(ps_api, pr, group):
    """ps_points_sum reads the same affine bytes: a rejected entry placed second of three fails the sum, an accepted one is
    added by the group law (the generator is one of the entries: G + G + 5G takes the doubling branch)."""
    gid, _ = _ids(ps_api, group, wm.AFFINE)
    grp = wm.GROUPS[group]
    first, third = grp.gen, grp.mul(5)
    acc, rej = wm.split_table(group, wm.AFFINE)
    wrong = []
    for raw, label in rej:
        try:
            ps_api.points_sum(gid, wm.encode_uncompressed(group, first) + raw + wm.encode_uncompressed(group, third))
            wrong.append(label)
        except ps_api.PlaysnarkError as e:
            if e.code != -3:
                wrong.append(label)
    for raw, label, pt in acc:
        got = ps_api.points_sum(gid, wm.encode_uncompressed(group, first) + raw + wm.encode_uncompressed(group, third))
        if got != wm.encode_uncompressed(group, grp.add(grp.add(first, pt), third)):
            wrong.append(label)
    assert not wrong, wrong


def test_model_rejects_the_subgroup_intruders(off_subgroup):
    for group, pts in ((wm.G1, _intruders(wm.G1, off_subgroup)), (wm.G2, _intruders(wm.G2, off_subgroup))):
        for name, pt in pts:
            assert wm.on_curve(group, pt) and not wm.in_subgroup(group, pt), (group, name)
    assert wm.in_subgroup(wm.G1, wm.GROUPS[wm.G1].gen) and wm.in_subgroup(wm.G2, wm.GROUPS[wm.G2].gen)


def _intruders(group, off_subgroup):
    if group == wm.G1:
        grp = wm.GROUPS[wm.G1]
        a, b = wm.g1_order3()
        return [("(0, 2)", a), ("(0, p-2)", b), ("G + (0, 2)", grp.add(grp.gen, a)), ("large order", off_subgroup[0]),
                ("large order, negated", grp.neg(off_subgroup[0]))]
    real, imag = wm.g2_special()
    return [("large order", off_subgroup[1]), ("special, real root", real), ("special, imaginary root", imag)]


# ---------------------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def valid(co):
    """{group: 600 oracle-made subgroup points}, made once"""
    return {wm.G1: co.G1.unpack(co.G1.gen_points(1234567, 89, 600)), wm.G2: co.G2.unpack(co.G2.gen_points(7654321, 97, 600))}


def _wire(group, fmt, pts):
    return [wm.encode(group, fmt, p) for p in pts]


@pytest.mark.gpu
@pytest.mark.parametrize("group,fmt", CASES, ids=IDS)
def test_device_accepted_entries_byte_for_byte(ps_api, ctx, valid, group, fmt):
    """Every accepted entry of one group and format in one upload of 600 points, astride the boundary of blocks 0 and 1 and
    again at both ends of the array; both downloads, whole and by ranges, are the model's encodings."""
    gid, fid = _ids(ps_api, group, fmt)
    acc, _ = wm.split_table(group, fmt)
    n = 600
    pts = list(valid[group][:n])
    rows = _wire(group, fmt, pts)
    where = [250 + i for i in range(len(acc))] + [0, n - 1]
    for i, (raw, _label, pt) in zip(where, acc + [acc[0], acc[-1]]):
        rows[i], pts[i] = raw, pt
    assert where[len(acc) - 1] >= 256
    arr = ps_api.Points.upload(ctx, gid, b"".join(rows), fid)
    assert len(arr) == n
    aff, com = _wire(group, wm.AFFINE, pts), _wire(group, wm.COMPRESSED, pts)
    got_a, got_c = arr.download(), arr.download_compressed()
    wa, wc = wm.WIRE[group], wm.WIRE[group] // 2
    bad = [(i, "affine") for i in range(n) if got_a[i * wa:(i + 1) * wa] != aff[i]]
    bad += [(i, "compressed") for i in range(n) if got_c[i * wc:(i + 1) * wc] != com[i]]
    assert not bad, [(i, f, acc[where.index(i)][1] if i in where else "padding") for i, f in bad]
    for first, cnt in ((255, 2), (256, 300), (599, 1), (600, 0)):
        assert arr.download(first, cnt) == b"".join(aff[first:first + cnt]), (first, cnt)
        assert arr.download_compressed(first, cnt) == b"".join(com[first:first + cnt]), (first, cnt)


def _try_upload(ps_api, ctx, gid, fid, raw):
    """the library's message for a failed upload with code -3, or what else happened"""
    try:
        ps_api.Points.upload(ctx, gid, raw, fid)
    except ps_api.PlaysnarkError as e:
        return _message(e) if e.code == -3 else "code %d" % e.code
    return "accepted"


@pytest.mark.gpu
@pytest.mark.parametrize("group,fmt", CASES, ids=IDS)
def test_device_rejects_every_rejected_entry_alone(ps_api, ctx, valid, group, fmt):
    """Each rejected entry alone at index 0 and at index 256 of 513 otherwise valid points: code -3 and "1 point(s)"; the
    same context then uploads the valid array and returns its bytes."""
    gid, fid = _ids(ps_api, group, fmt)
    _, rej = wm.split_table(group, fmt)
    good = _wire(group, fmt, valid[group][:N_REJ])
    want = b"".join(_wire(group, wm.AFFINE, valid[group][:N_REJ]))
    wrong = []
    for raw, label in rej:
        assert wm.decode(group, fmt, raw) is wm.REJECT
        for at in (0, 256):
            msg = _try_upload(ps_api, ctx, gid, fid, b"".join(good[:at] + [raw] + good[at + 1:]))
            if not msg.startswith("1 point(s)"):
                wrong.append((label, at, msg))
            if ps_api.Points.upload(ctx, gid, b"".join(good), fid).download() != want:
                wrong.append((label, at, "the upload after it"))
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("group,fmt", CASES, ids=IDS)
def test_device_counts_bad_points_across_blocks(ps_api, ctx, valid, group, fmt):
    gid, fid = _ids(ps_api, group, fmt)
    _, rej = wm.split_table(group, fmt)
    rows = _wire(group, fmt, valid[group][:N_REJ])
    want = b"".join(_wire(group, wm.COMPRESSED, valid[group][:N_REJ]))
    good = b"".join(rows)
    picks = [rej[k * len(rej) // 5] for k in range(5)]
    assert len({raw for raw, _ in picks}) == 5
    for at, (raw, _label) in zip((0, 255, 256, 511, 512), picks):
        rows[at] = raw
    msg = _try_upload(ps_api, ctx, gid, fid, b"".join(rows))
    assert msg.startswith("5 point(s)"), (msg, [label for _, label in picks])
    assert ps_api.Points.upload(ctx, gid, good, fid).download_compressed() == want


@pytest.mark.gpu
@pytest.mark.parametrize("group", [wm.G1, wm.G2])
def test_device_subgroup_check_with_one_intruder(ps_api, ctx, valid, off_subgroup, group):
    """One point outside the subgroup among 513 inside it, at both ends and on both sides of a block boundary.  (0, 2) has
    order 3: the 255-step ladder of [r]P meets P + P and P + (-P) at nearly every step."""
    gid, _ = _ids(ps_api, group, wm.AFFINE)
    n = N_REJ
    rows = _wire(group, wm.AFFINE, valid[group][:n])
    wrong = []
    for name, pt in _intruders(group, off_subgroup):
        for at in (0, 255, 256, 512):
            arr = ps_api.Points.upload(ctx, gid, b"".join(rows[:at] + [wm.encode_uncompressed(group, pt)] + rows[at + 1:]))
            got = (arr.in_subgroup(), arr.slice(at, 1).in_subgroup(), arr.slice(0, at).in_subgroup(), arr.slice(at + 1, n - at - 1).in_subgroup())
            if got != (False, False, True, True):
                wrong.append((name, at, got))
    assert not wrong, wrong


@pytest.mark.gpu
@pytest.mark.parametrize("group", [wm.G1, wm.G2])
def test_device_subgroup_check_of_identities_and_of_nothing(ps_api, ctx, group):
    gid, _ = _ids(ps_api, group, wm.AFFINE)
    ident = ps_api.Points.upload(ctx, gid, wm.encode_uncompressed(group, None) * N_REJ)
    assert ident.in_subgroup() and ident.download_compressed() == wm.encode_compressed(group, None) * N_REJ
    empty = ps_api.Points.upload(ctx, gid, b"")
    assert len(empty) == 0 and empty.in_subgroup() and empty.download() == b""
