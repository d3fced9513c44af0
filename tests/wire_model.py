"""Strict model of the ZCash point encodings of BLS12-381 in plain Python integers, and the table of edge encodings the
point codecs are tested on (tests/test_point_wire.py).

oracle/pyref.py's decoders are lax on purpose (they accept coordinates >= p and ignore flag bits), so they cannot give the
verdict on a malformed encoding.  The decoders here return a point ((x, y), Fp2 elements as (c0, c1)), None for the identity,
or REJECT, by the rules the kernels' comments state:

  uncompressed (96 B G1 / 192 B G2; x then y, an Fp2 element as c1 then c0)
    * the identity is exactly 0x40 followed by zeros;
    * otherwise the top three bits of byte 0 are clear, every coordinate is < p and the curve equation holds.
  compressed (48 B / 96 B)
    * 0x80 is set;
    * the identity is exactly 0xC0 followed by zeros;
    * otherwise x is read with the top three bits of byte 0 masked off (G2: c1 then c0) and is < p, x^3 + b must be a square,
      and the 0x20 bit says whether y is the "larger" root: y > (p-1)/2 in Fp; in Fp2 the comparison is on c1, and on c0 only
      when c1 = 0.

The square root in Fp2 is taken through the norm (sqrt(a0^2 + a1^2) in Fp, then x0^2 = (a0 +- n)/2), not by the complex
method the device uses, so that the two cannot share a mistake.

The "larger" boundary itself cannot be met by a curve point: no point of E(Fp) has y = (p-1)/2 or (p+1)/2, because
y^2 - 4 is not a cube there (asserted in tests/test_point_wire.py).  The comparison at the boundary is therefore covered by
fp_lex_larger's field tests (tests/test_device_field.py), not by this table.
"""
from oracle import pyref as pr

P, R = pr.P, pr.R
HALF = (P - 1) // 2
REJECT = "reject"
G1, G2 = "g1", "g2"
AFFINE, COMPRESSED = "affine", "compressed"
GROUPS = {G1: pr.G1, G2: pr.G2}
WIRE = {G1: 96, G2: 192}


# ---- fields ----
def fp_is_square(a):
    a %= P
    return a == 0 or pow(a, HALF, P) == 1


def fp_sqrt(a):
    """A square root of a in Fp (p = 3 mod 4), or None."""
    a %= P
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a else None


def fp2_sqrt(a):
    """A square root of a = (a0, a1) in Fp[u]/(u^2 + 1), or None, through the norm."""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        return (0, fp_sqrt(-a0))  # -1 is a non-residue: exactly one of a0, -a0 is a square
    n = fp_sqrt(a0 * a0 + a1 * a1)
    if n is None:
        return None
    inv2 = pow(2, P - 2, P)
    x0 = fp_sqrt((a0 + n) * inv2)
    if x0 is None:
        x0 = fp_sqrt((a0 - n) * inv2)
    x1 = a1 * pow(2 * x0, P - 2, P) % P
    assert ((x0 * x0 - x1 * x1) % P, 2 * x0 * x1 % P) == (a0, a1)
    return (x0, x1)


def rhs(group, x):
    """x^3 + b"""
    g = GROUPS[group]
    return g.fadd(g.fmul(g.fmul(x, x), x), g.b)


def lex_larger(group, y):
    if group == G1:
        return y > HALF
    return y[1] > HALF if y[1] != 0 else y[0] > HALF


def neg(group, pt):
    return GROUPS[group].neg(pt)


def on_curve(group, pt):
    return GROUPS[group].on_curve(pt)


def in_subgroup(group, pt):
    """[r]P = O, as (r-1)P + P: the group's mul reduces its scalar mod r."""
    if pt is None:
        return True
    g = GROUPS[group]
    return g.add(g.mul(R - 1, pt), pt) is None


# ---- decoding ----
def _words(raw):
    return [int.from_bytes(raw[i:i + 48], "big") for i in range(0, len(raw), 48)]


def decode_uncompressed(group, raw):
    assert len(raw) == WIRE[group]
    if raw[0] & 0x40:
        return None if raw[0] == 0x40 and not any(raw[1:]) else REJECT
    if raw[0] & 0xE0:
        return REJECT
    w = _words(raw)
    if any(v >= P for v in w):
        return REJECT
    pt = (w[0], w[1]) if group == G1 else ((w[1], w[0]), (w[3], w[2]))
    return pt if on_curve(group, pt) else REJECT


def decode_compressed(group, raw):
    assert len(raw) == WIRE[group] // 2
    if not raw[0] & 0x80:
        return REJECT
    if raw[0] & 0x40:
        return None if raw[0] == 0xC0 and not any(raw[1:]) else REJECT
    w = _words(bytes([raw[0] & 0x1F]) + raw[1:])
    if any(v >= P for v in w):
        return REJECT
    x = w[0] if group == G1 else (w[1], w[0])
    y = fp_sqrt(rhs(group, x)) if group == G1 else fp2_sqrt(rhs(group, x))
    if y is None:
        return REJECT
    if lex_larger(group, y) != bool(raw[0] & 0x20):
        y = GROUPS[group].fneg(y)
    return (x, y)


def decode(group, fmt, raw):
    return decode_uncompressed(group, raw) if fmt == AFFINE else decode_compressed(group, raw)


# ---- encoding (of a point the decoders accept) ----
def _be(*vals):
    return b"".join(v.to_bytes(48, "big") for v in vals)


def encode_uncompressed(group, pt):
    if pt is None:
        return bytes([0x40]) + bytes(WIRE[group] - 1)
    (x, y) = pt
    return _be(x, y) if group == G1 else _be(x[1], x[0], y[1], y[0])


def encode_compressed(group, pt):
    if pt is None:
        return bytes([0xC0]) + bytes(WIRE[group] // 2 - 1)
    (x, y) = pt
    out = bytearray(_be(x) if group == G1 else _be(x[1], x[0]))
    out[0] |= 0x80 | (0x20 if lex_larger(group, y) else 0)
    return bytes(out)


def encode(group, fmt, pt):
    return encode_uncompressed(group, pt) if fmt == AFFINE else encode_compressed(group, pt)


# ---- special points ----
def g1_order3():
    """(0, 2) and (0, p-2): the points of order 3 of E(Fp) with x = 0."""
    return (0, 2), (0, P - 2)


def g2_special():
    """Two points of the twist with x = (x0, t), t = 2, x0 = +-sqrt((t^3 - 4) / (3 t)): the imaginary part of x^3 + 4(1 + u)
    vanishes.  -> (p_real, p_imag): p_real has a right-hand side that is a square in Fp, so y.c1 = 0 and the sign bit is
    decided by y.c0; p_imag has one that is a non-square in Fp, so y.c0 = 0 (the alpha = -1 branch of the complex method)."""
    t = 2
    x0 = fp_sqrt((t ** 3 - 4) * pow(3 * t, P - 2, P))
    assert x0 is not None
    out = {}
    for s in (x0, P - x0):
        x = (s, t)
        a = rhs(G2, x)
        assert a[1] == 0 and a[0] != 0
        y = fp2_sqrt(a)
        out["real" if y[1] == 0 else "imag"] = (x, y)
    return out["real"], out["imag"]


def _flagged(raw, flag):
    out = bytearray(raw)
    out[0] |= flag
    return bytes(out)


def edge_table():
    """[(group, format, bytes, label)]: every entry is decided by decode(); nothing here says which are valid."""
    t = []
    gx, gy = pr.G1.gen
    (hx, hy) = pr.G2.gen

    # compressed G1
    xs = [0, 1, 2, 3, 4, 5, P - 2, P - 1, P, P + 1, (1 << 381) - 1, gx, gx + P]
    for x in xs:
        for flag in (0x80, 0xA0, 0x00, 0x20, 0xC0, 0xE0, 0x40):
            t.append((G1, COMPRESSED, _flagged(_be(x), flag), "x=%#x flag=%#04x" % (x, flag)))
    t.append((G1, COMPRESSED, bytes([0xC1]) + bytes(47), "identity, stray low bit in byte 0"))
    t.append((G1, COMPRESSED, bytes([0xC0]) + bytes(46) + b"\x01", "identity, stray last byte"))

    # compressed G2
    x2s = [(0, 0), (1, 0), (0, 1), (2, 0), (3, 0), (P - 1, 0), (0, P - 1), (P, 0), (0, P), (P - 1, P - 1), hx, (hx[0] + P, hx[1])]
    for x in x2s:
        for flag in (0x80, 0xA0, 0x00, 0xC0, 0xE0):
            t.append((G2, COMPRESSED, _flagged(_be(x[1], x[0]), flag), "x=(%#x, %#x) flag=%#04x" % (x[0], x[1], flag)))
    t.append((G2, COMPRESSED, bytes([0xC1]) + bytes(95), "identity, stray low bit in byte 0"))
    t.append((G2, COMPRESSED, bytes([0xC0]) + bytes(94) + b"\x01", "identity, stray last byte"))
    for name, pt in zip(("real", "imag"), g2_special()):
        for flag in (0x80, 0xA0):
            t.append((G2, COMPRESSED, _flagged(_be(pt[0][1], pt[0][0]), flag), "special x, %s right-hand side, flag=%#04x" % (name, flag)))

    # uncompressed G1
    shapes = [("G", gx, gy), ("(0, 2)", 0, 2), ("(0, p-2)", 0, P - 2), ("(0, 0)", 0, 0), ("(x+p, y)", gx + P, gy), ("(x, y+p)", gx, gy + P),
              ("(x, p-y)", gx, P - gy), ("(x, y^1)", gx, gy ^ 1), ("(p, 2)", P, 2), ("(0, p+2)", 0, P + 2)]
    for name, x, y in shapes:
        for flag in (0, 0x20, 0x80, 0x40):
            t.append((G1, AFFINE, _flagged(_be(x, y), flag), "%s flag=%#04x" % (name, flag)))
    t.append((G1, AFFINE, bytes([0x40]) + bytes(94) + b"\x01", "identity, stray last byte"))

    # uncompressed G2: the same shapes; the four coordinates of a point are (x.c1, x.c0, y.c1, y.c0) in wire order
    # The twist has no point with x = 0 (4 + 4u is not a square), so (0, 2) has no valid counterpart: x = 0 appears with an
    # off-curve y, and the special points, which have a zero coordinate in y, stand in as the second base whose coordinates
    # are raised by p (for them y.c1 + p, or y.c0 + p, is p itself: the alias of zero).
    real, imag = g2_special()
    g2w = [hx[1], hx[0], hy[1], hy[0]]
    realw = [real[0][1], real[0][0], real[1][1], real[1][0]]
    imagw = [imag[0][1], imag[0][0], imag[1][1], imag[1][0]]
    shapes2 = [("G", g2w), ("x = 0, y = 2", [0, 0, 0, 2]), ("x = 0, y = 2u", [0, 0, 2, 0]), ("(0, 0)", [0, 0, 0, 0]),
               ("(x, -y)", [hx[1], hx[0], P - hy[1], P - hy[0]]), ("(x, y^1)", [hx[1], hx[0], hy[1], hy[0] ^ 1]),
               ("special, real root", realw), ("special, imaginary root", imagw),
               ("special, real root, -y", realw[:2] + [0, P - realw[3]]), ("special, imaginary root, -y", imagw[:2] + [P - imagw[2], 0])]
    for base_name, base in (("G", g2w), ("special, real root", realw), ("special, imaginary root", imagw)):
        for k, cname in enumerate(("x.c1", "x.c0", "y.c1", "y.c0")):
            shapes2.append(("%s with %s + p" % (base_name, cname), [v + (P if i == k else 0) for i, v in enumerate(base)]))
    for name, w in shapes2:
        for flag in (0, 0x20, 0x80, 0x40):
            t.append((G2, AFFINE, _flagged(_be(*w), flag), "%s flag=%#04x" % (name, flag)))
    t.append((G2, AFFINE, bytes([0x40]) + bytes(190) + b"\x01", "identity, stray last byte"))

    # a few generic points as a control: for about half of the G2 ones c1 and c0 disagree on "larger"
    for group in (G1, G2):
        for k in range(2, 10):
            pt = GROUPS[group].mul(k)
            t.append((group, AFFINE, encode_uncompressed(group, pt), "%d G" % k))
            xb = encode_compressed(group, pt)
            for flag in (0x80, 0xA0):
                t.append((group, COMPRESSED, bytes([xb[0] & 0x1F | flag]) + xb[1:], "x(%d G) flag=%#04x" % (k, flag)))
    return t


def split_table(group, fmt):
    """(accepted, rejected) entries of one group and format: [(bytes, label, point)] and [(bytes, label)]; duplicates of the
    same bytes dropped."""
    acc, rej, seen = [], [], set()
    for g, f, raw, label in edge_table():
        if (g, f) != (group, fmt) or raw in seen:
            continue
        seen.add(raw)
        pt = decode(g, f, raw)
        if pt is REJECT:
            rej.append((raw, label))
        else:
            acc.append((raw, label, pt))
    return acc, rej
