"""Big-integer model of the group law on XYZZ points (playsnark_amd/csrc/curve.hpp, qtail.hpp), for the tests only.

Built on oracle/pyref.py (G1, G2, f2_*) and tests/field_model.py.  A point is (X, Y, ZZ, ZZZ) with x = X / ZZ, y = Y / ZZZ and
ZZ^3 = ZZZ^2; the identity is any point with ZZ = 0.  Two references:
  * geometric: the affine chord-and-tangent law of the oracle (pyref._Grp.add) over Python integers, the identity as None --
    for operands on the curve;
  * formula level: add-2008-s and dbl-2008-s evaluated mod p on ARBITRARY field values, the branch chosen by the same
    equalities mod p the device code uses (q_add, xyzz_add_inl: ZZ2 = 0, ZZ1 = 0, u1 = u2, s1 = s2) -- for operands off the
    curve whose limbs sit at the edge of the lazy-limb contract, where only the formulas define the answer.
test_device_tail.py shows that the two agree on on-curve operands, exceptional cases included.

Field elements are Python integers mod p (G1) or pairs of them (G2); limbs are Montgomery form (field_model.fp_mont).
"""
from __future__ import annotations

import numpy as np

import field_model as fm
from oracle import pyref as pr

P = fm.P
RINV = pow(fm.FP_RM, -1, P)

# the branches of an addition A + B, in the order the code tests for them
B_IDENTITY, A_IDENTITY, DOUBLE, CANCEL, GENERAL = "b_identity", "a_identity", "double", "cancel", "general"
BRANCHES = (B_IDENTITY, A_IDENTITY, DOUBLE, CANCEL, GENERAL)


class Curve:
    """One group: its oracle, the width of a coordinate in limbs and the packing of points into words."""

    def __init__(self, name):
        self.name = name
        self.f2 = name == "g2"
        self.grp = pr.G2 if self.f2 else pr.G1
        self.comps = 2 if self.f2 else 1
        self.W = fm.FP_L * self.comps  # words of a coordinate
        self.PT = 4 * self.W           # words of a point: x, y, zz, zzz (struct order)
        self.GL = 4 * self.comps       # lanes of a point in quad form
        self.NPB = 256 // self.GL      # points of a 256-thread block
        g = self.grp
        self.add, self.sub, self.mul, self.inv, self.neg = g.fadd, g.fsub, g.fmul, g.finv, g.fneg
        self.zero, self.one = g.zero, g.one

    # ---- field values ----
    def rand(self, rng):
        v = [int.from_bytes(rng.bytes(56), "little") % P for _ in range(self.comps)]
        return tuple(v) if self.f2 else v[0]

    def rand_nonzero(self, rng):
        while True:
            v = self.rand(rng)
            if v != self.zero:
                return v

    def comps_of(self, v):
        return list(v) if self.f2 else [v]

    def from_comps(self, c):
        return tuple(c) if self.f2 else c[0]

    def enc(self, v):
        """canonical Montgomery limbs of a field value"""
        return sum((fm.fp_mont(c) for c in self.comps_of(v)), [])

    def dec(self, words):
        """the field value any lazy limbs stand for"""
        return self.from_comps([fm.to_int(words[fm.FP_L * k:fm.FP_L * (k + 1)]) * RINV % P for k in range(self.comps)])

    # ---- points ----
    def rep(self, pt, lam):
        """the affine point (None: the identity) as (lam^2 x, lam^3 y, lam^2, lam^3); the identity as all zeros"""
        if pt is None:
            return (self.zero,) * 4
        l2 = self.mul(lam, lam)
        l3 = self.mul(l2, lam)
        return (self.mul(pt[0], l2), self.mul(pt[1], l3), l2, l3)

    def rand_rep(self, pt, rng):
        return self.rep(pt, self.rand_nonzero(rng))

    def pack(self, xyzz):
        """field values (X, Y, ZZ, ZZZ) -> the words of the struct, canonical limbs"""
        return sum((self.enc(c) for c in xyzz), [])

    def unpack(self, words):
        """words of a struct -> field values (X, Y, ZZ, ZZZ)"""
        return tuple(self.dec(words[self.W * j:self.W * (j + 1)]) for j in range(4))

    def is_identity(self, xyzz):
        return xyzz[2] == self.zero

    def affine(self, xyzz):
        if self.is_identity(xyzz):
            return None
        return (self.mul(xyzz[0], self.inv(xyzz[2])), self.mul(xyzz[1], self.inv(xyzz[3])))

    def consistent(self, xyzz):
        """ZZ^3 = ZZZ^2"""
        zz, zzz = xyzz[2], xyzz[3]
        return self.mul(self.mul(zz, zz), zz) == self.mul(zzz, zzz)

    def multiples(self, base, lo=-3, hi=3):
        """{m: m base} for lo <= m <= hi (0: None)"""
        out = {0: None}
        acc = None
        for m in range(1, max(hi, -lo) + 1):
            acc = self.grp.add(acc, base)
            out[m], out[-m] = acc, self.grp.neg(acc)
        return {m: out[m] for m in range(lo, hi + 1)}

    def times(self, k, base):
        """k base for any integer k (the oracle's Mul reduces mod r)"""
        k %= pr.R
        return None if k == 0 else self.grp.mul(k, base)

    # ---- formula level ----
    def classify(self, A, B):
        if B[2] == self.zero:
            return B_IDENTITY
        if A[2] == self.zero:
            return A_IDENTITY
        u1, u2 = self.mul(A[0], B[2]), self.mul(B[0], A[2])
        if u1 != u2:
            return GENERAL
        s1, s2 = self.mul(A[1], B[3]), self.mul(B[1], A[3])
        return DOUBLE if s1 == s2 else CANCEL

    def formula_dbl(self, A):
        """dbl-2008-s-1 (a = 0), as xyzz_dbl"""
        X, Y, ZZ, ZZZ = A
        if ZZ == self.zero:
            return A
        mul, sub, add = self.mul, self.sub, self.add
        u = add(Y, Y)
        v = mul(u, u)
        w = mul(u, v)
        s = mul(X, v)
        xx = mul(X, X)
        m = add(add(xx, xx), xx)
        x3 = sub(sub(mul(m, m), s), s)
        y3 = sub(mul(m, sub(s, x3)), mul(w, Y))
        return (x3, y3, mul(v, ZZ), mul(w, ZZZ))

    def formula_add(self, A, B):
        """(A + B, branch) by add-2008-s on whatever field values A and B hold"""
        kind = self.classify(A, B)
        if kind == B_IDENTITY:
            return A, kind
        if kind == A_IDENTITY:
            return B, kind
        if kind == DOUBLE:
            return self.formula_dbl(A), kind
        if kind == CANCEL:
            return (self.zero,) * 4, kind
        mul, sub = self.mul, self.sub
        u1, u2 = mul(A[0], B[2]), mul(B[0], A[2])
        s1, s2 = mul(A[1], B[3]), mul(B[1], A[3])
        p, r = sub(u2, u1), sub(s2, s1)
        pp = mul(p, p)
        ppp = mul(p, pp)
        q = mul(u1, pp)
        x3 = sub(sub(sub(mul(r, r), ppp), q), q)
        y3 = sub(mul(r, sub(q, x3)), mul(s1, ppp))
        return (x3, y3, mul(mul(A[2], B[2]), pp), mul(mul(A[3], B[3]), ppp)), kind


G1, G2 = Curve("g1"), Curve("g2")
CURVES = {"g1": G1, "g2": G2}


# ---- limbs of many values at once ----
def ints_to_limbs(vals):
    """canonical limbs (cases, 14) of non-negative integers below 2^392"""
    a = np.array(list(vals), dtype=object)
    out = np.empty((len(a), fm.FP_L), dtype=np.int64)
    for i in range(fm.FP_L):
        out[:, i] = ((a >> (fm.B * i)) & fm.MASK).astype(np.int64)
    return out


def pack_points(cv: Curve, points):
    """field-value points -> (n, PT) words, canonical Montgomery limbs"""
    vals = [c * fm.FP_RM % P for pt in points for coord in pt for c in cv.comps_of(coord)]
    return ints_to_limbs(vals).reshape(len(points), cv.PT)


def limb_values(rows):
    """the integer every row of limbs holds"""
    a = np.asarray(rows, dtype=np.int64).astype(object)
    w = np.array([1 << (fm.B * i) for i in range(a.shape[-1])], dtype=object)
    return (a * w).sum(axis=-1)
