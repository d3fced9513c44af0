"""Big-integer model of the product's lazy-limb field arithmetic (playsnark_amd/csrc/field.hpp), for the tests only.

Plain Python and numpy; no torch, no oracle code.  Three parts:
  * limbs <-> integers and the residue every operation must produce (a b R^-1 mod p, ...);
  * operand generators that mirror tests/host_limb_check.cpp (worst-case limbs of every class and sign pattern, random lazy
    operands) plus hand-picked edges (0, 1, p - 1, k p in several limb layouts, f_is_zero filter values, canon range ends);
  * an EXACT emulation, in signed 64-bit column arithmetic, of the two product algorithms the device runs: product scanning
    (f_mul and the fused forms, which fp_chain.inc reproduces term for term) and the negated-domain Fr chain
    (tools/gen_fr_chain.py).  Every emulation takes arrays of limbs of shape (cases, L).  With dtype=object the arithmetic is
    unbounded and the emulation also returns the largest |accumulator| it met, multiply-add by multiply-add in the device's
    term order; with dtype=int64 it is the fast form for large random sets (inside the contract, where the exact form shows
    that no column leaves 64 bits, the two agree).
"""
from __future__ import annotations

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
B = 28
MASK = (1 << B) - 1
FP_L, FR_L = 14, 10
FP_RM = 1 << (B * FP_L)  # Montgomery R of Fp: 2^392
FR_RM = 1 << (B * FR_L)  # Montgomery R of Fr: 2^280
FP_MOD = [(P >> (B * i)) & MASK for i in range(FP_L)]
FR_MOD = [(R >> (B * i)) & MASK for i in range(FR_L)]
FP_INV28 = (-pow(P, -1, 1 << B)) % (1 << B)
FR_INV28 = (-pow(R, -1, 1 << B)) % (1 << B)
TOP_SPAN = 15 * FP_MOD[FP_L - 1]  # host_limb_check.cpp: |value| <= 16 p bounds the top limb
FR_TOP_SPAN = 63 * FR_MOD[FR_L - 1]  # host_limb_check.cpp: |value| < 64 r
I64_LIM = 1 << 63


# ---------------------------------------------------------------------------------------------------------------------------
# limbs <-> integers
# ---------------------------------------------------------------------------------------------------------------------------
def to_int(limbs) -> int:
    return sum(int(x) << (B * i) for i, x in enumerate(limbs))


def from_int(v: int, L: int) -> list:
    """The carried form fp_propagate / fr_propagate give: limbs 0..L-2 in [0, 2^28), signed top limb."""
    out = []
    for _ in range(L - 1):
        out.append(v & MASK)
        v >>= B
    out.append(v)
    return out


def rows_to_ints(a) -> list:
    return [to_int(row) for row in np.asarray(a, dtype=object)]


def i32(x):
    """(i32) of a 64-bit value: two's-complement truncation, elementwise."""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def limb_class(a) -> np.ndarray:
    """Per row: the smallest c with |limb| < c 2^28 for every limb."""
    a = np.asarray(a, dtype=np.int64)
    return (np.abs(a).max(axis=1) >> B) + 1


def fp_mont(x: int) -> list:
    return from_int(x * FP_RM % P, FP_L)


def fr_mont(x: int) -> list:
    return from_int(x * FR_RM % R, FR_L)


def fp_val(limbs) -> int:
    """The field element a Montgomery-form Fp value stands for."""
    return to_int(limbs) * pow(FP_RM, -1, P) % P


def fr_val(limbs) -> int:
    return to_int(limbs) * pow(FR_RM, -1, R) % R


# ---------------------------------------------------------------------------------------------------------------------------
# operand generators (host_limb_check.cpp's, plus edges)
# ---------------------------------------------------------------------------------------------------------------------------
def worst(cls: int, pattern: int, rng, L=FP_L, top=TOP_SPAN) -> list:
    """Every limb at the edge of class cls (the top limb at the edge of |V| <= 16 p); pattern 0: all +, 1: all -,
    2: alternating, 3: random signs."""
    out = []
    for i in range(L):
        v = top if i == L - 1 else (cls << B) - 1
        neg = pattern == 1 or (pattern == 2 and i & 1) or (pattern == 3 and rng.integers(2))
        out.append(-v if neg else v)
    return out


def fr_worst(cls: int, pattern: int, rng) -> list:
    return worst(cls, pattern, rng, FR_L, FR_TOP_SPAN)


def random_lazy(cls: int, n: int, rng, L=FP_L, top=TOP_SPAN) -> np.ndarray:
    span = np.array([(cls << B) - 1] * (L - 1) + [top], dtype=np.int64)
    return rng.integers(-span, span + 1, size=(n, L), dtype=np.int64)


def random_canon(n: int, rng, mod=P, L=FP_L) -> np.ndarray:
    return np.array([from_int(int.from_bytes(rng.bytes(56), "little") % mod, L) for _ in range(n)], dtype=np.int64)


def relayout(limbs, cls: int, rng, L=FP_L) -> list:
    """The same value in another lazy layout inside class cls: random borrows between neighbouring limbs."""
    l = [int(x) for x in limbs]
    lim = (cls << B) - 1
    for _ in range(4 * L):
        i = int(rng.integers(L - 1))
        t = int(rng.integers(-cls, cls + 1))
        a, b = l[i] + (t << B), l[i + 1] - t
        if abs(a) <= lim and abs(b) <= lim:
            l[i], l[i + 1] = a, b
    return l


def fp_zero_edges(rng) -> list:
    """f_is_zero / fp_is_zero_exact cases inside the contract (class <= 8, |V| <= 16 p): k p for |k| <= 16 in several layouts,
    k p +- 1, non-zero values whose limb 0 is 0, and values whose filter value q = (V mod 2^28) p^-1 mod 2^28 is 0, 16, 32,
    33, 2^28 - 33 and 2^28 - 32 (the filter's boundaries)."""
    out = []
    for k in range(-16, 17):
        base = from_int(k * P, FP_L)
        out.append(base)
        if abs(k) <= 7:
            out.append([k * m for m in FP_MOD])  # limb by limb
        for cls in (2, 4, 8):
            out.append(relayout(base, cls, rng))
        if abs(k) < 16:
            out.append(relayout(from_int(k * P + 1, FP_L), 8, rng))
            out.append(relayout(from_int(k * P - 1, FP_L), 8, rng))
    pinv = pow(P, -1, 1 << B)
    for q in (0, 16, 32, 33, (1 << B) - 33, (1 << B) - 32, 1, (1 << B) - 1):
        for _ in range(8):
            hi =int.from_bytes(rng.bytes(48), "little") % (8 * P) - 4 * P
            l0 = q * P % (1 << B)
            v = (hi >> B << B) + l0
            out.append(relayout(from_int(v, FP_L), 4, rng))
            assert (to_int(out[-1]) & MASK) * pinv % (1 << B) == q
    for _ in range(16):  # limb 0 is zero, value is not
        v = (int.from_bytes(rng.bytes(48), "little") % (8 * P)) >> B << B
        out.append(from_int(v, FP_L))
    return out


def canon_edges(mod, L, rng) -> list:
    """fp_canon / fr_canon: values at the ends of (-2 mod, 3 mod) and around 0, mod, 2 mod, in lazy layouts up to class 7
    (their carry chain adds the carry to a limb in 32 bits: a class-8 limb plus a carry leaves int32)."""
    vals = [-2 * mod + 1, -2 * mod + 2, -mod - 1, -mod, -mod + 1, -1, 0, 1, mod - 1, mod, mod + 1, 2 * mod - 1, 2 * mod,
            2 * mod + 1, 3 * mod - 2, 3 * mod - 1]
    out = []
    for v in vals:
        base = from_int(v, L)
        out.append(base)
        for cls in (2, 7):
            out.append(relayout(base, cls, rng, L))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# exact emulation of the products
# ---------------------------------------------------------------------------------------------------------------------------
class Peak:
    """Largest |accumulator| met (exact mode only)."""

    def __init__(self, on: bool):
        self.on, self.v = on, 0

    def see(self, acc):
        if self.on:
            m = max(abs(int(x)) for x in acc)
            if m > self.v:
                self.v = m


def _col(a, i):
    return a[:, i]


def fp_prodscan(col_terms, n, dtype, track=False):
    """Product scanning with one accumulator, in the device chain's term order: column k first the operand products that
    col_terms(k) lists (pairs of limb columns), then m_i p_(k-i), then the Montgomery digit m_k and m_k p_0, then >> 28."""
    acc = np.zeros(n, dtype=dtype)
    peak = Peak(track)
    m = [None] * FP_L
    r = [None] * FP_L
    for k in range(2 * FP_L - 1):
        for x, y in col_terms(k):
            acc = acc + x * y
            peak.see(acc)
        for i in (range(0, k) if k < FP_L else range(k - FP_L + 1, FP_L)):
            acc = acc + m[i] * FP_MOD[k - i]
            peak.see(acc)
        if k < FP_L:
            m[k] = ((acc & MASK) * FP_INV28) & MASK
            acc = acc + m[k] * FP_MOD[0]
            peak.see(acc)
            acc = acc >> B
        else:
            r[k - FP_L] = acc & MASK
            acc = acc >> B
    r[FP_L - 1] = i32(acc)
    return np.stack(r, axis=1), peak.v


def _as(a, dtype):
    return np.asarray(a, dtype=np.int64).astype(dtype)


def _span(k, L):
    return range(max(0, k - L + 1), min(k, L - 1) + 1)


def fp_mulsum(prods, track=False, dtype=np.int64):
    """sum_q (+/-) a_q b_q under one reduction: f_mul (one product), f_mul2sub / f_mul2add (two), f_mul2add2sub (four).
    prods: list of (a, b, negate).  The chain negates the subtracted left operands (nc = -c) and multiplies-adds them."""
    ops = []
    for a, b, neg in prods:
        a, b = _as(a, dtype), _as(b, dtype)
        ops.append((-a if neg else a, b))
    n = ops[0][0].shape[0]
    return fp_prodscan(lambda k: [(x[:, i], y[:, k - i]) for x, y in ops for i in _span(k, FP_L)], n, dtype, track)


def fp_mul(a, b, track=False, dtype=np.int64):
    return fp_mulsum([(a, b, False)], track, dtype)


def fp_sqr(a, track=False, dtype=np.int64):
    """f_sqr_chain: 2 a_i a_(k-i) for 2i < k, then a_(k/2)^2."""
    a = _as(a, dtype)
    a2 = a + a

    def terms(k):
        t = [(a2[:, i], a[:, k - i]) for i in _span(k, FP_L) if 2 * i < k]
        if k % 2 == 0:
            t.append((a[:, k // 2], a[:, k // 2]))
        return t

    return fp_prodscan(terms, a.shape[0], dtype, track)


def fp_mulsum_ilp(prods, track=False, dtype=np.int64):
    """f_mulsum_ilp: every column its own accumulator, the products first, then the reduction column by column."""
    col = [np.zeros(np.asarray(prods[0][0]).shape[0], dtype=dtype) for _ in range(2 * FP_L)]
    peak = Peak(track)
    for a, b, neg in prods:
        a, b = _as(a, dtype), _as(b, dtype)
        for i in range(FP_L):
            for j in range(FP_L):
                col[i + j] = col[i + j] - a[:, i] * b[:, j] if neg else col[i + j] + a[:, i] * b[:, j]
                peak.see(col[i + j])
    for k in range(FP_L):
        m = ((col[k] & MASK) * FP_INV28) & MASK
        for j in range(FP_L):
            col[k + j] = col[k + j] + m * FP_MOD[j]
            peak.see(col[k + j])
        col[k + 1] = col[k + 1] + (col[k] >> B)
        peak.see(col[k + 1])
    r = []
    for k in range(FP_L, 2 * FP_L - 1):
        r.append(col[k] & MASK)
        col[k + 1] = col[k + 1] + (col[k] >> B)
        peak.see(col[k + 1])
    r.append(i32(col[2 * FP_L - 1]))
    return np.stack(r, axis=1), peak.v


def fr_mul_chain(a, b, track=False, dtype=np.int64):
    """fr_chain.inc: the negated domain.  N_k = -(column sum): the operand products as (-a_i) b_j, the modulus as -r_j,
    Montgomery digit m_k = N_k mod 2^28 (r = 1 mod 2^28), carry N_k >> 28 (the floor of the negated sum is the negated
    ceiling the positive sum needs), and the result limbs -(N_k mod 2^28): in (-2^28, 0]."""
    a, b = _as(a, dtype), _as(b, dtype)
    na = -a
    n = a.shape[0]
    acc = np.zeros(n, dtype=dtype)
    peak = Peak(track)
    m = [None] * FR_L
    r = [None] * FR_L
    for k in range(2 * FR_L - 1):
        for i in _span(k, FR_L):
            acc = acc + na[:, i] * b[:, k - i]
            peak.see(acc)
        for i in (range(0, k) if k < FR_L else range(k - FR_L + 1, FR_L)):
            acc = acc + m[i] * (-FR_MOD[k - i])
            peak.see(acc)
        if k < FR_L:
            m[k] = acc & MASK
        else:
            r[k - FR_L] = -(acc & MASK)
        acc = acc >> B
    r[FR_L - 1] = -i32(acc)
    return np.stack(r, axis=1), peak.v


def fr_mul_cpp(a, b, track=False, dtype=np.int64):
    """field.hpp's C++ fr_mul (the host form, and the device's with -DPS_FR_MUL_NO_CHAIN): positive domain, digit
    m_k = -acc mod 2^28, carry (acc + 2^28 - 1) >> 28, result limbs 0..8 in [0, 2^28)."""
    a, b = _as(a, dtype), _as(b, dtype)
    n = a.shape[0]
    acc = np.zeros(n, dtype=dtype)
    peak = Peak(track)
    m = [None] * FR_L
    r = [None] * FR_L
    for k in range(2 * FR_L - 1):
        for i in _span(k, FR_L):
            acc = acc + a[:, i] * b[:, k - i]
            peak.see(acc)
        for i in (range(0, k) if k < FR_L else range(k - FR_L + 1, FR_L)):
            acc = acc + m[i] * FR_MOD[k - i]
            peak.see(acc)
        if k < FR_L:
            m[k] = (-acc) & MASK
            acc = acc + MASK
            peak.see(acc)
        else:
            r[k - FR_L] = acc & MASK
        acc = acc >> B
    r[FR_L - 1] = i32(acc)
    return np.stack(r, axis=1), peak.v


# ---------------------------------------------------------------------------------------------------------------------------
# the cheap operations, in i32 semantics
# ---------------------------------------------------------------------------------------------------------------------------
def norm(a):
    """f_norm / fr_norm: one parallel carry-save step."""
    a = np.asarray(a, dtype=np.int64)
    L = a.shape[1]
    r = np.empty_like(a)
    r[:, 0] = a[:, 0] & MASK
    r[:, 1:L - 1] = (a[:, 1:L - 1] & MASK) + (a[:, 0:L - 2] >> B)
    r[:, L - 1] = i32(a[:, L - 1] + (a[:, L - 2] >> B))
    return r


def propagate(a):
    a = np.asarray(a, dtype=np.int64)
    L = a.shape[1]
    r = np.empty_like(a)
    c = np.zeros(a.shape[0], dtype=np.int64)
    for i in range(L - 1):
        t = i32(a[:, i] + c)
        r[:, i] = t & MASK
        c = t >> B
    r[:, L - 1] = i32(a[:, L - 1] + c)
    return r


def add(a, b):
    return i32(np.asarray(a, dtype=np.int64) + np.asarray(b, dtype=np.int64))


def sub(a, b):
    return i32(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# the contract, as bounds on the column accumulators
# ---------------------------------------------------------------------------------------------------------------------------
def column_bound(L, mod, class_sum, top=None):
    """An upper bound of |accumulator| over ALL operands inside the contract, for product scanning with the operand
    products' class products adding up to class_sum: column k holds (terms) x class_sum 2^56 from the operands, at most
    L terms m_i p_j < 2^28 p_j from the reduction, and the carry of the column below."""
    carry, worst = 0, 0
    for k in range(2 * L - 1):
        nterm = len(_span(k, L))
        ops = nterm * class_sum << (2 * B)
        red = sum(MASK * mod[k - i] for i in (range(0, k + 1) if k < L else range(k - L + 1, L)))
        tot = ops + red + carry
        worst = max(worst, tot)
        carry = (tot >> B) + 1
    return worst
