"""Inputs and exact expected values for tests/test_quotient_shapes_gpu.py, on the CPU alone.

Large vectors are built as big-endian byte strings with numpy (the form Poly.upload and the oracle take), circuits as numpy CSR
triples for QAP.from_csr together with the same circuit as a restate.SparseR1CS and its exact L.s, R.s, O.s.  Nothing here
touches the GPU; tests/test_quotient_shapes_gpu.py checks these helpers against the oracle without one.
"""
from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from oracle import coracle as co
from oracle import pyref as pr
from oracle import restate as rs

R = pr.R
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

# ---------------------------------------------------------------------------------------
# NTT pass shapes (playsnark_amd/csrc/ntt.hpp: NTT_TILE_LOG, NTT_MAX_K, the split of ntt_run / ntt_conv)
# ---------------------------------------------------------------------------------------
NTT_TILE_LOG, NTT_MAX_K = 10, 9


def ilog2_ceil(v: int) -> int:
    return max(0, (v - 1).bit_length())


def ntt_passes(p: int) -> tuple:
    """Stages per pass of a 2^p-point transform, forward order (the inverse walks them back)."""
    npass = 1 if p <= NTT_TILE_LOG else -(-p // NTT_MAX_K)
    ks, left = [], p
    for i in range(npass):
        ks.append(-(-left // (npass - i)))
        left -= ks[-1]
    return tuple(ks)


def quotient_conv_sizes(n: int) -> dict:
    """log2 sizes of the convolutions (ntt_conv) a quotient at n gates runs, by route, and the branches of qap_tables_build."""
    lognp = ilog2_ceil(max(n, 64))
    lognp_h = ilog2_ceil(max(n - 1, 64))
    pp, ph = ilog2_ceil(2 * n - 1), ilog2_ceil(max(2 * (n - 1) - 1, 1))
    return {
        "interpolate": {lognp + 1} | set(range(7, lognp + 1)),       # y -> Newton, then the Newton -> monomial levels
        "h_values": {lognp + 1},                                       # the batch of three convolutions with 1/d
        "h_interpolate": {lognp_h + 1} | set(range(7, lognp_h + 1)),  # h from its values on n+1..2n-1
        "product": {pp, ph},                                           # A*B, then the inverse series of rev(z)
        "n_is_np": n == 1 << lognp,
        "np_h_differs": lognp_h != lognp,
    }


# ---------------------------------------------------------------------------------------
# vectors of Fr as big-endian bytes
# ---------------------------------------------------------------------------------------
def random_fr_bytes(n: int, seed: int) -> bytes:
    """n values below 0x73 * 2^248 < r (0.9 r), uniform there: 32 random bytes each, the top byte drawn below 0x73."""
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 0] = g.integers(0, 0x73, size=n, dtype=np.uint8)
    return a.tobytes()


def small_fr_bytes(values) -> bytes:
    """Non-negative values below 2^64 as 32-byte big-endian words."""
    v = np.asarray(values, dtype=np.uint64)
    a = np.zeros((len(v), 4), dtype=">u8")
    a[:, 3] = v
    return a.tobytes()


def const_fr_bytes(n: int, value: int) -> bytes:
    return pr.fr_to_be32(value) * n


def monomial_bytes(n: int, i: int, value: int = 1) -> bytes:
    """x^i * value as n coefficients."""
    a = bytearray(32 * n)
    a[32 * i : 32 * i + 32] = pr.fr_to_be32(value)
    return bytes(a)


def ints(raw: bytes) -> list:
    return [int.from_bytes(raw[i : i + 32], "big") for i in range(0, len(raw), 32)]


def eval_bytes(raw: bytes, x: int) -> int:
    """p(x) for the coefficients p in raw (the oracle's Horner loop, without a round trip through Python ints)."""
    o = C.create_string_buffer(32)
    co.lib().or_poly_eval(raw, C.c_size_t(len(raw) // 32), pr.fr_to_be32(x), o)
    return int.from_bytes(o.raw, "big")


def conv_coeff(a: bytes, b: bytes, i: int) -> int:
    """Coefficient i of a*b as one O(n) convolution sum in Python integers."""
    na, nb = len(a) // 32, len(b) // 32
    lo, hi = max(0, i - (nb - 1)), min(i, na - 1)
    if lo > hi:
        return 0
    av = ints(a[32 * lo : 32 * (hi + 1)])
    bv = ints(b[32 * (i - hi) : 32 * (i - lo + 1)])
    return sum(map(operator.mul, av, reversed(bv))) % R


def all_minus_one_product(na: int, nb: int) -> bytes:
    """(r-1) (1 + x + .. + x^(na-1)) times the same of nb terms: (r-1)^2 = 1, so c_k counts the pairs i + j = k."""
    k = np.arange(na + nb - 1, dtype=np.int64)
    c = np.minimum(np.minimum(k + 1, na + nb - 1 - k), min(na, nb))
    return small_fr_bytes(c)


def mul_length_pairs(p: int) -> list:
    """(na, nb) with ilog2_ceil(na + nb - 1) == p: the exact power of two, just over 2^(p-1), and one skewed pair."""
    pairs = [(1 << (p - 1), (1 << (p - 1)) + 1)]
    over = (1 << (p - 1)) + 2  # na + nb
    pairs.append((over // 2, over - over // 2))
    if p >= 3 and p % 2 == 0:
        pairs.append(((1 << p) - 7, 8))
    else:
        pairs.append((1, 1 << p))
    out = []
    for pr_ in pairs:
        if pr_ not in out:
            out.append(pr_)
    return out


# ---------------------------------------------------------------------------------------
# circuits
# ---------------------------------------------------------------------------------------
def csr_of(rows) -> tuple:
    """rows[g] = [(col, int64 value), ..] -> (row_ptr u32, col u32, val i64) for QAP.from_csr."""
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint32)
    np.cumsum(lens, out=row_ptr[1:])
    col = np.fromiter((c for r in rows for c, _ in r), dtype=np.uint32, count=int(lens.sum()))
    val = np.fromiter((v for r in rows for _, v in r), dtype=np.int64, count=int(lens.sum()))
    return row_ptr, col, val


def dot(row, sol) -> int:
    return sum(v * sol[c] for c, v in row) % R


class Builder:
    """A satisfiable R1CS grown gate by gate.  Variable 0 is the constant 1, then `inputs` free variables of value `value(i)`;
    every gate adds one fresh output variable o: L.s * R.s = o + E.s, with E (extra entries of O) over earlier variables, so
    o's value is exact in Python integers."""

    def __init__(self, inputs: int, value):
        self.sol = [1] + [value(i) % R for i in range(inputs)]
        self.left, self.right, self.out = [], [], []

    @property
    def nvars(self):
        return len(self.sol)

    def gate(self, L, Rr, E=()):
        o = self.nvars
        val = (dot(L, self.sol) * dot(Rr, self.sol) - dot(E, self.sol)) % R
        self.sol.append(val)
        self.left.append(list(L))
        self.right.append(list(Rr))
        self.out.append([(o, 1)] + list(E))
        return o

    def circuit(self, nb_io: int = 2) -> rs.SparseR1CS:
        return rs.SparseR1CS(self.nvars, nb_io, self.left, self.right, self.out)


def fill_short_gates(b: Builder, n: int, seed: int):
    """Short gates (1-2 entries, small coefficients, like the tiled toy) up to n gates in all."""
    g = np.random.default_rng(seed)
    while len(b.left) < n:
        i, j, k = (int(x) for x in g.integers(0, b.nvars, size=3))
        b.gate([(i, 1), (k, 3)] if len(b.left) % 3 == 0 else [(i, 1)], [(j, 1)])


COEF_CLASSES = ("minus_one", "one", "minus_two", "int64_min", "int64_max", "random")
DENSE_LENGTHS = (1, 31, 32, 33, 64, 511, 512, 513, 8191, 8192, 8193, 100_003)


def coefs(kind: str, m: int, g: np.random.Generator) -> list:
    if kind == "random":
        return [int(v) for v in g.integers(INT64_MIN, INT64_MAX, size=m, dtype=np.int64, endpoint=True)]
    v = {"minus_one": -1, "one": 1, "minus_two": -2, "int64_min": INT64_MIN, "int64_max": INT64_MAX}[kind]
    return [v] * m


def dense_row(m: int, nvars: int, kind: str, g: np.random.Generator) -> list:
    """m entries over the variables 0..nvars-1, with at least one column repeated when m > 1 (the last entry repeats the
    first) -- and many more once m exceeds nvars."""
    cols = [int(c) for c in (np.arange(m, dtype=np.int64) * 7919 + int(g.integers(0, nvars))) % nvars]
    if m > 1:
        cols[-1] = cols[0]
    return list(zip(cols, coefs(kind, m, g)))


def dense_circuit(kind: str, witness: str, n: int, lengths=DENSE_LENGTHS, inputs: int = 1024, seed: int = 1):
    """One gate per row length whose L row is dense (coefficients of class `kind`) and whose R row is one entry, then short
    gates up to n.  witness 'minus_one': every free variable is r - 1; 'random': random values.  Gate j < len(lengths) is the
    dense gate of row length lengths[j]."""
    g = np.random.default_rng(seed)
    rnd = ints(random_fr_bytes(inputs, seed))
    b = Builder(inputs, (lambda i: R - 1) if witness == "minus_one" else rnd.__getitem__)
    for m in lengths:
        b.gate(dense_row(m, b.nvars, kind, g), [(1 + len(b.left) % inputs, 1)])
    fill_short_gates(b, n, seed + 1)
    return b


def transposed_long_circuit(n: int = 1025, seed: int = 3):
    """Dense gates (the row lengths of DENSE_LENGTHS up to 8193, random coefficients) and short ones up to n, with long rows
    in the transposed matrices as well: variable 1 is in every gate's L row with coefficient -1 (n > 512 entries), variable 2
    in exactly 512 R rows (the last length the per-row kernel owns) and the constant in 513 O rows."""
    g = np.random.default_rng(seed)
    b = Builder(32, ints(random_fr_bytes(32, seed)).__getitem__)
    lengths = [m for m in DENSE_LENGTHS if m < 10_000]
    for j in range(n):
        if j < len(lengths):
            L = dense_row(lengths[j], b.nvars, "random", g)
        else:
            L = [(int(g.integers(3, b.nvars)), int(g.integers(-5, 6)) or 1)]
        L = L + [(1, -1)]
        Rr = [(2, 1)] if j < 512 else [(int(g.integers(3, b.nvars)), 1)]
        if j % 7 == 3:
            Rr = Rr + [(0, 2)]
        E = [(0, int(g.integers(-9, 10)) or 1)] if j < 513 else []
        b.gate(L, Rr, E)
    return b


def values_bytes(c: rs.SparseR1CS, sol) -> tuple:
    """(L.s, R.s, O.s) of a circuit as byte strings for co.fast_quotient_bytes."""
    return tuple(co.pack_fr(v) for v in c.values(sol))


def permutation_circuit(n: int, seed: int):
    """n gates x_j * x_{(5j+1) mod n} = o_j over random x, as numpy CSR (no Python row lists: n reaches 2^20).  Variables
    [const, x_1..x_n, o_1..o_n].  Returns (nbVars, nbIO, (L, R, O) CSR triples, witness bytes, (yA, yB, yC) bytes)."""
    xb = random_fr_bytes(n, seed)
    x = ints(xb)
    perm = (5 * np.arange(n, dtype=np.int64) + 1) % n
    o = [x[j] * x[k] % R for j, k in enumerate(perm.tolist())]
    ob = co.pack_fr(o)
    ptr = np.arange(n + 1, dtype=np.uint32)
    ones = np.ones(n, dtype=np.int64)
    L = (ptr, (1 + np.arange(n)).astype(np.uint32), ones)
    Rm = (ptr, (1 + perm).astype(np.uint32), ones)
    O = (ptr, (1 + n + np.arange(n)).astype(np.uint32), ones)
    sol = pr.fr_to_be32(1) + xb + ob
    yB = b"".join(xb[32 * k : 32 * k + 32] for k in perm.tolist())
    return 2 * n + 1, 2, (L, Rm, O), sol, (xb, yB, ob)
