"""Shared by the tests of field-valued R1CS coefficients (not a test itself): the edge coefficients around the 64-bit limit
of the column sums, a seeded coefficient generator, a satisfiable MiMC-style circuit whose round constants are such
coefficients, and the packing of a matrix for ps_qap_create_fr."""
import numpy as np

from oracle import pyref as pr
from oracle import restate as rs

R = pr.R

# A canonical value v enters a column sum as min(v, r - v); it is "wide" when that magnitude is 2^64 or more.
EDGE = (
    (1 << 64) - 1,        # narrow, but no int64
    1 << 64,              # the first wide magnitude
    (1 << 64) + 1,
    R - ((1 << 64) - 1),  # narrow negative
    R - (1 << 64),        # wide negative
    (R - 1) // 2,         # the largest positive magnitude
    (R + 1) // 2,         # the largest negative magnitude
    R - 1,                # -1 written out
    R - (1 << 63),        # -2^63 written out: narrow
    (1 << 253) + 5,
    1 << 254,             # above r / 2, hence negative
)
I64_EDGE = (1, -1, 5, 1 << 62, (1 << 63) - 1, -(1 << 63))


def magnitude(v):
    """(|v|, negative) as the column sums take the canonical value v"""
    v %= R
    return (v, False) if v <= (R - 1) // 2 else (R - v, True)


def is_wide(v):
    return magnitude(v)[0] >= 1 << 64


def coef(rng):
    """One coefficient: an EDGE value, one of the int64 edge values (reduced mod r), or a random field element"""
    k = rng.next() % 3
    if k == 0:
        return EDGE[rng.next() % len(EDGE)]
    if k == 1:
        return I64_EDGE[rng.next() % len(I64_EDGE)] % R
    return rng.fr() or 1


def mimc_circuit(rounds, x0=3, seed=0x6D696D63, flip=None):
    """x -> (x + c_i)^3, `rounds` times.  Variables [const, x, out, intermediates..], nbIO = 3; round i is the gates
         (cur + c_i const) (cur + c_i const) = t          t (cur + c_i const) = next
    so there are 2 rounds gates and 2 rounds + 2 variables, and the `const` column holds `rounds` entries of L and 2 rounds of
    R.  c_i runs through EDGE first, then random field elements.  flip = (i, d) adds d to c_i in the MATRICES only: the
    witness is that of the unflipped circuit.  -> (SparseR1CS, witness mod r, the constants)"""
    rng = pr.SplitMix64(seed)
    cs = [EDGE[i] if i < len(EDGE) else (rng.fr() or 1) for i in range(rounds)]
    CONST, X, OUT = 0, 1, 2
    nvars = 3
    vals = {CONST: 1, X: x0 % R}
    left, right, out = [], [], []
    cur = X
    for i, c in enumerate(cs):
        cm = (c + flip[1]) % R if flip and flip[0] == i else c
        t = nvars
        nxt = OUT if i == rounds - 1 else nvars + 1
        nvars += 1 if i == rounds - 1 else 2
        s = (vals[cur] + c) % R
        vals[t] = s * s % R
        vals[nxt] = vals[t] * s % R
        left.append([(cur, 1), (CONST, cm)]); right.append([(cur, 1), (CONST, cm)]); out.append([(t, 1)])
        left.append([(t, 1)]); right.append([(cur, 1), (CONST, cm)]); out.append([(nxt, 1)])
        cur = nxt
    assert nvars == 2 * rounds + 2 and len(left) == 2 * rounds
    return rs.SparseR1CS(nvars, 3, left, right, out), [vals[i] for i in range(nvars)], cs


def csr_fr(rows):
    """rows[g] = [(col, value)] -> (row_ptr uint32, col uint32, val (nnz, 32) uint8 of v mod r): explicit zeros are kept"""
    row_ptr = np.zeros(len(rows) + 1, dtype=np.uint32)
    col, val = [], bytearray()
    for g, r in enumerate(rows):
        for c, v in r:
            col.append(c)
            val += (v % R).to_bytes(32, "big")
        row_ptr[g + 1] = len(col)
    return row_ptr, np.array(col, dtype=np.uint32), np.frombuffer(bytes(val), dtype=np.uint8).reshape(len(col), 32)


def rows_of(n, cols):
    """column view {variable: [(gate, coefficient)]} -> rows[g] = [(variable, coefficient)]"""
    rows = [[] for _ in range(n)]
    for c in sorted(cols):
        for g, v in cols[c]:
            rows[g].append((c, v))
    return rows


def count_wide(rows):
    return sum(1 for r in rows for _, v in r if is_wide(v))
