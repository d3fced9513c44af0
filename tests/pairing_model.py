"""Plain-integer model of the device pairing tower (playsnark_amd/csrc/pairing_body.inc over Fp / Fp2, pairing_dev.hpp),
for the tests only.  No limb emulation: a device value is read as residues, and every reference below is written from the
definition of the operation.

The device tower: Fp2 = Fp[u] / (u^2 + 1), Fp6 = Fp2[v] / (v^3 - xi) with xi = 1 + u, Fp12 = Fp6[w] / (w^2 - v).  In memory an
Fp12 is c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (each an Fp2 of two Fp of 14 limbs); c_i.c_j is the coefficient of
w^(2j + i).  Here an element is the list of its six Fp2 coefficients of 1, w, .., w^5 (w^6 = xi), an Fp2 a pair (a, b) = a + b u.
oracle/pairing.py works in Fp[w] / (w^12 - 2 w^6 + 2): there u = w^6 - 1, so a + b u at w^k is a - b at w^k and b at w^(k+6).
"""
from __future__ import annotations

import numpy as np

import field_model as fm

P = fm.P
W1, W2, W6, W12 = fm.FP_L, 2 * fm.FP_L, 6 * fm.FP_L, 12 * fm.FP_L
MONT_INV = pow(fm.FP_RM, -1, P)
# struct order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> power of w
W_POWER = [2 * j + i for i in range(2) for j in range(3)]
XI = (1, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# limbs -> residues
# ---------------------------------------------------------------------------------------------------------------------------
def fp_residues(rows):
    """rows: (cases, 14 k) limbs -> per case the k field elements the limbs stand for (Montgomery factor 2^392 removed)"""
    rows = np.asarray(rows, dtype=np.int64)
    k = rows.shape[1] // W1
    w = np.array([1 << (fm.B * i) for i in range(W1)], dtype=object)
    vals = (rows.reshape(len(rows), k, W1).astype(object) * w).sum(axis=2)
    return [[int(v) * MONT_INV % P for v in row] for row in vals]


def fp_values(rows):
    """The integer every group of 14 limbs holds (no reduction): for range checks"""
    rows = np.asarray(rows, dtype=np.int64)
    k = rows.shape[1] // W1
    w = np.array([1 << (fm.B * i) for i in range(W1)], dtype=object)
    return [[int(v) for v in row] for row in (rows.reshape(len(rows), k, W1).astype(object) * w).sum(axis=2)]


def f2s(res):
    """2 k residues -> k Fp2 pairs, memory order"""
    return [(res[2 * i], res[2 * i + 1]) for i in range(len(res) // 2)]


def f12_from_struct(c):
    """six Fp2 in struct order -> coefficients of 1, w, .., w^5"""
    out = [None] * 6
    for s, k in enumerate(W_POWER):
        out[k] = c[s]
    return out


def f12_to_struct(a):
    return [a[k] for k in W_POWER]


# ---------------------------------------------------------------------------------------------------------------------------
# the tower, from the definitions
# ---------------------------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def poly_mul_mod(a, b, n):
    """a b in Fp2[t] / (t^n - xi): coefficient lists of length n"""
    acc = [(0, 0)] * (2 * n - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            acc[i + j] = f2_add(acc[i + j], f2_mul(x, y))
    return [f2_add(acc[d], f2_mul(XI, acc[d + n])) if d + n < 2 * n - 1 else acc[d] for d in range(n)]


def f6_mul(a, b):  # Fp2[v] / (v^3 - xi), coefficients of 1, v, v^2
    return poly_mul_mod(a, b, 3)


def f12_mul(a, b):  # Fp2[w] / (w^6 - xi)
    return poly_mul_mod(a, b, 6)


def f12_sqr(a):
    return f12_mul(a, a)


def f12_line(a, b, c):
    """a + b w^2 + c w^3, the shape of a line value"""
    z = (0, 0)
    return [a, z, b, c, z, z]


F12_ONE = [(1, 0)] + [(0, 0)] * 5


# ---------------------------------------------------------------------------------------------------------------------------
# into the oracle's Fp12
# ---------------------------------------------------------------------------------------------------------------------------
def to_oracle(a):
    """The basis map: six Fp2 coefficients of w^k -> twelve Fp coefficients over w^12 - 2 w^6 + 2"""
    out = [0] * 12
    for k, (x, y) in enumerate(a):
        out[k] = (out[k] + x - y) % P
        out[k + 6] = (out[k + 6] + y) % P
    return out


def struct_residues_to_oracle(res12):
    """twelve residues in memory order -> the oracle's element"""
    return to_oracle(f12_from_struct(f2s(res12)))


# ---------------------------------------------------------------------------------------------------------------------------
# operand builders: tests/host_pairing_batch_check.cpp's worst12 for 2, 6 and 12 coefficients
# ---------------------------------------------------------------------------------------------------------------------------
def worst_coeffs(ncoef, cls, seed, rng):
    """ncoef Fp in memory order, every limb at the edge of class cls, coefficient k under sign pattern (seed + k) & 3"""
    return sum((fm.worst(cls, (seed + k) & 3, rng) for k in range(ncoef)), [])


def random_coeffs(ncoef, cls, n, rng):
    return np.concatenate([fm.random_lazy(cls, n, rng) for _ in range(ncoef)], axis=1)


def canon_coeffs(ncoef, n, rng):
    """random canonical Montgomery-form coefficients (class 1)"""
    return np.concatenate([fm.random_canon(n, rng) for _ in range(ncoef)], axis=1)


def coeff_class(rows):
    """per case, the largest limb class over all its coefficients"""
    return fm.limb_class(np.asarray(rows, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# launches: spread_index / spread_lanes of pairing_dev.hpp restated
# ---------------------------------------------------------------------------------------------------------------------------
def spread_lanes(n, simds):
    return min(64, max(1, -(-n // max(simds, 1))))


def wave_fill(n, lpw):
    """(waves, elements of the last wave) of a launch of n elements with lpw active lanes per wave"""
    waves = -(-n // lpw)
    return waves, n - (waves - 1) * lpw
