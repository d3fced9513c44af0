"""Inputs shared by the GPU tests of the whole-bucket point pass (test_bucket_sum_gpu.py, test_bucket_sum_entries_gpu.py):
the exceptional input kinds at n points, over one set of 4 097 base points per group that is made once."""
import numpy as np

SEED = 0x626F7264
SIZES = (1, 2, 63, 64, 65, 300, 4097)
SLICES, BUCKETS = 1, 2
KINDS = ("uniform", "zero", "equal", "repeated", "p_and_minus_p", "identities")


def _grp(ps_api, co, name):
    return (ps_api.G1, co.G1) if name == "g1" else (ps_api.G2, co.G2)


def _uniform_be32(n, seed):
    raw = np.random.RandomState(seed).randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F  # < 2^254 < r
    return raw.tobytes()


def _neg(pr, name, P):
    return (P[0], (pr.P - P[1]) % pr.P) if name == "g1" else (P[0], ((-P[1][0]) % pr.P, (-P[1][1]) % pr.P))


_base = {}


def _base_points(og, name):
    """4 097 distinct points, made once per group."""
    if name not in _base:
        _base[name] = og.gen_points(SEED + 11, SEED + 13, max(SIZES))
    return _base[name]


def _case(og, pr, name, kind, n):
    """(scalar bytes, point bytes) of one input kind at n points."""
    nb = og.nb
    raw = _base_points(og, name)[: n * nb]
    sc = _uniform_be32(n, SEED + n)
    if kind == "zero":
        sc = bytes(32 * n)
    elif kind == "equal":
        sc = sc[:32] * n
    elif kind == "repeated":  # one point, and few enough distinct scalars that buckets hold it several times
        raw = raw[:nb] * n
        sc = b"".join(sc[32 * (i % 3) : 32 * (i % 3) + 32] for i in range(n))
    elif kind == "p_and_minus_p":  # equal scalars, P and -P in turn: every window's bucket cancels (n even) or leaves P
        P = og.from_b(raw[:nb])
        pair = raw[:nb] + og.to_b(_neg(pr, name, P))
        raw = (pair * ((n + 1) // 2))[: n * nb]
        sc = sc[:32] * n
    elif kind == "identities":  # every third point is the identity; with equal-ish scalars some buckets start with one
        ident = og.to_b(None)
        raw = b"".join(ident if i % 3 == 0 else raw[i * nb : (i + 1) * nb] for i in range(n))
        sc = b"".join(sc[32 * (i % 5) : 32 * (i % 5) + 32] for i in range(n))
    else:
        assert kind == "uniform"
    return sc, raw
