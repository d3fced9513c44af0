"""The material of tests/test_verify_batch_gpu.py that needs no GPU, shared with tests/golden/gen_verify_batch_verdicts.py:
one key of a 21-gate circuit, two witnesses, the (r, s) of 300 proofs, and the tampered elements of every case -- all drawn
from fixed seeds, so that the oracle's verdict on every proof a test meets can be recorded once
(tests/golden/verify_batch_verdicts.json: oracle.pairing.groth16_verify is pure Python, 3.4 s per proof)."""
import hashlib
import json
import os

SEED = 0x76626174
GATES = 21
NPROOFS = 300
SIZES = (1, 2, 7, 64, 300)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_batch_verdicts.json")


def material(pr, rs):
    """(circuit, [witness for x = 3, witness for x = 4], setup, [(witness index, r, s)] * NPROOFS, diff)"""
    rng = pr.SplitMix64(SEED)
    circuits = [rs.synthetic_circuit(GATES, x0) for x0 in (3, 4)]
    c = circuits[0][0]
    tr = rs.groth16_setup(c, *[rng.fr() for _ in range(5)])
    draws = [(i % 2, rng.fr(), rng.fr()) for i in range(NPROOFS)]
    return c, [s for _, s in circuits], tr, draws, c.nbVars - c.nbIO


def tampers(pr, co, n, diff):
    """The cases of one batch size: (position, what, value) with what in A, B, C (value: the bytes of a random subgroup
    point) or io (value: (index, field element)), at the first, the middle and the last proof."""
    rng = pr.SplitMix64(SEED + 1000 + n)
    out = []
    for pos in sorted({0, n // 2, n - 1}):
        for what in ("A", "B", "C", "io"):
            if what == "io":
                out.append((pos, what, (rng.next() % diff, rng.fr())))
            else:
                grp, og = (pr.G2, co.G2) if what == "B" else (pr.G1, co.G1)
                out.append((pos, what, og.to_b(grp.mul(rng.fr()))))
    return out


def apply_tamper(abc, io, what, value):
    """(A, B, C) bytes and the io list of one proof with one element replaced"""
    a, b, c = abc
    io = list(io)
    if what == "io":
        io[value[0]] = value[1]
    else:
        a, b, c = (value if what == "A" else a), (value if what == "B" else b), (value if what == "C" else c)
    return (a, b, c), io


def digest(abc, io):
    h = hashlib.sha256()
    for part in abc:
        h.update(bytes(part))
    for v in io:
        h.update(int(v).to_bytes(32, "big"))
    return h.hexdigest()


def recorded_verdicts():
    with open(GOLDEN) as f:
        return json.load(f)["verdicts"]
