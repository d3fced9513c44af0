"""The material of tests/test_phgr13_verify_batch_gpu.py that needs no GPU, shared with
tests/golden/gen_phgr13_verify_batch_verdicts.py: the toxic waste of the keys, the tamper kinds with the equations each one
breaks, the tampered values and the digest of a case -- all from fixed seeds, so that the oracle's verdict on the eleven
proofs of the N = 1 test can be recorded once (tests/golden/phgr13_verify_batch_verdicts.json: oracle.pairing.phgr13_verify
is pure Python, about 8 s per proof)."""
import hashlib
import json
import os

SEED = 0x7068767662
GATES = 7  # the circuit of the tamper tests: diff = 6
FIELDS = ("vss", "vass", "wss", "wass", "yss", "yass", "hs", "gz")
KINDS = FIELDS + ("io",)
# bit c of `failed`: E0 division, E1 v, E2 w, E3 y, E4 linear -- read off the five equations
MASK = {"vss": 0b10011, "vass": 0b00010, "wss": 0b10101, "wass": 0b00100, "yss": 0b11001, "yass": 0b01000, "hs": 0b00001,
        "gz": 0b10000, "io": 0b00001}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phgr13_verify_batch_verdicts.json")


def toxic(pr, n):
    """The eight secrets of the key of the n-gate circuit"""
    rng = pr.SplitMix64(SEED + 1000 * n)
    return [rng.fr() for _ in range(8)]


def x0s(k):
    """k distinct inputs of rs.synthetic_circuit, as tests/test_phgr13_prove_batch_gpu.py draws them"""
    return [3 + 2 * j for j in range(k)]


def tamper_value(pr, co, what, diff, salt=0):
    """The bytes of a random subgroup point for a proof element, (index, field element) for io"""
    rng = pr.SplitMix64(SEED + 77 * KINDS.index(what) + 7919 * salt + 5)
    if what == "io":
        return (rng.next() % diff, rng.fr())
    grp, og = (pr.G2, co.G2) if what == "wss" else (pr.G1, co.G1)
    return og.to_b(grp.mul(rng.fr()))


def apply_tamper(fields, io, what, value):
    """(dict of the eight elements' bytes, io list) of one proof with one element replaced"""
    fields, io = dict(fields), list(io)
    if what == "io":
        io[value[0]] = value[1]
    else:
        fields[what] = value
    return fields, io


def digest(fields, io):
    h = hashlib.sha256()
    for f in FIELDS:
        h.update(bytes(fields[f]))
    for v in io:
        h.update(int(v).to_bytes(32, "big"))
    return h.hexdigest()


def single_cases(pr, co, rs):
    """The eleven (name, fields, io) of the N = 1 test: the proof of x0 = 3, its nine tampers, the proof of x0 = 0.  Made by
    the oracle's prover; the device's proofs are the same bytes."""
    c, sol = rs.synthetic_circuit(GATES, 3)
    diff = c.nbVars - c.nbIO
    st = rs.phgr13_setup(c, *toxic(pr, GATES))
    pf = rs.phgr13_prove(st.EK, c, sol)
    fields = {f: bytes(getattr(pf, f)) for f in FIELDS}
    out = [("valid", fields, sol[:diff])]
    for what in KINDS:
        out.append((what,) + apply_tamper(fields, sol[:diff], what, tamper_value(pr, co, what, diff)))
    c0, sol0 = rs.synthetic_circuit(GATES, 0)
    assert (c0.left, c0.right, c0.out, c0.nbVars) == (c.left, c.right, c.out, c.nbVars)
    pf0 = rs.phgr13_prove(st.EK, c, sol0)
    out.append(("x0=0", {f: bytes(getattr(pf0, f)) for f in FIELDS}, sol0[:diff]))
    return st, diff, out


def recorded_verdicts():
    with open(GOLDEN) as f:
        return json.load(f)["verdicts"]
