#!/usr/bin/env python3
"""Writes tests/golden/verify_batch_verdicts.json: oracle.pairing.groth16_verify's verdict on every proof that
tests/test_verify_batch_gpu.py meets -- the 300 valid proofs (made here by the oracle's prover from the same (r, s); the
device's proofs are byte-identical, and the test falls back to asking the oracle when a digest is not recorded) and every
tampered proof of every batch size -- keyed by the SHA-256 of A || B || C || io.  CPU only, a few minutes on eight cores:
    python tests/golden/gen_verify_batch_verdicts.py"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import verify_batch_cases as vc  # noqa: E402
from oracle import coracle as co  # noqa: E402
from oracle import pairing as pg  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402

_TRP = None


def _verdict(job):
    abc, io = job
    return vc.digest(abc, io), bool(pg.groth16_verify(_TRP, co.G1.from_b(abc[0]), co.G2.from_b(abc[1]), co.G1.from_b(abc[2]), io))


def main():
    global _TRP
    co.lib()
    c, sols, tr, draws, diff = vc.material(pr, rs)
    _TRP = rs.Bag(Alpha=co.G1.from_b(tr.Alpha), Beta2=co.G2.from_b(tr.Beta2), IoLP=co.G1.unpack(tr.IoLP), Gamma=co.G2.from_b(tr.Gamma),
                  Delta2=co.G2.from_b(tr.Delta2))
    proofs = []
    for w, r, s in draws:
        pf = rs.groth16_prove(tr, c, sols[w], r, s)
        proofs.append(((bytes(pf.A), bytes(pf.B), bytes(pf.C)), sols[w][:diff]))
    jobs = {vc.digest(*p): p for p in proofs}
    for n in vc.SIZES:
        for pos, what, value in vc.tampers(pr, co, n, diff):
            t = vc.apply_tamper(proofs[pos][0], proofs[pos][1], what, value)
            jobs[vc.digest(*t)] = t
    with multiprocessing.Pool(int(os.environ.get("JOBS", "6"))) as pool:
        verdicts = dict(pool.map(_verdict, list(jobs.values()), chunksize=4))
    assert sum(verdicts.values()) == len(proofs), "every untampered proof is valid, every tampered one is not"
    with open(vc.GOLDEN, "w") as f:
        json.dump({"what": "oracle.pairing.groth16_verify per proof of tests/test_verify_batch_gpu.py, by sha256(A||B||C||io)",
                   "verdicts": dict(sorted(verdicts.items()))}, f, indent=0)
    print(len(verdicts), "verdicts,", sum(verdicts.values()), "valid")


if __name__ == "__main__":
    main()
