#!/usr/bin/env python3
"""Writes tests/golden/phgr13_verify_batch_verdicts.json: oracle.pairing.phgr13_verify's verdict on the eleven proofs of the
N = 1 test of tests/test_phgr13_verify_batch_gpu.py -- the valid proof, its nine tampers and the proof of the x0 = 0
witness (tests/phgr13_verify_batch_cases.py, same seeds) -- keyed by the SHA-256 of the eight elements and io.  CPU only,
about 8 s per case:
    python tests/golden/gen_phgr13_verify_batch_verdicts.py"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import phgr13_verify_batch_cases as pc  # noqa: E402
from oracle import coracle as co  # noqa: E402
from oracle import pairing as pg  # noqa: E402
from oracle import pyref as pr  # noqa: E402
from oracle import restate as rs  # noqa: E402

_VK = None
_DIFF = 0


def _verdict(job):
    name, fields, io = job
    proof = rs.Bag(**{f: (co.G2 if f == "wss" else co.G1).from_b(fields[f]) for f in pc.FIELDS})
    return name, pc.digest(fields, io), bool(pg.phgr13_verify(_VK, _DIFF, proof, io))


def main():
    global _VK, _DIFF
    co.lib()
    st, _DIFF, cases = pc.single_cases(pr, co, rs)
    _VK = st.VK
    with multiprocessing.Pool(int(os.environ.get("JOBS", "6"))) as pool:
        res = pool.map(_verdict, cases)
    for name, _, v in res:
        assert v is (name in ("valid", "x0=0")), (name, v)
    with open(pc.GOLDEN, "w") as f:
        json.dump({"what": "oracle.pairing.phgr13_verify per case of the N = 1 test of tests/test_phgr13_verify_batch_gpu.py, "
                           "by sha256(vss||vass||wss||wass||yss||yass||hs||gz||io)",
                   "verdicts": dict(sorted((d, v) for _, d, v in res))}, f, indent=0)
    print(len(res), "verdicts,", sum(v for _, _, v in res), "valid")


if __name__ == "__main__":
    main()
