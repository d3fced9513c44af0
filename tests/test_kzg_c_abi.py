"""KZG from plain C99 (tests/abi_smoke_kzg.c): a caller commits to p = (3, 1, 4, 1, 5) over a string with tau = 11, opens it at
7 and 2, verifies one by one and as a batch, and prints the bytes -- through nothing but include/playsnark_hip.h.  The bytes are
compared here with the oracle's scalar multiplications.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, COEF, ZS = 11, [3, 1, 4, 1, 5], [7, 2]


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_c_caller_compiles_links_and_fails_loudly_without_a_gpu(tmp_path):
    from playsnark_amd import api

    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if api.device_count() == 0:
        assert res.returncode == 77, res.stdout + res.stderr
    else:
        assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.gpu
def test_c_caller_commits_opens_and_verifies(tmp_path, co, pr):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_kzg ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("commit", "y", "proofs"))
    assert bytes.fromhex(got["commit"]) == co.G1.to_b(co.G1.mul(pr.poly_eval(COEF, TAU)))
    ys = [pr.poly_eval(COEF, z) for z in ZS]
    assert bytes.fromhex(got["y"]) == b"".join(pr.fr_to_be32(y) for y in ys)
    want = b""
    for z in ZS:
        q, rem = pr.poly_div(COEF[::-1], [1, (-z) % pr.R])
        assert rem == [pr.poly_eval(COEF, z)]
        want += co.G1.to_b(co.G1.mul(pr.poly_eval(q[::-1], TAU)))
    assert bytes.fromhex(got["proofs"]) == want
