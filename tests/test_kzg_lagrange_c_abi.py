"""A polynomial held as its values, committed and opened from plain C99 (tests/abi_smoke_kzg_lagrange.c): a caller takes the
values v = (3, 1, 4, 1, 5, 9) on the domain 1..6, commits to them over the Lagrange form of a string with tau = 11, opens at the
node 2 and at 7, verifies, and prints the bytes -- through nothing but include/playsnark_hip.h.  The bytes are compared here with
the oracle's interpolation, division and scalar multiplication.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, V, ZS = 11, [3, 1, 4, 1, 5, 9], [2, 7]


def _build_smoke(tmp_path):
    """As tests/test_kzg_set_c_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg_lagrange")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg_lagrange.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
    assert "abi_smoke_kzg_lagrange ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("commit", "y", "proofs", "qv"))
    p = (pr.interpolate(V) + [0] * len(V))[: len(V)]
    g1 = lambda k: co.G1.to_b(co.G1.mul(k))
    assert bytes.fromhex(got["commit"]) == g1(pr.poly_eval(p, TAU))
    assert bytes.fromhex(got["y"]) == b"".join(pr.fr_to_be32(pr.poly_eval(p, z)) for z in ZS)
    assert pr.poly_eval(p, ZS[0]) == V[ZS[0] - 1]
    proofs, rows = b"", b""
    for z in ZS:
        q, _ = pr.poly_div(p[::-1], [1, (-z) % pr.R])
        q = q[::-1]
        proofs += g1(pr.poly_eval(q, TAU))
        rows += b"".join(pr.fr_to_be32(pr.poly_eval(q, i)) for i in range(1, len(V) + 1))
    assert bytes.fromhex(got["proofs"]) == proofs
    assert bytes.fromhex(got["qv"]) == rows
