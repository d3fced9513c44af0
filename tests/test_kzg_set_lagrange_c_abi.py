"""One proof for a set of points of a polynomial held as its values, from plain C99 (tests/abi_smoke_kzg_set_lagrange.c): a caller
takes the values v = (3, 1, 4, 1, 5) on the domain 1..5, opens the set {7, 2, 9} -- one of them a node -- over the Lagrange form
of a string with tau = 11, compares the bytes with the coefficient route within the same program, verifies, and prints them --
through nothing but include/playsnark_hip.h.  The bytes are compared here with the oracle's interpolation, division and scalar
multiplication.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, V, ZS = 11, [3, 1, 4, 1, 5], [7, 2, 9]


def _build_smoke(tmp_path):
    """As tests/test_kzg_lagrange_c_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg_set_lagrange")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg_set_lagrange.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_opens_the_set_and_verifies(tmp_path, co, pr):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_kzg_set_lagrange ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("commit", "y", "proof", "qv", "rem"))
    p = (pr.interpolate(V) + [0] * len(V))[: len(V)]
    g1 = lambda k: co.G1.to_b(co.G1.mul(k))
    zs_poly = [1]
    for z in ZS:
        zs_poly = pr.poly_mul(zs_poly, [(-z) % pr.R, 1])
    q, rem = pr.poly_div(p[::-1], zs_poly[::-1])
    q, rem = q[::-1], rem[::-1]
    assert bytes.fromhex(got["commit"]) == g1(pr.poly_eval(p, TAU))
    assert bytes.fromhex(got["y"]) == b"".join(pr.fr_to_be32(pr.poly_eval(p, z)) for z in ZS)
    assert pr.poly_eval(p, ZS[1]) == V[ZS[1] - 1]
    assert bytes.fromhex(got["proof"]) == g1(pr.poly_eval(q, TAU))
    assert bytes.fromhex(got["qv"]) == b"".join(pr.fr_to_be32(pr.poly_eval(q, i)) for i in range(1, len(V) + 1))
    assert bytes.fromhex(got["rem"]) == b"".join(pr.fr_to_be32(c) for c in rem)
