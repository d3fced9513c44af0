"""One polynomial, a set of points, one proof, from plain C99 (tests/abi_smoke_kzg_set.c): a caller divides p = (3, 1, 4, 1, 5, 9)
by (X - 2)(X - 7), opens it at {2, 7} over a string with tau = 11 with ONE proof, verifies it, sees a changed value and swapped
values rejected and prints the bytes -- through nothing but include/playsnark_hip.h.  The bytes are compared here with the
oracle's division and scalar multiplication.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, P, ZS = 11, [3, 1, 4, 1, 5, 9], [2, 7]


def _build_smoke(tmp_path):
    """As tests/test_kzg_multi_c_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg_set")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg_set.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_divides_opens_and_verifies(tmp_path, co, pr):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_kzg_set ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("q", "y", "rem", "proof"))
    zs_poly = pr.poly_mul([(-ZS[0]) % pr.R, 1], [(-ZS[1]) % pr.R, 1])
    q, rem = pr.poly_div(P[::-1], zs_poly[::-1])
    q, rem = q[::-1], rem[::-1]
    assert len(q) == 4 and len(rem) == 2
    assert bytes.fromhex(got["q"]) == b"".join(pr.fr_to_be32(v) for v in q)
    assert bytes.fromhex(got["y"]) == b"".join(pr.fr_to_be32(pr.poly_eval(P, z)) for z in ZS)
    assert bytes.fromhex(got["rem"]) == b"".join(pr.fr_to_be32(v) for v in rem)
    assert [pr.poly_eval(rem, z) for z in ZS] == [pr.poly_eval(P, z) for z in ZS]
    assert bytes.fromhex(got["proof"]) == co.G1.to_b(co.G1.mul(pr.poly_eval(q, TAU)))
