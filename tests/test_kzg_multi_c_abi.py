"""Many polynomials, one proof per point, from plain C99 (tests/abi_smoke_kzg_multi.c): a caller combines p0 = (3, 1, 4, 1, 5) and
p1 = (2, 7) with the weights (1, 2), opens both at 7 over a string with tau = 11 with ONE proof, verifies it, sees a changed
value rejected and prints the bytes -- through nothing but include/playsnark_hip.h.  The bytes are compared here with the
oracle's scalar multiplication.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, P0, P1, WEIGHTS, Z = 11, [3, 1, 4, 1, 5], [2, 7], (1, 2), 7


def _build_smoke(tmp_path):
    """As tests/test_kzg_c_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg_multi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg_multi.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_combines_opens_and_verifies(tmp_path, co, pr):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_kzg_multi ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("y", "proof"))
    assert bytes.fromhex(got["y"]) == pr.fr_to_be32(pr.poly_eval(P0, Z)) + pr.fr_to_be32(pr.poly_eval(P1, Z))
    f = pr.poly_add([WEIGHTS[0] * a for a in P0], [WEIGHTS[1] * a for a in P1])
    assert f == [7, 15, 4, 1, 5]
    q, rem = pr.poly_div(f[::-1], [1, (-Z) % pr.R])
    assert rem == [pr.poly_eval(f, Z)]
    assert bytes.fromhex(got["proof"]) == co.G1.to_b(co.G1.mul(pr.poly_eval(q[::-1], TAU)))
