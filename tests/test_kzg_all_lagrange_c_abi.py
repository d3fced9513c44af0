"""The proofs of every node of the domain from plain C99 (tests/abi_smoke_kzg_all_lagrange.c): a caller takes the values
v = (3, 1, 4, 1, 5) on the domain 1..5, computes the key table and all five proofs over the Lagrange form of a string with
tau = 11, compares them with the single-point openings within the same program, verifies each, and prints them -- through
nothing but include/playsnark_hip.h.  The bytes are compared here with the oracle's interpolation, division and scalar
multiplication.  Without a device the program exits 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, V = 11, [3, 1, 4, 1, 5]


def _build_smoke(tmp_path):
    """As tests/test_kzg_set_lagrange_c_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_kzg_all_lagrange")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_kzg_all_lagrange.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_opens_every_node_and_verifies(tmp_path, co, pr):
    from oracle import restate as rs

    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_kzg_all_lagrange ok" in res.stdout
    got = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ")[0] in ("commit", "key", "proofs"))
    n = len(V)
    p = (pr.interpolate(V) + [0] * n)[:n]
    g1 = lambda k: co.G1.to_b(co.G1.mul(k))
    assert bytes.fromhex(got["commit"]) == g1(pr.poly_eval(p, TAU))
    want = b""
    for m in range(1, n + 1):
        q, rem = pr.poly_div(p[::-1], [1, (-m) % pr.R])
        assert rem == [V[m - 1]]
        want += g1(pr.poly_eval(q[::-1], TAU))
    assert bytes.fromhex(got["proofs"]) == want
    lag = rs.lagrange_at(n, TAU)[0]
    key = b"".join(g1(sum(pr.fr_div(lag[i - 1], (m - i) % pr.R) for i in range(1, n + 1) if i != m) % pr.R) for m in range(1, n + 1))
    assert bytes.fromhex(got["key"]) == key
