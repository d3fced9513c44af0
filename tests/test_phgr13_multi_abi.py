"""The multi-device PHGR13 entries from plain C99 (tests/abi_smoke_phgr13_multi.c): the toy proof of
tests/golden/phgr13_toy.json through ps_phgr13_prove_multi (two contexts, rank-local keys) and through two
ps_phgr13_prove_shard parts folded, plus one PS_ERR_LENGTH refusal.  Without a device the program exits 77."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_file(tmp_path):
    """tests/golden/phgr13_toy.json (evaluation key and proof) as `name hex` lines for the C program."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "phgr13_toy.json")))
    lines = [f"{k} {v}" for k, v in g["ek"].items()] + [f"{k} {v}" for k, v in g["proof"].items()]
    path = tmp_path / "phgr13_toy.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    link = ["-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
    exe = str(tmp_path / "abi_smoke_phgr13_multi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_phgr13_multi.c"), "-o", exe] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_library_declares_the_multi_device_phgr13_entries():
    from playsnark_amd import _lib

    assert _lib.lib.ps_abi_version() == _lib.PS_ABI_VERSION == 5
    for name in ("ps_phgr13_prove_shard", "ps_phgr13_prove_multi"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    import ctypes

    assert ctypes.sizeof(_lib.Phgr13Device) == 3 * ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(_lib.Phgr13Ek)


def test_refusals_before_any_device_work():
    """Argument errors are found on the host: no device is needed to see them."""
    from playsnark_amd import _lib, api

    lib = _lib.lib
    out = _lib.Phgr13Proof()
    assert lib.ps_phgr13_prove_multi(None, 1, out) == _lib.PS_ERR_ARG
    assert lib.ps_phgr13_prove_multi((_lib.Phgr13Device * 1)(), 0, out) == _lib.PS_ERR_ARG
    assert lib.ps_phgr13_prove_multi((_lib.Phgr13Device * 65)(), 65, out) == _lib.PS_ERR_ARG
    assert lib.ps_phgr13_prove_multi((_lib.Phgr13Device * 2)(), 2, out) == _lib.PS_ERR_ARG  # NULL handles
    assert "NULL handle" in lib.ps_last_error().decode()
    assert lib.ps_phgr13_prove_shard(None, None, None, None, 0, 1, out) == _lib.PS_ERR_ARG
    with pytest.raises(api.PlaysnarkError):
        api.PHGR13ProveMulti([])


def test_c_caller_compiles_links_and_fails_loudly_without_a_gpu(tmp_path):
    from playsnark_amd import api

    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe, _fixture_file(tmp_path)], capture_output=True, text=True, timeout=300)
    if api.device_count() == 0:
        assert res.returncode == 77, res.stdout + res.stderr
    else:
        assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.gpu
def test_c_caller_proves_the_toy_circuit_over_two_contexts(tmp_path):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe, _fixture_file(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok" in res.stdout
