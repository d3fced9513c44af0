"""A circuit with field-valued coefficients from plain C99 (tests/abi_smoke_qap_fr.c) and through the C++ host mirror
(tests/abi_smoke_qap_fr_cpp.cpp): three MiMC-style rounds whose constants are 32-byte values (two of them wide),
ps_qap_create_fr, the key from a powers-of-tau string against the key from the values in the clear, one proof verified --
through nothing but include/playsnark_hip.h, respectively playsnark_amd/host/playsnark.hpp.  Without a device the programs
exit 77."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_smoke(tmp_path, lang):
    """As tests/test_abi.py builds its callers: -pedantic C99 against the header and the shared library alone; C++17 over the
    host mirror."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    link = ["-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
    if lang == "c":
        exe = str(tmp_path / "abi_smoke_qap_fr")
        cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tests", "abi_smoke_qap_fr.c"), "-o", exe] + link
    else:
        exe = str(tmp_path / "abi_smoke_qap_fr_cpp")
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, os.path.join(ROOT, "tests", "abi_smoke_qap_fr_cpp.cpp"), "-o", exe] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_callers_compile_link_and_fail_loudly_without_a_gpu(tmp_path, lang):
    from playsnark_amd import api

    exe = _build_smoke(tmp_path, lang)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if api.device_count() == 0:
        assert res.returncode == 77, res.stdout + res.stderr
    else:
        assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("lang,ok", [("c", "abi_smoke_qap_fr ok"), ("cpp", "abi_smoke_qap_fr_cpp ok")])
def test_callers_build_a_field_valued_circuit_and_use_it(tmp_path, lang, ok):
    exe = _build_smoke(tmp_path, lang)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ok in res.stdout
