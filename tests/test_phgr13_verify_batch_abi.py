"""The two entries of the PHGR13 batch verifier (ps_phgr13_verify_batch, ps_phgr13_verify_batch_info), added within ABI
revision 5: declared in the header with the argument lists the binding uses, listed in _lib.py, exported by the built
library, mirrored in host/playsnark.hpp, the Go shim and INTEGRATION.md; they refuse NULL arguments without touching a
device.  tests/abi_smoke_phgr13_verify_batch.c calls them from plain C99 and tests/abi_smoke_phgr13_verify_batch_cpp.cpp
through host/playsnark.hpp: both build and, without a device, exit 77; on the GPU each verifies a two-proof batch."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_phgr13_verify_batch": 7, "ps_phgr13_verify_batch_info": 2}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", _read("include", "playsnark_hip.h"), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ps_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_entries_are_declared_with_the_documented_arguments():
    from playsnark_amd import _lib

    protos = _prototypes()
    for name, nargs in ARGS.items():
        assert name in protos, name
        assert len([a for a in protos[name].split(",") if a.strip()]) == nargs, protos[name]
        assert name in _lib.SYMBOLS
        assert len(getattr(_lib.lib, name).argtypes) == nargs
    header = _read("include", "playsnark_hip.h")
    assert "#define PS_ABI_VERSION 5" in header and "then ps_phgr13_verify_batch and ps_phgr13_verify_batch_info" in header
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    # the struct the header declares: failed, device_loops, reserved[2], 32 bits each
    m = re.search(r"typedef struct \{([^}]*)\} ps_phgr13_batch_info;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and re.findall(r"uint32_t\s+(\w+)", m.group(1)) == ["failed", "device_loops", "reserved"]
    assert [f[0] for f in _lib.Phgr13BatchInfo._fields_] == ["failed", "device_loops", "reserved"]
    assert C.sizeof(_lib.Phgr13BatchInfo) == 16 and C.sizeof(_lib.Phgr13Proof) == 864


def test_the_stage_hook_is_exported_but_not_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ps_debug_phgr13_verify_batch_stage_ms\b", out)
    assert "ps_debug_phgr13_verify_batch_stage_ms" not in _read("include", "playsnark_hip.h")


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    ok = C.c_int(7)
    vk = _lib.Phgr13Vk()  # its three arrays are NULL
    one = (_lib.Phgr13Proof * 1)()
    assert lib.ps_phgr13_verify_batch(None, C.byref(vk), None, one, 1, bytes(32), C.byref(ok)) == _lib.PS_ERR_ARG
    assert b"ps_phgr13_verify_batch" in lib.ps_last_error()
    assert lib.ps_phgr13_verify_batch(None, None, None, None, 0, None, None) == _lib.PS_ERR_ARG
    assert lib.ps_phgr13_verify_batch_info(None, None) == _lib.PS_ERR_ARG
    info = _lib.Phgr13BatchInfo()
    assert lib.ps_phgr13_verify_batch_info(None, C.byref(info)) == _lib.PS_ERR_ARG
    assert b"ps_phgr13_verify_batch_info" in lib.ps_last_error()


def test_mirrors_name_the_entries():
    from playsnark_amd import api

    hpp, go, integ = _read("playsnark_amd", "host", "playsnark.hpp"), _read("shim", "playsnark_hip.go"), _read("INTEGRATION.md")
    for name in ARGS:
        assert name in hpp, name
        assert name in integ, name
        assert "C." + name + "(" in go, name
    assert "PHGR13VerifyBatch(" in hpp
    assert "func PHGR13VerifyBatchHIP(" in go and "PHGR13VerifyBatchHIP" in integ
    assert callable(api.PHGR13VerifyBatch) and callable(api.PHGR13VerifyBatchInfo)


def _build(tmp_path, lang):
    """As tests/test_abi.py builds its callers: -pedantic C99 against the header and the shared library alone; C++17 against
    host/playsnark.hpp."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    link = ["-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
    if lang == "c":
        exe = str(tmp_path / "abi_smoke_phgr13_verify_batch")
        cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "tests", "abi_smoke_phgr13_verify_batch.c"), "-o", exe] + link
    else:
        exe = str(tmp_path / "abi_smoke_phgr13_verify_batch_cpp")
        cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, os.path.join(ROOT, "tests", "abi_smoke_phgr13_verify_batch_cpp.cpp"),
               "-o", exe] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_callers_compile_link_and_fail_loudly_without_a_gpu(tmp_path, lang):
    from playsnark_amd import api

    exe = _build(tmp_path, lang)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if api.device_count() == 0:
        assert res.returncode == 77, res.stdout + res.stderr
    else:
        assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("lang", ["c", "cpp"])
def test_callers_verify_a_two_proof_batch(tmp_path, lang):
    exe = _build(tmp_path, lang)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_phgr13_verify_batch%s ok" % ("_cpp" if lang == "cpp" else "") in res.stdout
