"""The two entries of the PHGR13 batch prover (ps_msm_batch_multi, ps_phgr13_prove_batch), added within ABI revision 5:
declared in the header with the argument lists the binding uses, listed in _lib.py, exported by the built library, mirrored in
host/playsnark.hpp (which still compiles), the Go shim and INTEGRATION.md; they refuse NULL arguments without touching a
device.  tests/abi_smoke_phgr13_batch.c calls them from plain C99: it builds and, without a device, exits 77; on the GPU it
proves (7 gates, 3 witnesses) in one call and compares with three single calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_msm_batch_multi": 8, "ps_phgr13_prove_batch": 7}


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
    assert "#define PS_ABI_VERSION 5" in header and "then ps_msm_batch_multi and ps_phgr13_prove_batch" in header
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    assert C.sizeof(_lib.Phgr13Proof) == 864


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    assert lib.ps_msm_batch_multi(None, None, 1, None, 1, 1, 0, None) == _lib.PS_ERR_ARG
    assert b"ps_msm_batch_multi" in lib.ps_last_error()
    ek = _lib.Phgr13Ek()
    out = (_lib.Phgr13Proof * 1)()
    flags = (C.c_int * 1)()
    assert lib.ps_phgr13_prove_batch(None, C.byref(ek), None, None, 1, out, flags) == _lib.PS_ERR_ARG
    assert b"ps_phgr13_prove_batch" in lib.ps_last_error()


def test_mirrors_name_the_entries():
    hpp, go, integ = _read("playsnark_amd", "host", "playsnark.hpp"), _read("shim", "playsnark_hip.go"), _read("INTEGRATION.md")
    for name in ARGS:
        assert name in hpp, name
        assert name in integ, name
    assert "PHGR13ProveBatch(" in hpp and "SolCommitsBatch(" in hpp
    assert "func PHGR13ProveHIPBatch(" in go and "C.ps_phgr13_prove_batch(" in go
    assert "PHGR13ProveHIPBatch" in integ


def test_cpp_mirror_compiles_with_the_phgr13_batch_prover(tmp_path):
    src = tmp_path / "use_phgr13_batch.cpp"
    src.write_text(
        '#include "playsnark_amd/host/playsnark.hpp"\n'
        "using namespace playsnark;\n"
        "std::vector<ps_phgr13_proof> prove(Context& c, const ps_phgr13_ek& ek, const QAP& q, const Poly& sols, size_t k,\n"
        "                                   std::vector<int>* valid) {\n"
        "    SetBatchChunk(c, 0);\n"
        "    return PHGR13ProveBatch(c, ek, q, sols, k, valid);\n"
        "}\n"
        "std::vector<std::vector<Bytes>> sums(Context& c, const std::vector<const Points*>& a, const Poly& s, size_t k, size_t m, size_t d) {\n"
        "    return SolCommitsBatch(c, a, s, k, m, d);\n"
        "}\n"
    )
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "use_phgr13_batch.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_phgr13_batch")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_phgr13_batch.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_proves_a_batch_and_three_single_proofs(tmp_path):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_phgr13_batch ok" in res.stdout
