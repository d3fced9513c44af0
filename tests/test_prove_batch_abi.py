"""The three entries of the batch prover (ps_msm_batch, ps_msm_batch_set_chunk, ps_groth16_prove_batch), added within ABI
revision 5: declared in the header with the argument lists the binding uses, listed in _lib.py, exported by the built
library, mirrored in host/playsnark.hpp (which still compiles), the Go shim and INTEGRATION.md; they refuse NULL arguments
without touching a device.  tests/abi_smoke_prove_batch.c calls them from plain C99: it builds and, without a device, exits
77; on the GPU it proves (7 gates, 3 witnesses) in one call and compares with three single calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_msm_batch": 5, "ps_msm_batch_set_chunk": 2, "ps_groth16_prove_batch": 11}


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
    assert "#define PS_ABI_VERSION 5" in _read("include", "playsnark_hip.h")
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    assert lib.ps_msm_batch(None, None, None, 1, None) == _lib.PS_ERR_ARG
    assert b"ps_msm_batch" in lib.ps_last_error()
    assert lib.ps_msm_batch_set_chunk(None, 0) == _lib.PS_ERR_ARG
    pk = _lib.Groth16Pk()
    flags = (C.c_int * 1)()
    assert lib.ps_groth16_prove_batch(None, C.byref(pk), None, None, 1, b"\0" * 32, b"\0" * 32, None, None, None, flags) == _lib.PS_ERR_ARG
    assert b"ps_groth16_prove_batch" in lib.ps_last_error()


def test_mirrors_name_the_entries():
    hpp, go, integ = _read("playsnark_amd", "host", "playsnark.hpp"), _read("shim", "playsnark_hip.go"), _read("INTEGRATION.md")
    for name in ARGS:
        assert name in hpp, name
        assert name in integ, name
    assert "Groth16ProveBatch(" in hpp and "BlindEvalBatch(" in hpp
    assert "func Groth16ProveBatchHIP(" in go and "C.ps_groth16_prove_batch(" in go and "C.ps_msm_batch(" in go
    assert "Groth16ProveBatchHIP" in integ


def test_cpp_mirror_compiles_with_the_batch_prover(tmp_path):
    src = tmp_path / "use_batch.cpp"
    src.write_text(
        '#include "playsnark_amd/host/playsnark.hpp"\n'
        "using namespace playsnark;\n"
        "std::vector<Groth16Proof> prove(Context& c, const ps_groth16_pk& pk, const QAP& q, const Poly& sols, const std::vector<Scalar>& r,\n"
        "                                const std::vector<Scalar>& s, std::vector<int>* valid) {\n"
        "    SetBatchChunk(c, 0);\n"
        "    return Groth16ProveBatch(c, pk, q, sols, r, s, valid);\n"
        "}\n"
        "std::vector<Bytes> sums(Context& c, const Points& p, const Poly& k, size_t n) { return BlindEvalBatch(c, p, k, n); }\n"
    )
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "use_batch.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_prove_batch")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_prove_batch.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
    assert "abi_smoke_prove_batch ok" in res.stdout
