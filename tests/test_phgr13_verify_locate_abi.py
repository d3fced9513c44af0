"""The two entries of the locating PHGR13 batch verifier (ps_phgr13_verify_batch_locate, ps_phgr13_verify_batch_locate_info),
added within ABI revision 5: declared in the header with the argument lists the binding uses, listed in _lib.py, exported by
the built library, mirrored in api.py, host/playsnark.hpp, the Go shim and INTEGRATION.md; they refuse NULL arguments without
touching a device; the header states the soundness, the cost bounds and the memory of the call, and the plain call's comment
points to it.  tests/abi_smoke_phgr13_verify_locate.c calls them from plain C99: it builds and, without a device, exits 77;
on the GPU it locates the one bad proof of seven."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_phgr13_verify_batch_locate": 9, "ps_phgr13_verify_batch_locate_info": 2}
FIELDS = ["checks", "products", "levels", "invalid", "failed", "reserved"]


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
    assert "#define PS_ABI_VERSION 5" in header and "then ps_phgr13_verify_batch_locate and ps_phgr13_verify_batch_locate_info" in header
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    m = re.search(r"typedef struct \{([^}]*)\} ps_phgr13_locate_info;", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert m and re.findall(r"uint32_t\s+(\w+)", m.group(1)) == FIELDS
    assert [f[0] for f in _lib.Phgr13LocateInfo._fields_] == FIELDS and C.sizeof(_lib.Phgr13LocateInfo) == 32
    # no existing struct changed
    assert C.sizeof(_lib.Phgr13BatchInfo) == 16 and C.sizeof(_lib.VerifyLocateInfo) == 16 and C.sizeof(_lib.Phgr13Proof) == 864


def test_header_states_soundness_cost_and_memory():
    header = _read("include", "playsnark_hip.h")
    doc = header[header.index("WHICH proofs of a PHGR13 batch are invalid"):header.index("} ps_phgr13_locate_info;")]
    flat = " ".join(doc.replace("*", " ").split())
    assert "a set bit of failed[i] is always exact" in flat
    assert "nproofs / 2^bits(rho) per passed product" in flat
    assert "checks <= 1 + 2 b ceil(log2 N)" in flat and "products <= 5 + 2 ceil(log2 N) sum_i popcount(failed[i])" in flat
    assert "PS_ERR_HIP" in flat and "bytes asked for" in flat
    for figure in ("1 344 B per proof", "448 B per proof", "896 B per proof", "64 B per proof"):  # 2 sizeof(Fp12), XYZZ G1, XYZZ G2, 2 x 32
        assert figure in flat, figure
    plain = header[header.index("PHGR13Verify (pinochio.go:281-378) for nproofs proofs under ONE key"):header.index("} ps_phgr13_batch_info;")]
    assert "ps_phgr13_verify_batch_locate" in plain and "can be halved by the caller" not in header


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name
    assert re.search(r"\bT ps_debug_phgr13_verify_locate_ms\b", out)
    assert "ps_debug_phgr13_verify_locate_ms" not in _read("include", "playsnark_hip.h")


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    vk = _lib.Phgr13Vk()  # its three arrays are NULL
    one = (_lib.Phgr13Proof * 1)()
    valid, failed = C.create_string_buffer(1), C.create_string_buffer(1)
    n = C.c_size_t(7)
    assert lib.ps_phgr13_verify_batch_locate(None, C.byref(vk), None, one, 1, bytes(32), valid, failed, C.byref(n)) == _lib.PS_ERR_ARG
    assert b"ps_phgr13_verify_batch_locate" in lib.ps_last_error()
    assert lib.ps_phgr13_verify_batch_locate(None, None, None, None, 0, None, None, None, None) == _lib.PS_ERR_ARG
    assert lib.ps_phgr13_verify_batch_locate_info(None, None) == _lib.PS_ERR_ARG
    info = _lib.Phgr13LocateInfo()
    assert lib.ps_phgr13_verify_batch_locate_info(None, C.byref(info)) == _lib.PS_ERR_ARG
    assert b"ps_phgr13_verify_batch_locate_info" in lib.ps_last_error()


def test_mirrors_name_the_entries():
    import inspect

    from playsnark_amd import api

    hpp, go, integ = _read("playsnark_amd", "host", "playsnark.hpp"), _read("shim", "playsnark_hip.go"), _read("INTEGRATION.md")
    for name in ARGS:
        assert name + "(" in hpp, name
        assert name in integ, name
        assert "C." + name + "(" in go, name
    assert "PHGR13VerifyBatchLocate(" in hpp
    assert "func PHGR13VerifyBatchLocateHIP(" in go and "PHGR13VerifyBatchLocateHIP" in integ
    assert callable(api.PHGR13VerifyBatchLocate)
    assert inspect.signature(api.PHGR13VerifyBatch).parameters["locate"].default is False


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    exe = str(tmp_path / "abi_smoke_phgr13_verify_locate")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_phgr13_verify_locate.c"), "-o", exe, "-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
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
def test_c_caller_locates_the_bad_proof_of_seven(tmp_path):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "abi_smoke_phgr13_verify_locate ok" in res.stdout
