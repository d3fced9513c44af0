"""CPU: the two entries of the locating batch verifier (ps_groth16_verify_batch_locate, ps_groth16_verify_batch_locate_info)
are declared in the header with the documented argument lists, exported by the built library, mirrored by the Python
binding, host/playsnark.hpp, the Go shim and INTEGRATION.md, added within ABI revision 5, and refuse NULL arguments without
touching a device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_groth16_verify_batch_locate": 8, "ps_groth16_verify_batch_locate_info": 2}


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


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
    args = [" ".join(a.split()) for a in protos["ps_groth16_verify_batch_locate"].split(",")]
    assert args == ["ps_ctx* ctx", "const ps_groth16_vk* vk", "const ps_scalars* io", "const uint8_t* proofs", "size_t nproofs",
                    "const uint8_t* rho_be32", "uint8_t* valid", "size_t* ninvalid"]
    # the leading arguments are those of the plain batch call
    plain = [" ".join(a.split()) for a in protos["ps_groth16_verify_batch"].split(",")]
    assert args[:6] == plain[:6]
    header = _read("include", "playsnark_hip.h")
    m = re.search(r"typedef struct \{([^}]*)\} ps_verify_locate_info;", header)
    assert m and re.findall(r"uint32_t\s+(\w+);", m.group(1)) == ["checks", "levels", "invalid", "reserved"]
    assert C.sizeof(_lib.VerifyLocateInfo) == 16 and [f for f, _ in _lib.VerifyLocateInfo._fields_] == ["checks", "levels", "invalid", "reserved"]


def test_the_abi_revision_did_not_move():
    from playsnark_amd import _lib

    assert "#define PS_ABI_VERSION 5" in _read("include", "playsnark_hip.h")
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5


def test_the_header_states_soundness_cost_and_reference():
    header = _read("include", "playsnark_hip.h")
    doc = header[header.index("WHICH proofs of a batch are invalid"):header.index("} ps_verify_locate_info;")]
    for needle in ("groth16.go:214-233", "nproofs / 2^bits(rho)", "always exact", "1 + 2 b ceil(log2 N)", "B per proof", "PS_ERR_HIP", "2^20"):
        assert needle in doc, needle


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name


def test_the_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.Groth16VerifyBatchLocate)
    hpp = _read("playsnark_amd", "host", "playsnark.hpp")
    assert "Groth16VerifyBatchLocate(" in hpp and "ps_groth16_verify_batch_locate(" in hpp and "ps_groth16_verify_batch_locate_info(" in hpp
    shim = _read("shim", "playsnark_hip.go")
    assert "func Groth16VerifyBatchLocateHIP(" in shim and "C.ps_groth16_verify_batch_locate(" in shim
    doc = _read("INTEGRATION.md")
    assert "ps_groth16_verify_batch_locate" in doc and "Groth16VerifyBatchLocateHIP" in doc


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    vk = _lib.Groth16Vk()
    n = C.c_size_t(7)
    valid = C.create_string_buffer(1)
    assert lib.ps_groth16_verify_batch_locate(None, C.byref(vk), None, None, 0, None, None, C.byref(n)) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_verify_batch_locate(None, None, None, b"\0" * 384, 1, b"\0" * 32, valid, None) == _lib.PS_ERR_ARG
    assert b"ps_groth16_verify_batch_locate" in lib.ps_last_error()
    info = _lib.VerifyLocateInfo()
    assert lib.ps_groth16_verify_batch_locate_info(None, C.byref(info)) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_verify_batch_locate_info(None, None) == _lib.PS_ERR_ARG
    assert b"ps_groth16_verify_batch_locate_info" in lib.ps_last_error()
