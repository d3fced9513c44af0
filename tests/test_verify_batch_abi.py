"""CPU: the two entries of the batch verifier (ps_pairing_product_is_one, ps_groth16_verify_batch) are declared in the
header with the argument lists the binding uses, exported by the built library, refuse NULL arguments without touching a
device, and the library still stages through context buffers only."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
ARGS = {"ps_pairing_product_is_one": 5, "ps_groth16_verify_batch": 7}


def _prototypes():
    src = open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ps_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def test_entries_are_declared_with_the_documented_arguments():
    from playsnark_amd import _lib

    protos = _prototypes()
    for name, nargs in ARGS.items():
        assert name in protos, name
        assert len([a for a in protos[name].split(",") if a.strip()]) == nargs, protos[name]
        assert name in _lib.SYMBOLS
        assert len(getattr(_lib.lib, name).argtypes) == nargs
    assert "#define PS_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def test_entries_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for name in ARGS:
        assert re.search(r"\bT %s\b" % name, out), name


def test_null_arguments_are_refused_without_a_device():
    from playsnark_amd import _lib

    lib = _lib.lib
    one = C.c_int(7)
    assert lib.ps_pairing_product_is_one(None, None, None, 1, C.byref(one)) == _lib.PS_ERR_ARG
    assert lib.ps_pairing_product_is_one(None, None, None, 0, None) == _lib.PS_ERR_ARG
    assert b"ps_pairing_product_is_one" in lib.ps_last_error()
    vk = _lib.Groth16Vk()
    assert lib.ps_groth16_verify_batch(None, C.byref(vk), None, None, 0, None, C.byref(one)) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_verify_batch(None, None, None, b"\0" * 384, 1, b"\0" * 32, None) == _lib.PS_ERR_ARG
    assert b"ps_groth16_verify_batch" in lib.ps_last_error()


def test_library_still_does_not_import_the_stream_ordered_allocator():
    syms = subprocess.run(["nm", "-D", "--undefined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "hipMallocAsync" not in syms and "hipFreeAsync" not in syms
