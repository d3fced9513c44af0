"""CPU: the entry points for many polynomials at shared points -- ps_scalars_lincomb, ps_kzg_open_multi, ps_kzg_verify_multi --
are declared in the header with their argument lists, exported by the built library, listed and typed in the ctypes binding,
mirrored in the Python surface, the C++ header and the Go shim, and came in WITHIN ABI revision 5."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_scalars_lincomb": "ps_ctx*, const ps_scalars* const*, size_t, const uint8_t*, size_t, ps_scalars**",
    "ps_kzg_open_multi": "ps_ctx*, const ps_points*, const ps_scalars* const*, size_t, const uint8_t*, size_t, const uint8_t*, uint8_t*, uint8_t*",
    "ps_kzg_verify_multi": "ps_ctx*, const uint8_t[192], const uint8_t*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, "
                           "const uint8_t*, const uint8_t*, int, int*",
}


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def _types_only(args: str) -> str:
    """'ps_ctx* ctx, const uint8_t tau_g2_1[192]' -> 'ps_ctx*, const uint8_t[192]'"""
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        m = re.match(r"^(.*?)(\w+)(\[\d+\])?$", a)
        assert m, a
        out.append((m.group(1).strip() + (m.group(3) or "")).replace(" *", "*"))
    return ", ".join(out)


def test_header_declares_the_entries_with_these_argument_lists():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, want in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        assert _types_only(m.group(1)) == want, name
    h = _header()
    # the limits of the combination, who chooses the weights, and what is guaranteed
    assert "t * N < 2^32" in h and "m * t <= 2^20" in h
    assert "drawn AFTER the commitments and the values are fixed" in h
    assert "call returns ps_kzg_open's bytes" in h


def test_library_exports_and_binding_lists_them():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n in DECLARED:
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes is not None, f"{n} bound without argument types"
        assert len(getattr(_lib.lib, n).argtypes) == len(DECLARED[n].split(",")), n


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    assert "Then ps_scalars_lincomb, ps_kzg_open_multi and" in _header()  # appended to the revision list


def test_api_cpp_and_go_mirrors_exist():
    from playsnark_amd import api

    for n in ("LinComb", "Add", "Sub"):
        assert callable(getattr(api.Poly, n)), n
    for n in ("KZGOpenMulti", "KZGVerifyMulti"):
        assert callable(getattr(api, n)), n
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("LinCombHIP", "KZGOpenMulti", "KZGVerifyMulti"):
        assert re.search(r"func\s+%s\s*\(" % n, go), n
    cpp = open(os.path.join(ROOT, "playsnark_amd", "host", "playsnark.hpp")).read()
    for n in ("LinComb", "KZGOpenMulti", "KZGVerifyMulti"):
        assert re.search(r"\b%s\s*\(" % n, cpp), n
    for sym in DECLARED:
        assert "C." + sym in go, sym
        assert sym + "(" in cpp, sym


def test_null_arguments_are_refused_without_a_device():
    """The NULL checks come before anything is read through the context, so they need no GPU.  (Every other check of these
    calls reads the context's queue first, as ps_kzg_verify_batch does, and is covered on the device.)"""
    from playsnark_amd import _lib

    lib = _lib.lib
    ok = ctypes.c_int(-1)
    out = ctypes.c_void_p()
    ident2 = b"\x40" + bytes(191)
    one = (1).to_bytes(32, "big")
    assert lib.ps_kzg_verify_multi(None, ident2, None, 0, None, 0, None, None, None, None, 1, ctypes.byref(ok)) == _lib.PS_ERR_ARG
    assert lib.ps_scalars_lincomb(None, None, 1, one, 1, ctypes.byref(out)) == _lib.PS_ERR_ARG
    assert lib.ps_kzg_open_multi(None, None, None, 1, one, 1, one, None, None) == _lib.PS_ERR_ARG
