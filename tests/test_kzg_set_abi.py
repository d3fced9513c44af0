"""CPU: the entry points for one polynomial at a set of points -- ps_poly_scan_set_group, ps_poly_div_roots, ps_kzg_open_set,
ps_kzg_verify_set -- are declared in the header with their argument lists, exported by the built library, listed and typed in
the ctypes binding, mirrored in the Python surface, the C++ header and the Go shim, and came in WITHIN ABI revision 5."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_poly_scan_set_group": "void",
    "ps_poly_div_roots": "ps_ctx*, const ps_scalars*, const uint8_t*, size_t, ps_scalars**, uint8_t*, uint8_t*",
    "ps_kzg_open_set": "ps_ctx*, const ps_points*, const ps_scalars*, const uint8_t*, size_t, uint8_t*, uint8_t[96]",
    "ps_kzg_verify_set": "ps_ctx*, const ps_points*, const ps_points*, const uint8_t[96], const uint8_t*, const uint8_t*, size_t, "
                         "const uint8_t[96], int, int*",
}


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def _types_only(args: str) -> str:
    """'ps_ctx* ctx, const uint8_t commit[96]' -> 'ps_ctx*, const uint8_t[96]'"""
    if args.strip() == "void":
        return "void"
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
    # the two equations, the limits, and the reference lines
    assert "q = sum_j w_j (p - p(z_j)) / (X - z_j)" in h
    assert "e(commit - [r(tau)] G1, G2) * e(-proof, [Z_S(tau)] G2) == 1" in h
    assert "k > 1024" in h and "k * n >= 2^32" in h
    assert "algebra.go:119-137" in h


def test_library_exports_and_binding_lists_them():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n, args in DECLARED.items():
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes is not None, f"{n} bound without argument types"
        assert len(getattr(_lib.lib, n).argtypes) == (0 if args == "void" else len(args.split(","))), n


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    assert "Then ps_poly_scan_set_group, ps_poly_div_roots, ps_kzg_open_set and" in _header()  # appended to the revision list


def test_the_group_is_a_constant_of_the_build_and_needs_no_device():
    from playsnark_amd import _lib

    g = _lib.lib.ps_poly_scan_set_group()
    assert 1 <= g <= 32  # above 32 the accumulators would need the reduction step inside a group
    plan = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_scan_set_plan.hpp")).read()
    assert re.search(r"POLY_SCAN_SET_GROUP\s*=\s*%d\s*;" % g, plan)
    assert re.search(r"PS_KZG_SET_MAX\s*=\s*1024\s*;", plan)


def test_api_cpp_and_go_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.Poly.DivRoots)
    for n in ("KZGOpenSet", "KZGVerifySet"):
        assert callable(getattr(api, n)), n
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("DivRootsHIP", "KZGOpenSet", "KZGVerifySet"):
        assert re.search(r"func\s+(\([^)]*\)\s*)?%s\s*\(" % n, go), n
    cpp = open(os.path.join(ROOT, "playsnark_amd", "host", "playsnark.hpp")).read()
    for n in ("DivRoots", "KZGOpenSet", "KZGVerifySet"):
        assert re.search(r"\b%s\s*\(" % n, cpp), n
    for sym in ("ps_poly_div_roots", "ps_kzg_open_set", "ps_kzg_verify_set"):
        assert "C." + sym in go, sym
        assert sym + "(" in cpp, sym


def test_null_arguments_are_refused_without_a_device():
    """The NULL checks come before anything is read through the context, so they need no GPU.  (Every other check of these
    calls reads the context or the polynomial first and is covered on the device.)"""
    from playsnark_amd import _lib

    lib = _lib.lib
    ok = ctypes.c_int(-1)
    out = ctypes.c_void_p()
    one = (1).to_bytes(32, "big")
    ident = b"\x40" + bytes(95)
    buf = ctypes.create_string_buffer(96)
    assert lib.ps_poly_div_roots(None, None, one, 1, ctypes.byref(out), buf, None) == _lib.PS_ERR_ARG
    assert "NULL argument" in lib.ps_last_error().decode()
    assert lib.ps_poly_div_roots(None, None, one, 1, None, buf, None) == _lib.PS_ERR_ARG
    assert lib.ps_kzg_open_set(None, None, None, one, 1, buf, buf) == _lib.PS_ERR_ARG
    assert lib.ps_kzg_verify_set(None, None, None, ident, one, one, 1, ident, 1, ctypes.byref(ok)) == _lib.PS_ERR_ARG
    assert ok.value == -1  # refused before the verdict is touched
