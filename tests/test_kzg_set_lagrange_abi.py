"""CPU: the entry points for a set of points of a polynomial held as its values on the domain -- ps_poly_lagrange_set_group,
ps_poly_div_roots_lagrange, ps_kzg_open_set_lagrange -- are declared in the header with their argument lists, exported by the
built library, listed and typed in the ctypes binding, mirrored in the Python surface, the C++ header and the Go shim, and came
in WITHIN ABI revision 5."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_poly_lagrange_set_group": "void",
    "ps_poly_div_roots_lagrange": "ps_ctx*, const ps_qap*, const ps_scalars*, const uint8_t*, size_t, ps_scalars**, uint8_t*, uint8_t*",
    "ps_kzg_open_set_lagrange": "ps_ctx*, const ps_qap*, const ps_points*, const ps_scalars*, const uint8_t*, size_t, uint8_t*, uint8_t[96]",
}


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def _types_only(args: str) -> str:
    """'ps_ctx* ctx, uint8_t out[96]' -> 'ps_ctx*, uint8_t[96]'"""
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
    # the identity, the limits and the conventions
    assert "q(i) = sum_j c_j (y_j - v_i) / (z_j - i)" in h
    assert "ceil(k / G) partial rows of n scalars" in h and "never k * n" in h
    assert "k > 1024 or k * n >= 2^32" in h and "the message names both indices" in h


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
    assert re.search(r"Then\s+\*?\s*ps_poly_lagrange_set_group, ps_poly_div_roots_lagrange and ps_kzg_open_set_lagrange", _header())  # appended to the revision list


def test_the_group_is_a_constant_of_the_build_and_needs_no_device():
    from playsnark_amd import _lib

    g = _lib.lib.ps_poly_lagrange_set_group()
    plan = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_lagrange_set_plan.hpp")).read()
    assert g == int(re.search(r"#else\s*\n\s*constexpr int POLY_LAGR_SET_GROUP\s*=\s*(\d+)\s*;", plan).group(1))
    assert 2 <= g <= 32  # one inversion serves more than one point


def test_api_cpp_and_go_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.Poly.DivRootsLagrange) and callable(api.KZGOpenSetLagrange)
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("PolyLagrangeSetGroup", "DivRootsLagrangeHIP", "KZGOpenSetLagrange"):
        assert re.search(r"func\s+(\([^)]*\)\s*)?%s\s*\(" % n, go), n
    cpp = open(os.path.join(ROOT, "playsnark_amd", "host", "playsnark.hpp")).read()
    for n in ("DivRootsLagrange", "KZGOpenSetLagrange"):
        assert re.search(r"\b%s\s*\(" % n, cpp), n
    for sym in DECLARED:
        assert "C." + sym in go, sym
    for sym in ("ps_poly_div_roots_lagrange", "ps_kzg_open_set_lagrange"):
        assert sym + "(" in cpp, sym


def test_null_arguments_are_refused_without_a_device():
    """The NULL checks come before anything is read through the context, so they need no GPU.  (Every other check of these
    calls reads the domain or the values first and is covered on the device.)"""
    from playsnark_amd import _lib

    lib = _lib.lib
    out = ctypes.c_void_p()
    one = (1).to_bytes(32, "big")
    buf = ctypes.create_string_buffer(96)
    for name, call in {
        "ps_poly_div_roots_lagrange": lambda: lib.ps_poly_div_roots_lagrange(None, None, None, one, 1, ctypes.byref(out), buf, None),
        "ps_kzg_open_set_lagrange": lambda: lib.ps_kzg_open_set_lagrange(None, None, None, None, one, 1, buf, buf),
    }.items():
        assert call() == _lib.PS_ERR_ARG, name
        assert lib.ps_last_error().decode() == name + ": NULL argument"
    assert lib.ps_poly_div_roots_lagrange(None, None, None, one, 1, None, buf, None) == _lib.PS_ERR_ARG
