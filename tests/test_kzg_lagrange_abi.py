"""CPU: the entry points for polynomials held as their values on the domain -- ps_poly_lagrange_tile, ps_qap_gate_values,
ps_poly_eval_lagrange, ps_poly_div_linear_lagrange, ps_kzg_commit_lagrange, ps_kzg_open_lagrange -- are declared in the header
with their argument lists, exported by the built library, listed and typed in the ctypes binding, mirrored in the Python surface,
the C++ header and the Go shim, and came in WITHIN ABI revision 5."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_poly_lagrange_tile": "void",
    "ps_qap_gate_values": "ps_ctx*, const ps_qap*, const ps_scalars*, int, ps_scalars**",
    "ps_poly_eval_lagrange": "ps_ctx*, const ps_qap*, const ps_scalars*, const uint8_t*, size_t, uint8_t*",
    "ps_poly_div_linear_lagrange": "ps_ctx*, const ps_qap*, const ps_scalars*, const uint8_t*, size_t, ps_scalars**, uint8_t*",
    "ps_kzg_commit_lagrange": "ps_ctx*, const ps_points*, const ps_scalars*, uint8_t[96]",
    "ps_kzg_open_lagrange": "ps_ctx*, const ps_qap*, const ps_points*, const ps_scalars*, const uint8_t*, size_t, uint8_t*, uint8_t*",
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
    # the identities, the limits and the conventions
    assert "p(z) = prod_i (z - i) * sum_i w_i v_i e_i" in h
    assert "q_m = (sum_{i != m} w_i v_i e_i - v_m sum_{i != m} w_i e_i) / w_m" in h
    assert "k * n >= 2^32" in h and "exactly n elements" in h
    assert "ps_points_monomial_to_lagrange" in h and "ps_points_lagrange_check" in h


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
    assert "Then ps_poly_lagrange_tile, ps_qap_gate_values, ps_poly_eval_lagrange," in _header()  # appended to the revision list


def test_the_tile_is_a_constant_of_the_build_and_needs_no_device():
    from playsnark_amd import _lib

    t = _lib.lib.ps_poly_lagrange_tile()
    plan = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_lagrange_plan.hpp")).read()
    log_items = int(re.search(r"#else\s*\n\s*constexpr int POLY_LAGR_LOG_ITEMS\s*=\s*(\d+)\s*;", plan).group(1))
    assert t == 256 << log_items and 1 <= log_items <= 4


def test_api_cpp_and_go_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.QAP.gate_values) and callable(api.Poly.EvalLagrange) and callable(api.Poly.DivLinearLagrange)
    for n in ("KZGCommitLagrange", "KZGOpenLagrange"):
        assert callable(getattr(api, n)), n
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("GateValuesHIP", "EvalLagrangeHIP", "DivLinearLagrangeHIP", "KZGCommitLagrange", "KZGOpenLagrange"):
        assert re.search(r"func\s+(\([^)]*\)\s*)?%s\s*\(" % n, go), n
    cpp = open(os.path.join(ROOT, "playsnark_amd", "host", "playsnark.hpp")).read()
    for n in ("GateValues", "EvalLagrange", "DivLinearLagrange", "KZGCommitLagrange", "KZGOpenLagrange"):
        assert re.search(r"\b%s\s*\(" % n, cpp), n
    for sym in ("ps_qap_gate_values", "ps_poly_eval_lagrange", "ps_poly_div_linear_lagrange", "ps_kzg_commit_lagrange", "ps_kzg_open_lagrange"):
        assert "C." + sym in go, sym
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
        "ps_qap_gate_values": lambda: lib.ps_qap_gate_values(None, None, None, 0, ctypes.byref(out)),
        "ps_poly_eval_lagrange": lambda: lib.ps_poly_eval_lagrange(None, None, None, one, 1, buf),
        "ps_poly_div_linear_lagrange": lambda: lib.ps_poly_div_linear_lagrange(None, None, None, one, 1, ctypes.byref(out), buf),
        "ps_kzg_commit_lagrange": lambda: lib.ps_kzg_commit_lagrange(None, None, None, buf),
        "ps_kzg_open_lagrange": lambda: lib.ps_kzg_open_lagrange(None, None, None, None, one, 1, buf, buf),
    }.items():
        assert call() == _lib.PS_ERR_ARG, name
        assert lib.ps_last_error().decode() == name + ": NULL argument"
    assert lib.ps_poly_div_linear_lagrange(None, None, None, one, 1, None, buf) == _lib.PS_ERR_ARG
