"""CPU: the entry points for the proofs of every node of the domain -- ps_kzg_all_key_lagrange, ps_kzg_open_all_lagrange -- are
declared in the header with their argument lists, exported by the built library, listed and typed in the ctypes binding,
mirrored in the Python surface, the C++ header and the Go shim, and came in WITHIN ABI revision 5."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_kzg_all_key_lagrange": "ps_ctx*, const ps_qap*, const ps_points*, ps_points**",
    "ps_kzg_open_all_lagrange": "ps_ctx*, const ps_qap*, const ps_points*, const ps_points*, const ps_scalars*, ps_points**",
}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _types_only(args: str) -> str:
    """'ps_ctx* ctx, uint8_t out[96]' -> 'ps_ctx*, uint8_t[96]'"""
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        m = re.match(r"^(.*?)(\w+)(\[\d+\])?$", a)
        assert m, a
        out.append((m.group(1).strip() + (m.group(3) or "")).replace(" *", "*"))
    return ", ".join(out)


def test_header_declares_the_entries_with_these_argument_lists():
    h = _read("include", "playsnark_hip.h")
    src = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, want in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        assert _types_only(m.group(1)) == want, name
    # the identity, the limit and the conventions
    assert "pi_m = v_m K_m - U_m + g_m lag_g1[m-1]" in h
    assert "S = 2^p >= 2n - 1" in h and "n > 2^30 is PS_ERR_ARG" in h
    assert "kappa is antisymmetric" in h and "one identity point" in h
    assert "computed inside the call and dropped" in h


def test_library_exports_and_binding_lists_them():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n, args in DECLARED.items():
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes is not None, f"{n} bound without argument types"
        assert len(getattr(_lib.lib, n).argtypes) == len(args.split(",")), n


def test_the_stage_hook_is_exported_and_stays_out_of_the_header():
    from playsnark_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT ps_debug_kzg_all_stage_ms\b", out)
    assert "ps_debug_kzg_all_stage_ms" not in _read("include", "playsnark_hip.h")


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    h = _read("include", "playsnark_hip.h")
    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", h)
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    assert re.search(r"Then\s+\*?\s*ps_kzg_all_key_lagrange and ps_kzg_open_all_lagrange", h)  # appended to the revision list


def test_the_limit_is_a_constant_of_the_plan_header():
    plan = _read("playsnark_amd", "csrc", "kzg_all_plan.hpp")
    assert re.search(r"constexpr uint64_t KZG_ALL_MAX_N\s*=\s*\(uint64_t\)1 << 30;", plan)
    assert "2^30" in _read("playsnark_amd", "csrc", "kzg.inc")


def test_the_point_kernels_multiply_with_ec_mul_fr_and_the_correlation_is_written_once():
    hpp = _read("playsnark_amd", "csrc", "kzg_all.hpp")
    for name in ("k_kzg_all_load", "k_kzg_all_combine"):
        body = hpp[hpp.index("k_" + name[2:] + "(") :]
        body = body[: body.index("\n}\n")]
        assert "ec_mul_fr<KF>(" in body, name
    inc = _read("playsnark_amd", "csrc", "kzg.inc")
    assert len(re.findall(r"\bstatic void ec_correlate\(", inc)) == 1
    assert len(re.findall(r"\bec_correlate<F>\(", inc)) == 2  # the two new entries share it


def test_api_cpp_and_go_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.KZGAllKeyLagrange) and callable(api.KZGOpenAllLagrange)
    go = _read("shim", "playsnark_hip.go")
    for n in ("KZGAllKeyLagrange", "KZGOpenAllLagrange"):
        assert re.search(r"func\s+(\([^)]*\)\s*)?%s\s*\(" % n, go), n
    cpp = _read("playsnark_amd", "host", "playsnark.hpp")
    for n in ("KZGAllKeyLagrange", "KZGOpenAllLagrange"):
        assert re.search(r"\b%s\s*\(" % n, cpp), n
    for sym in DECLARED:
        assert "C." + sym in go, sym
        assert sym + "(" in cpp, sym


def test_null_arguments_are_refused_without_a_device():
    """The NULL checks come before anything is read through the context, so they need no GPU.  (Every other check of these
    calls reads the domain or the arrays first and is covered on the device.)"""
    from playsnark_amd import _lib

    lib = _lib.lib
    out = ctypes.c_void_p()
    for name, call in {
        "ps_kzg_all_key_lagrange": lambda: lib.ps_kzg_all_key_lagrange(None, None, None, ctypes.byref(out)),
        "ps_kzg_open_all_lagrange": lambda: lib.ps_kzg_open_all_lagrange(None, None, None, None, None, ctypes.byref(out)),
    }.items():
        assert call() == _lib.PS_ERR_ARG, name
        assert lib.ps_last_error().decode() == name + ": NULL argument"
    assert lib.ps_kzg_all_key_lagrange(None, None, None, None) == _lib.PS_ERR_ARG
    assert lib.ps_kzg_open_all_lagrange(None, None, None, None, None, None) == _lib.PS_ERR_ARG
