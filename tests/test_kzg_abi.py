"""CPU: the KZG entry points -- ps_poly_scan_tile, ps_poly_eval, ps_poly_div_linear, ps_kzg_commit, ps_kzg_open, ps_kzg_verify,
ps_kzg_verify_batch -- are declared in the header with their argument lists, exported by the built library, listed and typed
in the ctypes binding, mirrored in the Python surface and the Go shim, and came in WITHIN ABI revision 5."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the argument list the header declares, types only, white space squeezed
DECLARED = {
    "ps_poly_scan_tile": "void",
    "ps_poly_eval": "ps_ctx*, const ps_scalars*, const uint8_t*, size_t, uint8_t*",
    "ps_poly_div_linear": "ps_ctx*, const ps_scalars*, const uint8_t*, size_t, ps_scalars**, uint8_t*",
    "ps_kzg_commit": "ps_ctx*, const ps_points*, const ps_scalars*, uint8_t[96]",
    "ps_kzg_open": "ps_ctx*, const ps_points*, const ps_scalars*, const uint8_t*, size_t, uint8_t*, uint8_t*",
    "ps_kzg_verify": "const uint8_t[192], const uint8_t[96], const uint8_t[32], const uint8_t[32], const uint8_t[96], int*",
    "ps_kzg_verify_batch": "ps_ctx*, const uint8_t[192], const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, "
                           "size_t, int, int*",
}


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def _types_only(args: str) -> str:
    """'ps_ctx* ctx, const uint8_t tau_g2_1[192]' -> 'ps_ctx*, const uint8_t[192]'"""
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        if a == "void":
            out.append(a)
            continue
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
    # the header states the false-accept bound of the batch and the equation of the single check
    assert "false-accept bound" in _header()
    assert "e(commit - y G1 + z proof, G2) = e(proof, tau_g2_1)" in _header()


def test_library_exports_and_binding_lists_them():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n in DECLARED:
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes is not None, f"{n} bound without argument types"
        nargs = 0 if DECLARED[n] == "void" else len(DECLARED[n].split(","))
        assert len(getattr(_lib.lib, n).argtypes) == nargs, n


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    assert "ps_kzg_verify and ps_kzg_verify_batch (no struct at all)" in _header()  # appended to the revision list


def test_the_tile_is_a_whole_number_of_workgroup_rows():
    """ps_poly_scan_tile needs no device: 256 threads times the items of a thread."""
    from playsnark_amd import _lib

    t = _lib.lib.ps_poly_scan_tile()
    assert t >= 256 and t % 256 == 0


def test_api_and_go_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.Poly.Eval) and callable(api.Poly.DivLinear)
    for n in ("KZGCommit", "KZGOpen", "KZGVerify", "KZGVerifyBatch"):
        assert callable(getattr(api, n)), n
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("KZGCommit", "KZGOpen", "KZGVerify", "KZGVerifyBatch", "PolyScanTile"):
        assert re.search(r"func\s+%s\s*\(" % n, go), n
    for n in ("EvalHIP", "DivLinearHIP"):
        assert re.search(r"func\s+\(p Poly\)\s+%s\s*\(" % n, go), n
    for sym in DECLARED:
        assert "C." + sym in go, sym


def test_host_only_argument_checks_need_no_device():
    """ps_kzg_verify runs on the host: NULL, a scalar that is not below r and a point that is not on the curve are told apart
    without a GPU."""
    from playsnark_amd import _lib

    lib = _lib.lib
    ok = ctypes.c_int(-1)
    ident1, ident2 = b"\x40" + bytes(95), b"\x40" + bytes(191)
    one, r = (1).to_bytes(32, "big"), (0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001).to_bytes(32, "big")
    assert lib.ps_kzg_verify(None, ident1, one, one, ident1, ctypes.byref(ok)) == _lib.PS_ERR_ARG
    assert lib.ps_kzg_verify(ident2, ident1, r, one, ident1, ctypes.byref(ok)) == _lib.PS_ERR_ENCODING
    assert lib.ps_kzg_verify(ident2, ident1, one, r, ident1, ctypes.byref(ok)) == _lib.PS_ERR_ENCODING
    off_curve = (1).to_bytes(48, "big") + (1).to_bytes(48, "big")
    assert lib.ps_kzg_verify(ident2, off_curve, one, one, ident1, ctypes.byref(ok)) == _lib.PS_ERR_ENCODING
    # the commitment of the zero polynomial opens to 0 everywhere with the identity proof: 0 - 0 G1 + z 0 = 0
    assert lib.ps_kzg_verify(ident2, ident1, one, bytes(32), ident1, ctypes.byref(ok)) == _lib.PS_OK and ok.value == 1
