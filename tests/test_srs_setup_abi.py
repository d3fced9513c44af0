"""CPU: the entry points of the setup from a powers-of-tau string -- ps_qap_column_sums, ps_groth16_setup_from_srs,
ps_groth16_crs_contribute, ps_groth16_crs_check_update -- are exported by the built library, declared in the header and
mirrored in the Python surface, and they came in WITHIN ABI revision 5 (no existing struct changed: found by symbol)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ps_qap_column_sums", "ps_groth16_setup_from_srs", "ps_groth16_crs_contribute", "ps_groth16_crs_check_update")


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def test_library_exports_the_four_symbols():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n in NEW:
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes, f"{n} bound without argument types"


def test_header_declares_them_and_the_srs_struct():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ps_groth16_srs\s*;", src)
    assert m, "ps_groth16_srs not declared"
    fields = re.findall(r"(\w+)\s*(?:\[\d+\])?\s*;", m.group(1))
    assert fields == ["tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"], fields
    # the section cites what it replaces
    assert "groth16.go:64-101" in _header() and "groth16.go:254-264" in _header()


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5


def test_srs_struct_mirror_matches_the_header_layout():
    from playsnark_amd import _lib

    s = _lib.Groth16Srs
    assert [f for f, _ in s._fields_] == ["tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"]
    assert ctypes.sizeof(s) == 4 * ctypes.sizeof(ctypes.c_void_p) + 192 and s.beta_g2.offset == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_api_has_the_mirrors():
    from playsnark_amd import api

    assert callable(api.QAP.column_sums)
    for n in ("Groth16SRS", "NewGroth16SetupFromSRS", "Groth16Contribute", "Groth16CheckUpdate"):
        assert callable(getattr(api, n)), n
