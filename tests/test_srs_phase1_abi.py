"""CPU: the phase-1 entry points -- ps_scalars_powers, ps_groth16_srs_contribute, ps_groth16_srs_check,
ps_groth16_srs_check_update -- are exported by the built library, declared in the header (with ps_groth16_srs_share) and mirrored
in the Python and C++ surfaces, and they came in WITHIN ABI revision 5 (no existing struct changed: found by symbol)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ps_scalars_powers", "ps_groth16_srs_contribute", "ps_groth16_srs_check", "ps_groth16_srs_check_update")


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def test_library_exports_the_symbols():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n in NEW:
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes, f"{n} bound without argument types"


def test_header_declares_them_and_the_share_struct():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ps_groth16_srs_share\s*;", src)
    assert m, "ps_groth16_srs_share not declared"
    assert re.findall(r"(\w+)\s*\[192\]", m.group(1)) == ["t_g2", "a_g2", "b_g2"]
    # the setup from a string now points at the check instead of disclaiming it
    assert "not done here" not in _header()
    assert re.search(r"ps_groth16_srs_check\s*\(below\)", _header())


def test_abi_revision_is_still_5_and_the_srs_struct_unchanged():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5
    s = _lib.Groth16Srs
    assert [f for f, _ in s._fields_] == ["tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"]
    assert ctypes.sizeof(s) == 4 * ctypes.sizeof(ctypes.c_void_p) + 192


def test_share_struct_mirror_matches_the_header_layout():
    from playsnark_amd import _lib

    s = _lib.Groth16SrsShare
    assert [f for f, _ in s._fields_] == ["t_g2", "a_g2", "b_g2"]
    assert ctypes.sizeof(s) == 3 * 192 and s.a_g2.offset == 192 and s.b_g2.offset == 384


def test_api_and_cpp_mirrors_exist():
    from playsnark_amd import api

    assert callable(api.Poly.powers) and callable(api.Groth16SRS.initial) and callable(api.Groth16SRS.truncate)
    for n in ("Groth16SRSContribute", "Groth16SRSCheck", "Groth16SRSCheckUpdate"):
        assert callable(getattr(api, n)), n
    hpp = open(os.path.join(ROOT, "playsnark_amd", "host", "playsnark.hpp")).read()
    go = open(os.path.join(ROOT, "shim", "playsnark_hip.go")).read()
    for n in ("Groth16SRSContribute", "Groth16SRSCheck", "Groth16SRSCheckUpdate"):
        assert re.search(r"\b%s\s*\(" % n, hpp), n
        assert re.search(r"func\s+%s\s*\(" % n, go), n
    for sym in NEW:
        assert sym in hpp and "C." + sym in go, sym
