"""CPU: the entry for R1CS matrices with field coefficients -- ps_qap_create_fr and ps_qap_wide_entries -- is exported by the
built library, declared in the header and mirrored in the Python surface, within ABI revision 5; and the Python packing never
narrows a coefficient: a list holding one value that is no int64 goes out as 32-byte canonical values mod r, an all-int64
list as int64, a float not at all."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_circuits as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ps_qap_create_fr", "ps_qap_wide_entries")


def _header():
    return open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()


def test_library_exports_both_symbols():
    from playsnark_amd import _lib

    raw = ctypes.CDLL(_lib.library_path())  # a fresh handle: dlsym, not the binding's attribute cache
    for n in NEW:
        assert getattr(raw, n, None) is not None, f"{n} not exported"
        assert n in _lib.SYMBOLS
        assert getattr(_lib.lib, n).argtypes, f"{n} bound without argument types"


def test_header_declares_them_and_the_struct():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ps_csr_fr\s*;", src)
    assert m, "ps_csr_fr not declared"
    assert re.findall(r"(\w+)\s*;", m.group(1)) == ["row_ptr", "col", "val_be32"]
    # the int64 struct is as it was
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ps_csr\s*;", src)
    assert m and re.findall(r"(\w+)\s*;", m.group(1)) == ["row_ptr", "col", "val"]


def test_abi_revision_is_still_5():
    from playsnark_amd import _lib

    assert re.search(r"#define\s+PS_ABI_VERSION\s+5\b", _header())
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5


def test_struct_mirror_and_api():
    from playsnark_amd import _lib, api

    assert [f for f, _ in _lib.CsrFr._fields_] == ["row_ptr", "col", "val_be32"]
    assert ctypes.sizeof(_lib.CsrFr) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert callable(api.QAP.wide_entries)


def _values(keep):
    return bytes(keep[2])


def test_a_list_with_one_value_beyond_int64_is_packed_as_field_elements():
    from playsnark_amd import _lib, api

    vals = [1, -1, 5, (1 << 63) - 1, -(1 << 63), 1 << 63, -(1 << 63) - 1] + list(wc.EDGE)
    rows = [[(i % 4, v)] for i, v in enumerate(vals)]
    fr, structs, keep = api._csr3((rows, [[(0, 1)]] * len(rows), [[(1, -1)]] * len(rows)))
    assert fr and all(isinstance(s, _lib.CsrFr) for s in structs)
    raw = _values(keep[0])
    assert len(raw) == 32 * len(vals)
    assert [int.from_bytes(raw[32 * i : 32 * i + 32], "big") for i in range(len(vals))] == [v % wc.R for v in vals]
    # one wide matrix takes the other two along: -1 becomes r - 1
    assert _values(keep[2]) == (wc.R - 1).to_bytes(32, "big") * len(rows)
    assert list(keep[0][0]) == list(range(len(vals) + 1)) and list(keep[0][1])[: len(vals)] == [i % 4 for i in range(len(vals))]
    # the single-matrix helper decides for its own matrix, and never narrows either
    s, k = api._csr(rows)
    assert isinstance(s, _lib.CsrFr) and _values(k) == raw


def test_an_all_int64_list_is_still_packed_as_int64():
    from playsnark_amd import _lib, api

    vals = [1, -1, 5, 1 << 62, (1 << 63) - 1, -(1 << 63)]
    rows = [[(i, v), (i + 1, 0)] for i, v in enumerate(vals)]  # (zeros are dropped, as before)
    fr, structs, keep = api._csr3((rows, rows, rows))
    assert not fr and all(isinstance(s, _lib.Csr) for s in structs)
    for k in keep:
        assert isinstance(k[2], ctypes.Array) and k[2]._type_ is ctypes.c_int64 and list(k[2]) == vals
        assert list(k[0]) == list(range(len(vals) + 1))
    s, k = api._csr(rows)
    assert isinstance(s, _lib.Csr) and list(k[2]) == vals


def test_a_float_coefficient_is_a_type_error():
    from playsnark_amd import api

    for bad in (1.0, 2.5, "3", None):
        with pytest.raises(TypeError):
            api._csr3(([[(0, bad)]], [[(0, 1)]], [[(0, 1)]]))
    with pytest.raises(TypeError):
        api._csr(api.dense_to_rows([[1.5]]))
