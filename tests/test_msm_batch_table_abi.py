"""ps_msm_batch_set_table, added within ABI revision 5: declared in the header with the argument list the binding uses, listed
in _lib.py, exported by the built library, mirrored in host/playsnark.hpp (which still compiles), the Go shim and
INTEGRATION.md; it refuses a NULL context without touching a device, and on a context every mode outside 0..2."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
NAME = "ps_msm_batch_set_table"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_is_declared_with_the_documented_arguments():
    from playsnark_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", _read("include", "playsnark_hip.h"), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(ps_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    assert NAME in protos
    assert len([a for a in protos[NAME].split(",") if a.strip()]) == 2, protos[NAME]
    assert NAME in _lib.SYMBOLS
    assert len(getattr(_lib.lib, NAME).argtypes) == 2
    assert "#define PS_ABI_VERSION 5" in _read("include", "playsnark_hip.h")
    assert _lib.PS_ABI_VERSION == 5 and _lib.lib.ps_abi_version() == 5


def test_entry_is_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s\b" % NAME, out)


def test_null_context_is_refused_without_a_device():
    from playsnark_amd import _lib

    for mode in (0, 1, 2, 3):
        assert _lib.lib.ps_msm_batch_set_table(None, mode) == _lib.PS_ERR_ARG
        assert NAME.encode() in _lib.lib.ps_last_error()


def test_mirrors_name_the_entry(tmp_path):
    hpp, go, integ = _read("playsnark_amd", "host", "playsnark.hpp"), _read("shim", "playsnark_hip.go"), _read("INTEGRATION.md")
    assert NAME in hpp and "SetBatchTable(" in hpp
    assert "C.%s(" % NAME in go and "func SetBatchTableHIP(" in go
    assert NAME in integ
    src = tmp_path / "use_batch_table.cpp"
    src.write_text('#include "playsnark_amd/host/playsnark.hpp"\n'
                   "void plain(playsnark::Context& c) { playsnark::SetBatchTable(c, 1); }\n")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, "-c", str(src), "-o", str(tmp_path / "use_batch_table.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]


@pytest.mark.gpu
def test_modes_outside_0_to_2_are_refused(ps_api, ctx):
    try:
        for mode in (0, 1, 2):
            ctx.set_batch_table(mode)
        for mode in (-1, 3, 1 << 20):
            with pytest.raises(ps_api.PlaysnarkError) as e:
                ctx.set_batch_table(mode)
            assert e.value.code == -5 and NAME in str(e.value)
    finally:
        ctx.set_batch_table(0)
