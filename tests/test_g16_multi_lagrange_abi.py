"""The multi-device Groth16 entries over rank-local Lagrange-form keys, as far as a machine without a GPU can check them: the
library exports ps_groth16_prove_local within ABI revision 5, argument errors are found before any device work, a plain-C99
caller (tests/abi_smoke_g16_multi.c) compiles and links against the header and the shared library alone -- and proves the toy
circuit with a GPU --, and the shipped code object holds the two new kernel families without spills or scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_smoke(tmp_path):
    """As tests/test_abi.py builds its plain-C caller: -pedantic C99 against the header and the shared library alone."""
    pkg = os.path.join(ROOT, "playsnark_amd")
    link = ["-L" + pkg, "-lplaysnark_hip", "-Wl,-rpath," + pkg]
    exe = str(tmp_path / "abi_smoke_g16_multi")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "abi_smoke_g16_multi.c"), "-o", exe] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_library_exports_the_local_entry_within_revision_5():
    import ctypes

    from playsnark_amd import _lib

    assert _lib.lib.ps_abi_version() == _lib.PS_ABI_VERSION == 5
    assert "ps_groth16_prove_local" in _lib.SYMBOLS and hasattr(_lib.lib, "ps_groth16_prove_local")
    header = open(os.path.join(ROOT, "include", "playsnark_hip.h")).read()
    assert re.search(r"\bint ps_groth16_prove_local\(", header) and "PS_G16_MULTI_HSPLIT" in header
    # no struct changed: the device struct is three handles and the key
    assert ctypes.sizeof(_lib.Groth16Device) == 3 * ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(_lib.Groth16Pk)


def test_refusals_before_any_device_work():
    """Argument errors are found on the host: no device is needed to see them."""
    from playsnark_amd import _lib, api

    lib = _lib.lib
    r = s = bytes(32)
    import ctypes as C

    bufs = [C.create_string_buffer(96), C.create_string_buffer(192), C.create_string_buffer(96)]
    assert lib.ps_groth16_prove_multi(None, 1, r, s, *bufs) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_prove_multi((_lib.Groth16Device * 1)(), 0, r, s, *bufs) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_prove_multi((_lib.Groth16Device * 65)(), 65, r, s, *bufs) == _lib.PS_ERR_ARG
    assert lib.ps_groth16_prove_multi((_lib.Groth16Device * 2)(), 2, r, s, *bufs) == _lib.PS_ERR_ARG  # NULL handles
    assert "NULL handle" in lib.ps_last_error().decode()
    pk = _lib.Groth16Pk()
    assert lib.ps_groth16_prove_local(None, None, None, None, r, s, 0, 1, *bufs) == _lib.PS_ERR_ARG
    assert "NULL argument" in lib.ps_last_error().decode()
    # rank / world are looked at before any handle is followed (the handles here are not real ones)
    fake = C.c_void_p(1)
    for rank, world in ((0, 0), (-1, 2), (2, 2), (0, -1)):
        assert lib.ps_groth16_prove_local(fake, C.byref(pk), fake, fake, r, s, rank, world, *bufs) == _lib.PS_ERR_ARG
        assert "bad rank / world" in lib.ps_last_error().decode()
    # ... and so is the form of the key: one without lxi / lxi2 / lxi_t is refused
    assert lib.ps_groth16_prove_local(fake, C.byref(pk), fake, fake, r, s, 0, 2, *bufs) == _lib.PS_ERR_ARG
    assert "lxi" in lib.ps_last_error().decode()
    with pytest.raises(api.PlaysnarkError):
        api.Groth16ProveMulti([], 1, 2)
    with pytest.raises(ValueError):  # a key with neither form complete
        api.Groth16Setup(b"", b"", b"", b"", b"", None, None, None, None)


def test_c_caller_compiles_links_and_fails_loudly_without_a_gpu(tmp_path):
    from playsnark_amd import api

    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if api.device_count() == 0:
        assert res.returncode == 77, res.stdout + res.stderr
        assert "no gfx950 device" in res.stdout
    else:
        assert res.returncode == 0, res.stdout + res.stderr


@pytest.mark.gpu
def test_c_caller_proves_the_toy_circuit_over_two_contexts(tmp_path):
    exe = _build_smoke(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ok" in res.stdout


def test_new_kernels_neither_spill_nor_use_scratch():
    """k_own_rows, k_own_rows_long and k_h_values_range in the shipped gfx950 code object (read as tests/test_code_object.py does)."""
    import shutil
    import tempfile

    from test_code_object import LIB, LLVM, kernel_notes

    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(LIB, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        co = [f for f in os.listdir(d) if f.endswith("gfx950")]
        assert len(co) == 1, os.listdir(d)
        notes = kernel_notes(os.path.join(d, co[0]))
    new = [n for n in notes if re.search(r"k_own_rows|k_h_values_range", n)]
    assert len(new) == 3, new
    for n in new:
        assert int(notes[n]["vgpr_spill_count"]) == 0 and int(notes[n].get("sgpr_spill_count", 0)) == 0, (n, notes[n])
        assert int(notes[n]["private_segment_fixed_size"]) == 0, (n, notes[n])
