"""The set apply pass of ps_poly_div_roots / ps_kzg_open_set in the shipped gfx950 code object, read without a GPU (as
tests/test_code_object_kzg_multi.py does): k_poly_scan_set_apply is there once, spills no register, uses no scratch and no
dynamic stack -- its eight 10-limb accumulators stay in registers -- fits the 256 registers a workgroup of 256 threads may
have, keeps the scan's 20 480 B of LDS, and the kernels it runs beside are what they were.  Bounds, not pinned counts: the
counts of the build are recorded in DESIGN.md section 11."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    assert os.path.exists(LIB), "the library has not been built"
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "LLVM tools of ROCm not present"
    d = tmp_path_factory.mktemp("co")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    co = [f for f in os.listdir(d) if f.endswith("gfx950")]
    assert len(co) == 1, os.listdir(d)
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / co[0])], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count" and cur.get("name"):
            kernels[cur["name"]] = cur
            cur = {}
        cur[key] = val
    if cur.get("name"):
        kernels[cur["name"]] = cur
    return kernels


def _hits(notes, name):
    return [v for k, v in notes.items() if re.search(r"\d%s(E|I)" % name, k)]


def test_set_apply_kernel_is_shipped_once_and_uses_no_spill_no_scratch_no_dynamic_stack(notes):
    hits = _hits(notes, "k_poly_scan_set_apply")
    assert len(hits) == 1, [h["name"] for h in hits]
    k = hits[0]
    assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
    assert int(k["private_segment_fixed_size"]) == 0, k
    assert k.get("uses_dynamic_stack", "false") == "false", k


def test_set_apply_kernel_fits_256_registers_at_256_threads_with_the_scans_lds(notes):
    (k,) = _hits(notes, "k_poly_scan_set_apply")
    print("k_poly_scan_set_apply: vgpr", k["vgpr_count"], "agpr", k["agpr_count"], "sgpr", k.get("sgpr_count"), "lds", k["group_segment_fixed_size"])
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 256, k
    assert int(k["max_flat_workgroup_size"]) == 256, k
    assert int(k["group_segment_fixed_size"]) == 20480, k


def test_the_scan_kernels_are_still_two_tile_instantiations_and_one_carry_walk(notes):
    """The set pass is a kernel of its own name: totals and carry walk are reused as they are."""
    assert len(_hits(notes, "k_poly_scan_tile")) == 2 and len(_hits(notes, "k_poly_scan_carries")) == 1


def test_the_fold_of_partial_rows_added_no_second_lincomb_kernel(notes):
    assert len(_hits(notes, "k_fr_lincomb")) == 1
