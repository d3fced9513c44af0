"""The three kernels of the polynomial scan (ps_poly_eval, ps_poly_div_linear, ps_kzg_open) in the shipped gfx950 code object,
read without a GPU (as tests/test_code_object_batch.py does): every one of them is there, spills no register and uses no
scratch; the tile kernels use at most 128 registers, so that at least two workgroups of 256 threads fit a CU (128 registers
are four waves per SIMD, and a workgroup needs one wave on each).  Their register counts are recorded in DESIGN.md section 11,
not pinned here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")

# kernel -> number of instantiations in the object (k_poly_scan_tile: the totals and the apply pass)
KERNELS = {"k_poly_scan_tile": 2, "k_poly_scan_carries": 1}


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


def test_scan_kernels_are_shipped_and_use_no_spill_and_no_scratch(notes):
    for name, count in KERNELS.items():
        hits = _hits(notes, name)
        assert len(hits) == count, (name, [h["name"] for h in hits])
        for k in hits:
            assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
            assert int(k["private_segment_fixed_size"]) == 0, k
            assert k.get("uses_dynamic_stack", "false") == "false", k


def test_tile_kernels_leave_room_for_two_workgroups_per_cu(notes):
    for k in _hits(notes, "k_poly_scan_tile"):
        assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 128, k
        assert int(k["max_flat_workgroup_size"]) == 256, k
        assert 2 * int(k["group_segment_fixed_size"]) <= 160 * 1024, k  # and so does their LDS
