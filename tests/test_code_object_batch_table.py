"""The two sort kernels of the tabled batch pass (k_sort_count_batch_tab, k_sort_partition_batch_tab; csrc/msm_batch.hpp) in
the shipped gfx950 code object, read without a GPU (as tests/test_code_object_batch.py does, from the notes of the code object
alone): each is there exactly once and spills no register, and each keeps at most 64 registers -- their workgroups have 1024
threads, sixteen waves, and two of them per CU (eight waves per SIMD) need that.  The counts are recorded in DESIGN.md
section 10."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")

KERNELS = ("k_sort_count_batch_tab", "k_sort_partition_batch_tab")


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


@pytest.mark.parametrize("name", KERNELS)
def test_tabled_sort_kernel_is_shipped_once_spills_nothing_and_keeps_64_registers(notes, name):
    hits = _hits(notes, name)
    assert len(hits) == 1, (name, [h["name"] for h in hits])
    (k,) = hits
    assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 64, k
    assert int(k["max_flat_workgroup_size"]) == 1024, k
