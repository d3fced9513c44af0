"""The kernels of ps_msm_batch and ps_groth16_prove_batch in the shipped gfx950 code object, read without a GPU (as
tests/test_code_object.py does): every one of them is there and spills no register.  Their register counts are recorded in
DESIGN.md section 10, not pinned here.  k_batch_fold is bounded to two waves per SIMD (at most 256 registers), like the
tail kernels it runs behind; k_sort_partition_batch keeps its sixteen waves of at most 64 registers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")

# kernel -> number of instantiations in the object (k_batch_fold: G1, and G2 on lane pairs)
KERNELS = {"k_sort_count_batch": 1, "k_sort_partition_batch": 1, "k_batch_fold": 2, "k_spmv_batch": 1, "k_spmv_long_rows_batch": 1,
           "k_check_gates_batch": 1, "k_g16b_fill_ab": 1, "k_g16b_fill_c": 1}


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


def test_batch_kernels_are_shipped_and_do_not_spill(notes):
    for name, count in KERNELS.items():
        hits = _hits(notes, name)
        assert len(hits) == count, (name, [h["name"] for h in hits])
        for k in hits:
            assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k


def test_batch_kernels_keep_their_occupancy(notes):
    for k in _hits(notes, "k_batch_fold"):
        assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 256, k
    (k,) = _hits(notes, "k_sort_partition_batch")
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 64, k
