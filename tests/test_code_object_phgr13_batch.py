"""The kernels behind ps_msm_batch_multi and ps_phgr13_prove_batch in the shipped gfx950 code object, read without a GPU (as
tests/test_code_object_batch.py does).  The change adds no kernel of its own: the member stride is a runtime argument of
k_sort_count_batch, which must therefore still exist exactly once (no second instantiation, no template parameter), take the
extra 4-byte argument and spill nothing; every other kernel the two entries launch is shipped and spills nothing.  Register
counts are recorded in DESIGN.md section 10, not pinned here, but the sort kernel must keep the occupancy its 1024-thread
workgroups need (at most 64 registers: two workgroups per CU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")

# kernel -> number of instantiations in the object: the batch sort, the fold (G1, and G2 on lane pairs), the encoders, and the
# witness kernels the PHGR13 batch prover shares with the Groth16 one
KERNELS = {"k_sort_count_batch": 1, "k_sort_partition_batch": 1, "k_batch_fold": 2, "k_points_to_bytes_g1": 1, "k_points_to_bytes_g2": 1,
           "k_spmv_batch": 1, "k_spmv_long_rows_batch": 1, "k_check_gates_batch": 1, "k_fr_to_mont": 1, "k_fr_from_mont": 1}


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


def test_kernels_are_shipped_once_and_do_not_spill(notes):
    for name, count in KERNELS.items():
        hits = _hits(notes, name)
        assert len(hits) == count, (name, [h["name"] for h in hits])
        for k in hits:
            assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k


def test_the_stride_is_a_runtime_argument_of_the_one_sort_kernel(notes):
    """Itanium mangling of (const u32*, u32 n, u32 stride, u32 N, int c, int W, u32 NB, DigitConst, ...): three `j` in a row
    behind the pointer where the parent had two, and no template argument list."""
    (k,) = _hits(notes, "k_sort_count_batch")
    assert re.search(r"k_sort_count_batchEPKjjjjiij", k["name"]), k["name"]
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 64, k
