"""The batch verifier's kernels in the shipped gfx950 code object, read without a GPU (as tests/test_code_object.py does).

k_f12_product and k_fr_weighted_columns spill nothing.  k_miller_batch -- one Miller loop per lane, the tower inlined over
Fp2 values in registers -- does NOT fit the 512 registers of one wave per SIMD: f (168 registers), the running point (84),
the pair (84) and the temporaries of f12_sqr / f12_mul_line are alive together, and the compiler spills 1 204 registers
(2 624 bytes of scratch per lane) inside the 63-step loop.  That is what ships and what is pinned here, as an upper bound,
so that a regression is seen and an improvement is not refused (csrc/pairing_dev.hpp)."""
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


def _one(notes, name):
    hit = [k for k in notes if name in k]
    assert len(hit) == 1, (name, hit)
    return notes[hit[0]]


def test_product_and_column_kernels_do_not_spill(notes):
    for name in ("k_f12_product", "k_fr_weighted_columns"):
        assert int(_one(notes, name)["vgpr_spill_count"]) == 0, (name, _one(notes, name))
    assert int(_one(notes, "k_fr_weighted_columns")["private_segment_fixed_size"]) == 0
    # k_f12_product: the frame of its out-of-line Fp products, nothing spilled; and registers for two waves per SIMD
    k = _one(notes, "k_f12_product")
    assert int(k["private_segment_fixed_size"]) <= 176, k
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 256, k


def test_miller_kernel_is_what_was_measured(notes):
    """Pinned from the shipped object: PINNED below.  The allocation is exact (it decides the occupancy: one wave per
    SIMD); spills and scratch are upper bounds, so that an improvement is not refused."""
    k = _one(notes, "k_miller_batch")
    assert (int(k["vgpr_count"]), int(k["agpr_count"])) == PINNED["alloc"], k
    assert int(k["vgpr_spill_count"]) <= PINNED["spills"], k
    assert int(k["private_segment_fixed_size"]) <= PINNED["scratch"], k


PINNED = {"alloc": (512, 256), "spills": 1204, "scratch": 2624}
