"""The shipped gfx950 code object, read without a GPU: the whole-bucket point pass (msm.hpp section 4b, k_bucket_sum) runs
two waves per SIMD without spilling and holds ONE inlined copy of the mixed addition -- a second copy (a peeled first
trip, say) would be ~42 KB more ISA against a 64 KB instruction cache."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")

MADD_MADS_G1 = 3542  # 64-bit multiply-adds of one G1 mixed addition per lane


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or LLVM tools not present")
    d = tmp_path_factory.mktemp("co")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    co = [f for f in os.listdir(d) if f.endswith("gfx950")]
    assert len(co) == 1, os.listdir(d)
    return str(d / co[0])


def kernel_notes(co):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
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


def _g1(names):
    g1 = [n for n in names if "k_bucket_sum" in n and "Fp2s" not in n]
    assert len(g1) == 1, g1
    return g1[0]


def test_g1_bucket_sum_fits_two_waves_per_simd_without_spilling(code_object):
    notes = kernel_notes(code_object)
    assert len([n for n in notes if "k_bucket_sum" in n]) == 2, [n for n in notes if "k_bucket_sum" in n]  # G1 and the lane-pair G2
    n = notes[_g1(notes)]
    assert int(n["vgpr_spill_count"]) == 0, n
    assert int(n["vgpr_count"]) + int(n["agpr_count"]) <= 256, n


def test_g2_bucket_sum_spills_no_more_than_the_slice_kernel(code_object):
    notes = kernel_notes(code_object)
    new = [n for n in notes if "k_bucket_sum" in n and "Fp2s" in n]
    old = [n for n in notes if "k_accumulate" in n and "Fp2s" in n]
    assert len(new) == 1 and len(old) == 1, (new, old)
    assert int(notes[new[0]]["vgpr_spill_count"]) <= int(notes[old[0]]["vgpr_spill_count"]), (notes[new[0]], notes[old[0]])


def test_g1_bucket_sum_holds_one_copy_of_the_mixed_addition(code_object):
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", code_object], check=True, capture_output=True, text=True).stdout
    bodies = {}
    name = None
    for line in asm.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            bodies[name] = 0
        elif name and "v_mad_" in line and "64" in line:
            bodies[name] += 1
    c = bodies[_g1(bodies)]
    assert 3500 <= c <= 2 * MADD_MADS_G1, c
