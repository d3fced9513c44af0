"""The kernels of the openings at every node of the domain (ps_kzg_all_key_lagrange, ps_kzg_open_all_lagrange) in the shipped
gfx950 code object, read without a GPU (as tests/test_code_object_kzg_set_lagrange.py does): each of the five kernels of
kzg_all.hpp is there once, spills no register and uses no dynamic stack; the three scalar-side kernels use no scratch at all; the
two point kernels multiply by full-width scalars (ec_mul_fr, whose window table of eight points lives in private memory) and are
held to the scratch and the registers of k_ec_scale, the existing kernel that does one such multiplication per lane and nothing
else.  k_ec_scale<Fp> as the parent commit built it: 248 VGPRs and 3 360 B of scratch (eight XYZZ points of 224 B are 1 792 B;
the rest are the out-of-line additions' operands) -- the figures DESIGN.md section 11 quotes; the library under test must still
show them, so that the bound is the parent's and not one that moved with the build."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
SCALAR_KERNELS = ["k_kzg_all_kappa", "k_kzg_all_weights", "k_kzg_all_finish"]
POINT_KERNELS = ["k_kzg_all_load", "k_kzg_all_combine"]
EC_SCALE_PARENT = {"vgpr": 248, "scratch": 3360}  # k_ec_scale<Fp> at the parent commit


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


def _g1(hits):
    """the G1 instance of a kernel templated over the field"""
    return [k for k in hits if "INS_2FpE" in k["name"]]


@pytest.mark.parametrize("name", SCALAR_KERNELS + POINT_KERNELS)
def test_each_kernel_is_shipped_once(notes, name):
    assert len(_hits(notes, name)) == 1, [h["name"] for h in _hits(notes, name)]


@pytest.mark.parametrize("name", SCALAR_KERNELS + POINT_KERNELS)
def test_no_spill_and_no_dynamic_stack(notes, name):
    assert _hits(notes, name)
    for k in _hits(notes, name):
        print(name, "vgpr", k["vgpr_count"], "agpr", k["agpr_count"], "sgpr", k.get("sgpr_count"), "scratch", k["private_segment_fixed_size"],
              "lds", k["group_segment_fixed_size"])
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert k.get("uses_dynamic_stack", "false") == "false", k
        assert int(k["group_segment_fixed_size"]) == 0, k
        assert int(k["max_flat_workgroup_size"]) == 256, k


@pytest.mark.parametrize("name", SCALAR_KERNELS)
def test_the_scalar_side_uses_no_scratch(notes, name):
    for k in _hits(notes, name):
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= 128, k  # four waves per SIMD and more


def test_k_ec_scale_is_what_the_parent_commit_built(notes):
    (k,) = _g1(_hits(notes, "k_ec_scale"))
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) == EC_SCALE_PARENT["vgpr"], k
    assert int(k["private_segment_fixed_size"]) == EC_SCALE_PARENT["scratch"], k


@pytest.mark.parametrize("name", POINT_KERNELS)
def test_the_point_kernels_stay_within_k_ec_scale(notes, name):
    (k,) = _hits(notes, name)
    assert "INS_2FpE" in k["name"], k  # G1 only
    assert int(k["private_segment_fixed_size"]) <= EC_SCALE_PARENT["scratch"], k
    assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= EC_SCALE_PARENT["vgpr"], k  # two waves per SIMD need at most 256
