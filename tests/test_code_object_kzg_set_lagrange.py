"""The kernel of the value-form set openings (ps_poly_div_roots_lagrange, ps_kzg_open_set_lagrange) in the shipped gfx950 code
object, read without a GPU (as tests/test_code_object_kzg_lagrange.py does): k_lagr_fold is there once, spills no register, uses
no scratch and no dynamic stack, keeps its LDS static and within the 64 KB a workgroup may have, and stays within the figures
DESIGN.md section 11 quotes for this build, as upper bounds: 200 VGPRs (two waves per SIMD need at most 256) and 61 480 B of LDS
(two workgroups per CU need at most 80 KB each).  The sum of the partial rows is k_fr_lincomb, which tests/test_code_object_kzg_multi.py
covers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "playsnark_amd", "libplaysnark_hip.so")
LDS_MAX = 64 * 1024
VGPR_CEILING = {"k_lagr_fold": 200}
LDS_CEILING = {"k_lagr_fold": 61480}


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


def test_the_fold_kernel_is_shipped_once(notes):
    assert len(_hits(notes, "k_lagr_fold")) == 1, [h["name"] for h in _hits(notes, "k_lagr_fold")]


@pytest.mark.parametrize("name", sorted(VGPR_CEILING))
def test_no_spill_no_scratch_no_dynamic_stack(notes, name):
    assert _hits(notes, name)
    for k in _hits(notes, name):
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert k.get("uses_dynamic_stack", "false") == "false", k


@pytest.mark.parametrize("name", sorted(VGPR_CEILING))
def test_static_lds_and_registers_within_the_figures_the_design_quotes(notes, name):
    assert _hits(notes, name)
    for k in _hits(notes, name):
        print(name, "vgpr", k["vgpr_count"], "agpr", k["agpr_count"], "sgpr", k.get("sgpr_count"), "lds", k["group_segment_fixed_size"])
        assert int(k["group_segment_fixed_size"]) <= LDS_CEILING[name] <= LDS_MAX, k
        assert int(k["vgpr_count"]) + int(k["agpr_count"]) <= VGPR_CEILING[name], k
        assert int(k["max_flat_workgroup_size"]) == 256, k
