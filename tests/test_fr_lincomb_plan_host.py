"""CPU: the index arithmetic of ps_scalars_lincomb (playsnark_amd/csrc/fr_lincomb_plan.hpp), compiled for the host under
ASan + UBSan by tests/host_fr_lincomb_plan.cpp -- a stand-alone program; no Python code is loaded under a sanitizer -- and swept
over t = 1 .. 4R + 3, the launch edges 65 535 R - 1, 65 535 R, 65 535 R + 1, 2 * 65 535 R + 1 and 2^20.  The program checks row
groups, launches, workgroup counts, the table and output layout, the reduction step and the size limits against literal
loops; the table it prints is derived here a second time, in Python integers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows_per_group():
    src = open(os.path.join(ROOT, "playsnark_amd", "csrc", "fr_lincomb_plan.hpp")).read()
    return int(re.search(r"FR_LINCOMB_ROWS\s*=\s*(\d+)\s*;", src).group(1))


def test_lincomb_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_fr_lincomb_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_fr_lincomb_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_fr_lincomb_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    R = _rows_per_group()
    edge = 65535 * R
    assert [r[0] for r in rows] == list(range(1, 4 * R + 4)) + [edge - 1, edge, edge + 1, 2 * edge + 1, 2**20]
    for t, groups, last, launches in rows:
        assert groups == -(-t // R) and last == t - (groups - 1) * R and launches == -(-groups // 65535), t
    assert {1, 2, 3} <= {r[3] for r in rows}  # the second and third launch are met
    assert {r[2] for r in rows} == set(range(1, R + 1))  # and every length of a last group
