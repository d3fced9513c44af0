"""CPU: the index arithmetic of the value-form evaluation and quotient (playsnark_amd/csrc/poly_lagrange_plan.hpp), compiled for
the host under ASan + UBSan by tests/host_poly_lagrange_plan.cpp -- a stand-alone program; no Python code is loaded under a
sanitizer -- and swept over n around 1, T and 2T (each +- 1).  The program checks tiles, every (tile, thread, item) <-> node round
trip, the node lookup of on-domain points at both edges of every tile, row and partial offsets written through into real arrays,
the walk's chunks and reduction step, and the limits, against literal loops; the table it prints is derived here a second time,
in Python integers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    src = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_lagrange_plan.hpp")).read()
    return 256 << int(re.search(r"#else\s*\n\s*constexpr int POLY_LAGR_LOG_ITEMS\s*=\s*(\d+)\s*;", src).group(1))


def test_lagrange_plan_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_poly_lagrange_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_poly_lagrange_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_poly_lagrange_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    T = _tile()
    assert [r[0] for r in rows] == [1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
    for n, tiles, last, chunks in rows:
        assert tiles == -(-n // T) and last == n - (tiles - 1) * T and chunks == 1, n
    assert {r[2] for r in rows} >= {1, 2, T - 1, T}  # a tile of one node, a full one, and one node short of it
