"""CPU: the index arithmetic of the polynomial scan (playsnark_amd/csrc/poly_scan_plan.hpp), compiled for the host under
ASan + UBSan by tests/host_poly_scan_plan.cpp -- a stand-alone program; no Python code is loaded under a sanitizer -- and swept
over n = 1 .. 3T + 2, the chunk edges 256 T - 1, 256 T, 256 T + 1, 2 * 256 T + 1 and 2^32 - 1.  The program checks tile and
chunk counts, every tile's length, the exponent of every carry and how the kernels compose it, buffer sizes and the k * n
bound against literal loops; the table it prints is derived here a second time, in Python integers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    src = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_scan_plan.hpp")).read()
    log_items = int(re.search(r"POLY_SCAN_LOG_ITEMS\s*=\s*(\d+)\s*;", src).group(1))
    return 256 << log_items


def test_scan_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_poly_scan_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_poly_scan_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_poly_scan_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    T = _tile()
    from playsnark_amd import _lib

    assert T == _lib.lib.ps_poly_scan_tile()  # the shipped library was built from this header
    edge = 256 * T
    assert [r[0] for r in rows] == list(range(1, 3 * T + 3)) + [edge - 1, edge, edge + 1, 2 * edge + 1, 2**32 - 1]
    for n, tiles, last, chunks in rows:
        assert tiles == -(-n // T) and last == n - (tiles - 1) * T and chunks == -(-tiles // 256), n
    assert {r[3] for r in rows} == {1, 2, 3, 2**21 // 256}  # the second and third chunk of the carry walk are met
