"""CPU: the index arithmetic of the set apply pass (playsnark_amd/csrc/poly_scan_set_plan.hpp), compiled for the host under
ASan + UBSan by tests/host_poly_scan_set_plan.cpp -- a stand-alone program; no Python code is loaded under a sanitizer -- and
swept over k = 1 .. 4G + 3 and 1024 with n in {1, k - 1, k, k + 1, T - 1 + k, T + k, T + k + 1, 2T + 1}, T = 2048.  The program
checks groups, the last group, the quotient length, the store predicate, buffer sizes, the reduction step and both limits
against literal loops; the table it prints is derived here a second time, in Python integers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2048


def _group():
    src = open(os.path.join(ROOT, "playsnark_amd", "csrc", "poly_scan_set_plan.hpp")).read()
    return int(re.search(r"POLY_SCAN_SET_GROUP\s*=\s*(\d+)\s*;", src).group(1))


def test_set_plan_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_poly_scan_set_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_poly_scan_set_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_poly_scan_set_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    G = _group()
    want = [(k, n) for k in list(range(1, 4 * G + 4)) + [1024]
            for n in (1, k - 1, k, k + 1, T - 1 + k, T + k, T + k + 1, 2 * T + 1) if n >= 1]
    assert [(r[0], r[1]) for r in rows] == want
    for k, n, groups, last, nq, stored in rows:
        assert groups == -(-k // G) and last == k - (groups - 1) * G, k
        assert nq == max(n - k, 0), (k, n)
        assert stored == sum(1 for i in range(1, n) if i - 1 < n - k) if n <= 64 else stored == nq, (k, n)
    assert {r[3] for r in rows} == set(range(1, G + 1))  # every length of a last group
    assert {r[4] for r in rows} >= {0, 1, T - 1, T, T + 1}  # the empty quotient, one coefficient, and the cut on a tile's edge
    assert {(r[4] % 8) for r in rows} == set(range(8))  # ... on a thread's edge and inside a thread's items
