"""CPU: the index arithmetic of the value-form set quotient (playsnark_amd/csrc/poly_lagrange_set_plan.hpp), compiled for the
host under ASan + UBSan by tests/host_poly_lagrange_set_plan.cpp -- a stand-alone program; no Python code is loaded under a
sanitizer -- and swept over n around 1, T and 2T and k around 1, G and 2G (each +- 1).  The program checks the groups, every
(tile, group, thread, item, number) <-> (node, point) round trip, the partial rows, the weights and the LDS slots written through
into real arrays, and the limits, against literal loops; the table it prints is derived here a second time, in Python integers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(header, name):
    src = open(os.path.join(ROOT, "playsnark_amd", "csrc", header)).read()
    return int(re.search(r"#else\s*\n\s*constexpr int %s\s*=\s*(\d+)\s*;" % name, src).group(1))


def test_lagrange_set_plan_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_poly_lagrange_set_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_poly_lagrange_set_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_poly_lagrange_set_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    T = 256 << _const("poly_lagrange_plan.hpp", "POLY_LAGR_LOG_ITEMS")
    G = _const("poly_lagrange_set_plan.hpp", "POLY_LAGR_SET_GROUP")
    ks = [k for k in (1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1) if k >= 1]
    assert [(r[0], r[1]) for r in rows] == [(n, k) for n in (1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1) for k in ks]
    for n, k, groups, last, partial_rows in rows:
        assert groups == -(-k // G) and last == k - (groups - 1) * G, (n, k)
        assert partial_rows == (groups if groups > 1 else 0), (n, k)
    assert {r[3] for r in rows} >= {1, G}  # a group of one point and a full one
