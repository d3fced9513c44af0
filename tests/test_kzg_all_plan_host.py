"""CPU: the index arithmetic of the openings at every node of the domain (playsnark_amd/csrc/kzg_all_plan.hpp), compiled for the
host under ASan + UBSan by tests/host_kzg_all_plan.cpp -- a stand-alone program; no Python code is loaded under a sanitizer.
The program checks p and S on both sides of every power of two up to 2^20, every offset of kappa written through its wrapped
index into a real array (inside [0, S), no two colliding, the way back agreeing), the convolution through those indices against
the literal Toeplitz sum and its sign under reversal, the buffer sizes and the limit n <= 2^30; the table it prints is derived
here a second time, in Python integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kzg_all_plan_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_kzg_all_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_kzg_all_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_kzg_all_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    want = sorted({n for k in range(21) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1) if n >= 1})
    assert [r[0] for r in rows] == want
    for n, p, S in rows:
        assert S == 1 << p and S >= 2 * n - 1 and (p == 0 or S // 2 < 2 * n - 1), n
        assert p == (2 * n - 2).bit_length(), n  # ceil(log2(2n - 1))
    by_n = {r[0]: r[1] for r in rows}
    assert by_n[1] == 0 and by_n[2] == 2 and by_n[256] == 9 and by_n[257] == 10 and by_n[4097] == 14 and by_n[1 << 16] == 17
    # the sizes the GPU test runs sit on both sides of a doubling
    for k in range(1, 21):
        assert by_n[(1 << k) + 1] == by_n[1 << k] + 1 == k + 2
