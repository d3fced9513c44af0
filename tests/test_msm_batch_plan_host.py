"""CPU: the pass arithmetic of ps_msm_batch (playsnark_amd/csrc/msm_batch_plan.hpp: how many of a batch's K member sums run
as one sort / accumulation / tail, under the sort's bucket and offset limits, a byte cap, the reduction's grid limits and
ps_msm_batch_set_chunk), compiled for the host under ASan + UBSan by tests/host_msm_batch_plan.cpp and swept over n in
1..2^26, K in 1..2^16, c in 4..16.  The program checks every pass against the five limits and that the passes partition
0..K in order; the table of pass sizes it prints is derived here a second time, in Python integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(n, W, NB, pb, min_slice, chunk):
    """The largest Kc with Kc W NB <= 2^20, Kc n W < 2^31, Kc W <= 2^16, bytes <= 4 GiB and Kc <= chunk (0: no such limit)."""
    slices = -(-n * W // min_slice)
    kc = min((1 << 20) // (W * NB), ((1 << 31) - 1) // (n * W), (1 << 16) // W, (4 << 30) // ((W * NB + 2 * slices) * pb))
    return min(kc, chunk) if chunk else kc


def test_pass_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_msm_batch_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_msm_batch_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_msm_batch_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    assert len(rows) == 15 * 13 * 2 * 2 * 4
    seen_zero = seen_many = False
    for n, W, NB, pb, min_slice, chunk, kc in rows:
        assert kc == _members(n, W, NB, pb, min_slice, chunk), (n, W, NB, pb, chunk)
        seen_zero |= kc == 0
        seen_many |= kc > 1000
    assert seen_zero and seen_many
