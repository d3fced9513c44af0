"""CPU: the pass arithmetic of the tabled batch pass (playsnark_amd/csrc/msm_batch_plan.hpp with BatchShape::table set: a
member has n * W entries but ONE bucket set of NB buckets), compiled for the host under ASan + UBSan by
tests/host_msm_batch_table_plan.cpp and swept over n in 1..2^26 - 1, K in 1..2^16 and the table windows 8, 9, 10, 13, 16, 20.
The program checks every pass against the five tabled limits, that the passes partition 0..K in order, and that the
five-value BatchShape initialiser still yields the plain pass sizes; the table of pass sizes it prints is derived here a
second time, in Python integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(n, W, NB, pb, min_slice, chunk, tabled):
    """The largest Kc with Kc * buckets <= 2^20, Kc n W < 2^31, Kc * sets <= 2^16, bytes <= 4 GiB and Kc <= chunk (0: no such
    limit), where a member has (NB buckets, 1 set) over a table and (W NB, W) on the plain plan."""
    buckets, sets = (NB, 1) if tabled else (W * NB, W)
    slices = -(-n * W // min_slice)
    kc = min((1 << 20) // buckets, ((1 << 31) - 1) // (n * W), (1 << 16) // sets, (4 << 30) // ((buckets + 2 * slices) * pb))
    return min(kc, chunk) if chunk else kc


def test_tabled_pass_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_msm_batch_table_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_msm_batch_table_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_msm_batch_table_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    assert len(rows) == 16 * 6 * 2 * 2 * 4
    seen_zero = seen_many = seen_wider = False
    for n, W, NB, pb, min_slice, chunk, kc, kp in rows:
        assert kc == _members(n, W, NB, pb, min_slice, chunk, True), (n, W, NB, pb, chunk)
        assert kp == _members(n, W, NB, pb, min_slice, chunk, False), (n, W, NB, pb, chunk)
        seen_zero |= kc == 0
        seen_many |= kc > 1000
        seen_wider |= kc > kp
    assert seen_zero and seen_many and seen_wider
