"""CPU: the pass arithmetic of ps_msm_batch_multi (playsnark_amd/csrc/msm_batch_multi_plan.hpp: the passes of ps_msm_batch
under the point size of the largest group present and under the member stride, which bounds the 32-bit scalar index of
k_sort_count_batch), compiled for the host under ASan + UBSan by tests/host_msm_batch_multi_plan.cpp and swept over n in
1..2^26, c in 4..16, the three group mixes and strides from n to 2^33.  The program checks every pass against the limits in
128-bit arithmetic and that a packed batch gets exactly the passes of ps_msm_batch; the table of pass sizes it prints is
derived here a second time, in Python integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _members(n, W, NB, pb, chunk, stride):
    """The largest Kc with Kc W NB <= 2^20, Kc n W < 2^31, Kc W <= 2^16, bytes <= 4 GiB, Kc <= chunk (0: no such limit) and
    (Kc - 1) stride + n - 1 < 2^32."""
    slices = -(-n * W // 2)
    kc = min((1 << 20) // (W * NB), ((1 << 31) - 1) // (n * W), (1 << 16) // W, (4 << 30) // ((W * NB + 2 * slices) * pb))
    kc = min(kc, chunk) if chunk else kc
    if kc == 0:
        return 0
    return min(kc, ((1 << 32) - n) // stride + 1)


def test_pass_arithmetic_on_the_host(tmp_path):
    exe = str(tmp_path / "host_msm_batch_multi_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_msm_batch_multi_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_msm_batch_multi_plan ok", ""]
    rows = [tuple(map(int, ln.split())) for ln in lines[:-2]]
    assert len(rows) >= 15 * 13 * 2 * 3 * 2 * 4  # at least four of the six strides are >= n for every n
    seen_zero = seen_many = seen_stride = False
    for n, W, NB, pb, chunk, stride, kc in rows:
        assert stride >= n
        assert kc == _members(n, W, NB, pb, chunk, stride), (n, W, NB, pb, chunk, stride)
        seen_zero |= kc == 0
        seen_many |= kc > 1000
        seen_stride |= 0 < kc < _members(n, W, NB, pb, chunk, n)
    assert seen_zero and seen_many and seen_stride
