"""CPU: the buckets of a sum in order of size -- perm[] is a permutation in non-increasing size classes, and the verdict
word is what a direct computation gives.

The whole-bucket point pass (msm.hpp section 4b) hands bucket perm[t] to logical thread t and nothing clears the bucket
array, so every bucket must appear in perm[] exactly once.  tests/host_bucket_order.cpp compiles the index arithmetic the
ordering kernels are built from (playsnark_amd/csrc/bucket_order.hpp) for the host, under ASan + UBSan, and runs it in
their roles over generated offs[] arrays: all buckets empty, one entry in all, every bucket of size 1, sizes 0..300
mixed, one bucket holding everything, evenly filled sums with and without an outlier, bucket counts around the tile
size -- with the place kernel's workgroups reaching their cursors in three different orders."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_perm_is_a_permutation_in_size_order_and_the_verdict_is_direct(tmp_path):
    exe = str(tmp_path / "host_bucket_order")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_bucket_order.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "host_bucket_order ok" in run.stdout
