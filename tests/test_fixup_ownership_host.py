"""CPU: every bucket of a sum has exactly one writer and every partial slot of the accumulation exactly one reader.

The bucket array is never cleared, so the fix-up (msm.hpp section 5) is correct only if the accumulation's flush, the
classification, the pair kernel, the chain kernel and the heavy kernels share the buckets out without overlap or gap.
tests/host_fixup_ownership.cpp compiles the predicates those kernels are built from (playsnark_amd/csrc/fixup_class.hpp)
for the host, under ASan + UBSan, and runs them over generated offs[] arrays -- uniform fills, all-empty, one bucket
holding everything, buckets ending on slice boundaries, spans of 2, 3, 7, 8 and 9 slices, ragged and short lists -- with
effective slice lengths from 4 to 64."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_bucket_has_one_writer_and_every_slot_one_reader(tmp_path):
    exe = str(tmp_path / "host_fixup_ownership")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_fixup_ownership.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "host_fixup_ownership ok" in run.stdout
