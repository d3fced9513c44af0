"""CPU: the scope type that owns every temporary of a library call (playsnark_amd/csrc/scope.hpp), compiled for the host under
ASan + UBSan by tests/host_scope.cpp against counting stand-ins for the HIP and handle calls it makes: each acquired thing
freed exactly once on every way out, one synchronisation before the first hipFree and none without scratch, reverse order,
results kept on success and released otherwise, the error text kept, slot addresses stable, failed allocations unrecorded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scope_on_the_host(tmp_path):
    exe = str(tmp_path / "host_scope")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_scope.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert run.stdout.split("\n")[-2:] == ["host_scope ok", ""]
    assert run.stderr == ""
