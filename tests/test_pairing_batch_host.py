"""CPU: the host-callable pieces of the batch verifier's kernels (playsnark_amd/csrc/pairing_dev.hpp) under
AddressSanitizer + UndefinedBehaviorSanitizer, lanes emulated by a loop (tests/host_pairing_batch_check.cpp), in the manner
of tests/test_host_sanitizers.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_helpers_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_pairing_batch_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                            os.path.join(ROOT, "tests", "host_pairing_batch_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    for line in ("f12_mul_mem == f12_mul", "product tree of 1000 worst-case factors == serial product", "spread_index covers every element exactly once",
                 "weighted column sums ok", "host_pairing_batch_check ok"):
        assert line in run.stdout
