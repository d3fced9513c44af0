"""CPU: the index arithmetic of the locating batch verifier's trees (playsnark_amd/csrc/locate_dev.hpp: level sizes and
offsets, the proofs a node covers, carried nodes) and its modular addition of plain words, compiled for the host under
ASan + UBSan by tests/host_locate_index.cpp and run over every tree size up to 1 100, the sizes at the caps, and descents
after marked leaves (the bound 1 + 2 b ceil(log2 N) on the tested nodes included).  The descent is the loop the library
ships, locate_bisect of playsnark_amd/csrc/locate_descent.hpp, with an oracle in place of the device's checks
(tests/host_locate_descent.hpp): also cut into passes of 1 and of 3 sets, and stopped by a check that returns an error."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_indices_and_descent_on_the_host(tmp_path):
    exe = str(tmp_path / "host_locate_index")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_locate_index.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "host_locate_index ok" in run.stdout
