"""CPU: the index arithmetic of the locating PHGR13 batch verifier (playsnark_amd/csrc/locate_phgr13_dev.hpp: which trees a
root mask needs, where the nodes of the level-major G1 trees and of the F tree lie, the host loops per equation), compiled
for the host under ASan + UBSan by tests/host_phgr13_locate_index.cpp -- its own main, no Python in the process -- and run
over every root mask, tree sizes 1 .. 70 and some larger ones with 1 .. 70 trees side by side, and descents with masks after
marked leaves (the bounds on checks and products included).  The descent is the loop the library ships, locate_bisect of
playsnark_amd/csrc/locate_descent.hpp, with an oracle in place of the device's checks (tests/host_locate_descent.hpp): also
cut into passes of 1 and of 3 sets, and stopped by a check that returns an error."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tree_layout_masks_and_descent_on_the_host(tmp_path):
    exe = str(tmp_path / "host_phgr13_locate_index")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_phgr13_locate_index.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "host_phgr13_locate_index ok" in run.stdout
