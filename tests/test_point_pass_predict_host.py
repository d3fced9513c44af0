"""CPU: the host's guess of the point pass an admitted sum will take (playsnark_amd/csrc/point_pass_predict.hpp), compiled
for the host under ASan + UBSan by tests/host_point_pass_predict.cpp.  The program drives sequences of (key, device verdict)
through the history as the library does -- predict at the launch, observe at the finish, one sum at a time and four in
flight -- and checks: the first sight of a key launches both families; a repeated verdict is predicted; a flip asks for a
redo, holds the key on both families for PP_HOLD launches and predicts again; an alternating stream pays one redo; another
key (array, table, offset, length, window, sets, width, group, sums over the sort) inherits nothing; eviction keeps the history at PP_SLOTS."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_point_pass_prediction_on_the_host(tmp_path):
    exe = str(tmp_path / "host_point_pass_predict")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_point_pass_predict.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    m = re.fullmatch(r"host_point_pass_predict ok \(hold (\d+), slots (\d+)\)\n", run.stdout)
    assert m, run.stdout
    # the hold covers at least one queue-full of sums (PS_MSM_QUEUE = 4), and a prover's arrays fit the history
    assert int(m.group(1)) >= 4 and int(m.group(2)) >= 7
