"""CPU: the index arithmetic of the range-sharded provers (playsnark_amd/csrc/share_ranges.hpp: a rank's range of an array,
and its pieces of a sum of several segments with a few fixed entries behind them), compiled for the host under ASan + UBSan
by tests/host_share_ranges.cpp and run for every length up to 70 over 1 to 9 ranks; the table of ranges it prints is
playsnark_amd.dist.shard_range's, entry by entry."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranges_and_pieces_on_the_host(tmp_path):
    from playsnark_amd.dist import shard_range

    exe = str(tmp_path / "host_share_ranges")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_share_ranges.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_share_ranges ok", ""]
    table = {}
    for line in lines[:-2]:
        n, world, rank, first, cnt = map(int, line.split())
        assert (n, world, rank) not in table
        table[n, world, rank] = (first, cnt)
    want = {(n, world, rank): shard_range(n, rank, world) for n in range(71) for world in range(1, 10) for rank in range(world)}
    assert table == want
