"""bench.py's host logic: the synthetic R1CS it proves in `extras` is the oracle's synthetic circuit, and
`python3 bench.py --gpus N` starts N ranks by itself (a driver-run SCALE record must never be a silent one-GPU
number).  CPU tests; the runs on a real GPU are gpu-marked."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_synthetic_r1cs_is_the_oracles_synthetic_circuit():
    from oracle import restate as rs

    bench = _bench()
    for n in (4, 8, 64, 1024):
        nvars, L, Rm, O, sol = bench.synthetic_r1cs(n)
        c, want_sol = rs.synthetic_circuit(n)
        assert nvars == c.nbVars and sol == want_sol
        for (ptr, col, val), rows in ((L, c.left), (Rm, c.right), (O, c.out)):
            got = [sorted((int(col[e]), int(val[e])) for e in range(ptr[g], ptr[g + 1])) for g in range(n)]
            assert got == [sorted(r) for r in rows]


def test_quotient_work_counts_match_design():
    bench = _bench()
    nbytes, bfly = bench.quotient_work(1 << 20)
    assert nbytes == 74 * (1 << 20) * 64            # 74 x 2^20 element-transforms, 2 x 32 B each
    assert bfly == 567 * (1 << 20)


def test_bench_starts_its_own_ranks(monkeypatch, capsys):
    """No WORLD_SIZE and --gpus 4: one child process of torch.distributed.run with --nproc-per-node=4, the
    caller's flags passed through, rank 0's JSON line relayed, other output sent to stderr."""
    bench = _bench()
    seen = {}

    class Done:
        returncode = 0
        stdout = 'noise from a rank\n{"metric": "G1 scalar-muls/s", "n_gpus": 4}\n'

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--total-log2n", "24"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--total-log2n", "24"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert json.loads(out.out.strip())["n_gpus"] == 4 and "noise from a rank" in out.err


def test_bench_refuses_a_world_that_differs_from_gpus(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE=2 but --gpus 8" in str(e.value.code)


def test_dlog_check_of_the_bench_line_against_pyref_and_published_multiples():
    """bench.py verifies every rank's partial sum and the folded result through sum_i k_i (a_i G) = (sum a_i k_i) G with a
    fixed-base multiplication of its own (plain integers).  That arithmetic against the Python twin, and against the
    published multiples 2 G1 = a572cbea..., 2 G2 = aa4edef9... (x coordinates of the Ethereum BLS public keys of secret key 2)."""
    import random

    from oracle import pyref as pr

    bench = _bench()
    rnd = random.Random(11)
    for s in (0, 1, 2, 3, pr.R - 1, pr.R, pr.R + 5) + tuple(rnd.randrange(pr.R) for _ in range(3)):
        assert bench.fixed_base_mul_bytes("g1", s) == pr.g1_to_bytes(pr.G1.mul(s % pr.R))
        assert bench.fixed_base_mul_bytes("g2", s) == pr.g2_to_bytes(pr.G2.mul(s % pr.R))
    assert bench.fixed_base_mul_bytes("g1", 2)[:48].hex() == (
        "0572cbea904d67468808c8eb50a9450c9721db309128012543902d0ac358a62ae28f75bb8f1c7c42c39a8c5529bf0f4e")
    assert bench.fixed_base_mul_bytes("g2", 2)[:8].hex() == "0a4edef9c1ed7f72"  # x_c1 first: the compressed form is aa4edef9...
    a = [rnd.randrange(pr.R) for _ in range(9)]
    k = [rnd.randrange(pr.R) for _ in range(9)]
    a_b = b"".join(x.to_bytes(32, "big") for x in a)
    assert bench.dlog_of_sum(a_b, b"".join(x.to_bytes(32, "big") for x in k)) == sum(x * y for x, y in zip(a, k)) % pr.R
    w = [5, -7, 0, 1, -(1 << 62), 9, 2, 3, 4]
    assert bench.dlog_of_sum(a_b, w) == sum(x * (y % pr.R) for x, y in zip(a, w)) % pr.R


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_on_one_gpu():
    """`python3 bench.py --gpus 2` as the driver types it (no torchrun around it): two ranks (gloo for the exchange,
    both on GPU 0), weak and strong scaling lines."""
    env = dict(os.environ, PS_BENCH_DEVICE="0", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1"]
    res = subprocess.run(base + ["--log2n", "14"], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["devices"] == [0, 0]
    assert line["config"]["points_per_gpu"] == 1 << 14 and line["value"] > 0 and "cpu_baseline" not in line
    assert line["verified"] is True and line["verified_dlog"] == {**line["verified_dlog"], "ranks": [True, True], "folded": True}
    res = subprocess.run(base + ["--total-log2n", "15"], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["points_per_gpu"] == 1 << 14
    assert "2^15 points in total" in line["config"]["workload"] and line["verified"] is True


@pytest.mark.gpu
def test_bench_many_ranks_rehearsal_verifies_every_share():
    """BASELINE config #4's shape on one device: 2^20 points in total over FOUR gloo ranks (VERDICT r3 asked for eight; a
    GPU box kills a command with more than six processes on its card, and this pytest process is one of them) and THREE
    (shards of unequal length).  Every rank's partial sum and the folded result are checked by discrete logarithm inside
    bench.py, so a multi-GPU line can no longer be an unverified number."""
    env = dict(os.environ, PS_BENCH_DEVICE="0", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    for ranks in (4, 3):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(ranks), "--backend", "gloo", "--steps", "3", "--warmup", "1",
               "--total-log2n", "20"]
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == ranks and line["scaling"] == "strong" and line["config"]["devices"] == [0] * ranks
        assert line["verified"] is True and line["verified_dlog"]["ranks"] == [True] * ranks and line["verified_dlog"]["folded"] is True


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--group", "g2", "--log2n", "12"], ["--group", "g1", "--log2n", "12", "--no-table"],
                                   ["--group", "g1", "--log2n", "12", "--scalars", "witness"]])
def test_bench_side_configurations_print_their_line(flags):
    """The configurations tools/size_sweep.sh and the secondary numbers drive (`--group g2` once died on a missing PMC
    record after the G2 file name had been dropped from the table): one JSON line, roofline present, traffic null where no
    PMC pass exists."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-extras", "--no-cpu-baseline", "--steps", "3", "--warmup", "1"] + flags
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["value"] > 0 and line["n_gpus"] == 1 and line["roofline"]["traffic"] is None
    assert line["unit"].startswith(flags[1].upper())


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps sums, prints the headline fields and none of the measurements that take
    runs of their own, and --dump-outputs writes the sum of the last timed step: byte for byte (sum a_i k_i mod r) G over the
    run's seeded inputs."""
    import numpy as np

    bench = _bench()
    n, steps = 1 << 12, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--log2n", "12", "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["unit"] == "G1 scalar-muls/s" and line["higher_is_better"] is True and line["dtype"] and line["metric"]
    assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - n) < 1e-6 * n  # value = n sums' worth of muls per ms_per_step
    assert not {"roofline", "stage_ms", "ms_per_step_one_at_a_time", "ms_per_step_with_h2d", "verified_dlog", "cpu_baseline",
                "extras"} & set(line)
    got = np.load(tmp_path / "out" / "result_affine.npy")
    assert got.dtype == np.float64 and got.shape == (96,)
    a = bench.uniform_scalars_be32(n, bench.SEED + 1000).tobytes()
    k = bench.uniform_scalars_be32(n, bench.SEED + 2000).tobytes()
    assert bytes(got.astype(np.uint8)) == bench.fixed_base_mul_bytes("g1", bench.dlog_of_sum(a, k))
