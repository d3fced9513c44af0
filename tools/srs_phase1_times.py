"""Wall time of the phase-1 calls on one device: ps_groth16_srs_contribute, ps_groth16_srs_check, ps_groth16_srs_check_update
for a string of 2^k gates (2^(k+1) - 1, 2^k, 2^k, 2^k points), once each after a warm-up at 2^8 gates that pays for the first
launches.  With --setup the circuit's key is derived from the contributed string as well (ps_groth16_setup_from_srs on the
synthetic circuit), the call the phase-1 times are to be read beside.

    python tools/srs_phase1_times.py --log-gates 16 [--setup] > profiles/srs_phase1_times.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from playsnark_amd import api  # noqa: E402

R = api.R_ORDER


def timed(ctx, f):
    ctx.sync()
    t0 = time.perf_counter()
    out = f()
    ctx.sync()
    return out, time.perf_counter() - t0


def clear_string(ctx, n, x, alpha, beta):
    """A string from values held in the clear (a measurement may; a ceremony starts from Groth16SRS.initial)"""
    tau = api.Poly.powers(ctx, x, 2 * n - 1)
    g2 = api.Points.from_scalars(ctx, api.G2, api.Poly.upload(ctx, [beta]))
    return api.Groth16SRS(api.Points.from_scalars(ctx, api.G1, tau), api.Points.from_scalars(ctx, api.G2, tau.slice(0, n)),
                          api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, alpha)),
                          api.Points.from_scalars(ctx, api.G1, api.Poly.powers(ctx, x, n, beta)), g2.download())


def run(ctx, n, label, setup):
    state = 0x9E3779B97F4A7C15

    def draw():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) % 2**64
        return state

    fr = lambda: (draw() << 192 | draw() << 128 | draw() << 64 | draw()) % R or 1
    s0 = clear_string(ctx, n, fr(), fr(), fr())
    rhos = [(draw() << 64 | draw()) or 1 for _ in range(2 * n - 2)]
    (s1, share), t_con = timed(ctx, lambda: api.Groth16SRSContribute(ctx, s0, fr(), fr(), fr()))
    ok, t_chk = timed(ctx, lambda: api.Groth16SRSCheck(ctx, s1, rhos))
    assert ok
    ok, t_raw = timed(ctx, lambda: api.Groth16SRSCheck(ctx, s1, rhos, check_subgroup=False))
    assert ok
    ok, t_upd = timed(ctx, lambda: api.Groth16SRSCheckUpdate(ctx, s0, s1, share, rhos))
    assert ok
    print(f"{label} gates={n} points={4 * n - 1}G1+{n}G2  contribute {t_con * 1e3:.1f} ms  check {t_chk * 1e3:.1f} ms  "
          f"(without subgroup tests {t_raw * 1e3:.1f} ms)  check_update {t_upd * 1e3:.1f} ms", flush=True)
    if setup:
        from oracle import restate as rs

        c, _ = rs.synthetic_circuit(n)
        q = api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
        _, t_set = timed(ctx, lambda: api.NewGroth16SetupFromSRS(q, s1))
        print(f"{label} gates={n}  setup_from_srs {t_set * 1e3:.1f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gates", type=int, default=16)
    ap.add_argument("--setup", action="store_true")
    a = ap.parse_args()
    ctx = api.Context(0)
    run(ctx, 1 << 8, "warm-up", False)
    run(ctx, 1 << a.log_gates, "measured", a.setup)


if __name__ == "__main__":
    main()
