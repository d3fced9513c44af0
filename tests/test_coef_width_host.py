"""CPU: the coefficient classification of the column sums over points (playsnark_amd/csrc/coef_width.hpp: signed magnitude
min(v, r - v), its 64-bit words, narrow or wide, and the range test of ps_qap_create_fr), compiled for the host under
ASan + UBSan by tests/host_coef_width.cpp and compared with Python integers over the edge set, the int64 corners and a few
hundred seeded values."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_circuits as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = wc.R


def _inputs():
    from oracle import pyref as pr

    rng = pr.SplitMix64(0x636F6566)
    vals = list(wc.EDGE) + [0, 1, 1 << 63, (-(1 << 63)) % R, (1 << 63) - 1, (1 << 128) - 1, 1 << 128, R - (1 << 128), (1 << 192) + 7,
                            R - (1 << 192), (R - 1) // 2 - 1, (R + 1) // 2 + 1]
    for i in range(300):
        bits = 1 + rng.next() % 255  # every magnitude length, not just full-width values
        v = rng.fr() >> (255 - bits)
        vals.append(v if i % 2 else (R - v) % R)
    vals += [wc.coef(rng) for _ in range(60)]
    not_canonical = [R, R + 1, (1 << 256) - 1, 1 << 255]
    return vals, not_canonical


def test_classification_on_the_host(tmp_path):
    exe = str(tmp_path / "host_coef_width")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "host_coef_width.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    vals, bad = _inputs()
    assert all(0 <= v < R for v in vals)
    text = "".join("%064x\n" % v for v in vals + bad)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = run.stdout.split("\n")
    assert lines[-2:] == ["host_coef_width ok %d" % (len(vals) + len(bad)), ""]
    assert len(lines) == len(vals) + len(bad) + 2
    seen_words = set()
    for v, line in zip(vals, lines):
        mag, neg = wc.magnitude(v)
        assert mag == min(v, R - v) and neg == (v > (R - 1) // 2)
        words = (mag.bit_length() + 63) // 64
        seen_words.add(words)
        want = "1 %d %d %d %064x" % (neg, mag >= 1 << 64, words, mag)
        assert line == want, (hex(v), line, want)
        assert wc.is_wide(v) == (words > 1)
    assert seen_words == {0, 1, 2, 3, 4}
    for v, line in zip(bad, lines[len(vals):]):
        assert line == "0 0 0 0 " + "0" * 64, hex(v)


def test_the_edge_set_is_what_its_comments_say():
    wide = [wc.is_wide(v) for v in wc.EDGE]
    assert wide == [False, True, True, False, True, True, True, False, False, True, True]
    neg = [wc.magnitude(v)[1] for v in wc.EDGE]
    assert neg == [False, False, False, True, True, False, True, True, True, False, True]
    assert wc.magnitude(1 << 254) == (R - (1 << 254), True) and wc.magnitude((1 << 253) + 5) == ((1 << 253) + 5, False)
