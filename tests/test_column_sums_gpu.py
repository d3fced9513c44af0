"""GPU: ps_qap_column_sums -- out[i] = sum_j M[j][i] P[j] over points (csrc/ec_spmv.hpp) -- against the oracle's group
arithmetic, term by term (Mul per coefficient, Add per term), byte for byte.

The matrices are hand-built and need not be satisfiable (no witness is involved).  Shapes (gates, vars): (1, 1), (4, 6) (the
toy's), (65, 40), (600, 9); at (600, 9) one column has exactly 512 non-zeros (the last one a single thread sums), one 513 (the
first one a workgroup sums) and one all 600.  Coefficients come from {1, -1, 5, 2^62, 2^63 - 1, -2^63, random int64}."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = (1, -1, 5, 1 << 62, (1 << 63) - 1, -(1 << 63))


def _coef(rng):
    k = rng.next() % (len(EDGE) + 1)
    if k < len(EDGE):
        return EDGE[k]
    v = (rng.next() & ((1 << 64) - 1)) - (1 << 63)
    return v or 1


def _sign(rng):
    return 1 if rng.next() & 1 else -1


def _case_1x1(pr):
    # one gate, one variable: the largest magnitudes; O leaves the variable in no gate
    return 1, 1, [{0: [(0, (1 << 63) - 1)]}, {0: [(0, -(1 << 63))]}, {}], [0x1234567]


def _case_toy(pr):
    a = 0xABCDEF0123456789
    ks = [a, 0, a, pr.R - a]  # P0 = P2 (the same point twice), P1 the identity, P3 = -P0
    L = {
        0: [(0, 5), (2, 5)],                     # P + P inside every plane: the doubling branch of the mixed addition
        1: [(0, 1 << 62), (3, 1 << 62)],         # P + (-P), equal coefficients: the identity in the middle of a sum
        2: [(0, 1), (1, -1)],                    # an identity input
        # 3: in no gate
        4: [(0, 1), (2, 1), (3, 2)],             # a + a - 2a: cancels only with the last addition
        5: [(0, -(1 << 63)), (1, 5), (2, (1 << 63) - 1), (3, -1)],
    }
    R = {0: [(0, 0), (1, 7), (3, -5)],           # an explicit zero coefficient, and the identity as the only other early term
         2: [(2, (1 << 63) - 1), (3, (1 << 63) - 1)],
         5: [(1, 1)]}                            # the identity alone
    O = {i: [(i % 4, -(1 << 63))] for i in range(6)}
    return 4, 6, [L, R, O], ks


def _case_mid(pr):
    rng = pr.SplitMix64(65040)
    n, m = 65, 40
    ks = [0 if g % 11 == 3 else rng.fr() for g in range(n)]
    ks[20] = ks[10]
    ks[30] = pr.R - ks[10]
    mats = []
    for _ in range(3):
        cols = {}
        for g in range(n):
            for col in {rng.next() % (m - 1) for _ in range(1 + rng.next() % 3)}:  # (variable m - 1 stays in no gate)
                cols.setdefault(col, []).append((g, _coef(rng)))
        mats.append(cols)
    mats[0][7] = [(10, 5), (20, 5), (30, 5), (31, 1)]  # P, P again, -P with one coefficient, then an unrelated point
    return n, m, mats, ks


def _case_long(pr, unit_only):
    """(600, 9): columns of 512, 513 and 600 non-zeros in L; +-1 everywhere, and (unless unit_only) every seventh entry of
    the long columns drawn from the full set."""
    rng = pr.SplitMix64(6009)
    n, m = 600, 9
    ks = [0 if g % 97 == 5 else rng.fr() for g in range(n)]
    ks[300] = ks[100]
    ks[301] = pr.R - ks[100]

    def column(gates):
        return [(g, _sign(rng) if unit_only or i % 7 else _coef(rng)) for i, g in enumerate(gates)]

    L = {0: column(range(600)), 1: column(range(512)), 2: column(range(87, 600)),
         3: [(100, 1), (300, 1), (301, 2)], 5: column(range(0, 600, 50))}  # (3: a + a - 2a, cancels only in total; 4: in no gate)
    R = {0: column(range(513)), 6: column(range(3, 600, 40)), 8: [(599, -1)]}
    O = {7: column(range(600 - 512, 600)), 2: column(range(1, 600, 60))}
    assert [len(L[c]) for c in (0, 1, 2)] == [600, 512, 513] and len(R[0]) == 513 and len(O[7]) == 512
    return n, m, [L, R, O], ks


def _csr(n, cols):
    """column view {variable: [(gate, coefficient)]} -> (row_ptr, col, val) with rows = gates; explicit zeros are kept"""
    rows = [[] for _ in range(n)]
    for c in sorted(cols):
        for g, v in cols[c]:
            rows[g].append((c, v))
    row_ptr = np.zeros(n + 1, dtype=np.uint32)
    col, val = [], []
    for g, r in enumerate(rows):
        for c, v in r:
            col.append(c)
            val.append(v)
        row_ptr[g + 1] = len(col)
    return row_ptr, np.array(col, dtype=np.uint32), np.array(val, dtype=np.int64)


def _reference(G, prG, pts, entries, R):
    """sum of coefficient * point over the entries of one column: the oracle's Mul and Add, term by term"""
    acc = None
    for g, c in entries:
        p = pts[g]
        if p is None or c == 0:
            continue
        t = p if c == 1 else prG.neg(p) if c == -1 else G.mul(c % R, p)
        acc = t if acc is None else (acc if t is None else G.add(acc, t))
    return acc


CASES = {"1x1": lambda pr: _case_1x1(pr), "toy": lambda pr: _case_toy(pr), "65x40": lambda pr: _case_mid(pr),
         "600x9": lambda pr: _case_long(pr, False), "600x9-unit": lambda pr: _case_long(pr, True)}


@pytest.mark.parametrize("case,group", [("1x1", 1), ("toy", 1), ("65x40", 1), ("600x9", 1), ("1x1", 2), ("toy", 2), ("600x9-unit", 2)])
def test_column_sums_match_the_oracle(ps_api, ctx, co, pr, case, group):
    n, m, mats, ks = CASES[case](pr)
    G, prG = (co.G1, pr.G1) if group == 1 else (co.G2, pr.G2)
    q = ps_api.QAP.from_csr(ctx, m, 1, *[_csr(n, cols) for cols in mats])
    P = ps_api.Points.from_scalars(ctx, group, ps_api.Poly.upload(ctx, ks))
    pts = G.unpack(P.download())
    assert [p is None for p in pts] == [k == 0 for k in ks]
    for which, cols in enumerate(mats):
        got = q.column_sums(which, P)
        assert len(got) == m and got.group == group
        raw = got.download()
        for i in range(m):
            want = G.to_b(_reference(G, prG, pts, cols.get(i, []), pr.R))
            assert raw[i * G.nb : (i + 1) * G.nb] == want, (case, group, which, i, len(cols.get(i, [])))
    q.free()


def test_special_columns_of_the_toy_case_are_what_they_are_meant_to_be(ps_api, ctx, co, pr):
    """The cancellations of the hand-built case really happen: the identity bytes come back for P + (-P), for the column that
    cancels only in total, for the identity alone and for the variable in no gate."""
    n, m, mats, ks = _case_toy(pr)
    q = ps_api.QAP.from_csr(ctx, m, 1, *[_csr(n, cols) for cols in mats])
    for group, G in ((1, co.G1), (2, co.G2)):
        P = ps_api.Points.from_scalars(ctx, group, ps_api.Poly.upload(ctx, ks))
        ident = G.to_b(None)
        raw = q.column_sums(0, P).download()
        at = lambda i: raw[i * G.nb : (i + 1) * G.nb]
        assert at(1) == ident and at(3) == ident and at(4) == ident
        assert at(0) == G.to_b(G.mul(10 * ks[0] % pr.R)) and at(2) == G.to_b(G.mul(ks[0]))
        raw = q.column_sums(1, P).download()
        assert raw[5 * G.nb : 6 * G.nb] == ident and raw[1 * G.nb : 2 * G.nb] == ident
    q.free()


def test_wrong_number_of_points_is_a_length_mismatch(ps_api, ctx, pr):
    n, m, mats, ks = _case_toy(pr)
    q = ps_api.QAP.from_csr(ctx, m, 1, *[_csr(n, cols) for cols in mats])
    for cnt in (n - 1, n + 1):
        P = ps_api.Points.from_scalars(ctx, 1, ps_api.Poly.upload(ctx, list(range(1, cnt + 1))))
        with pytest.raises(ps_api.LengthMismatch):
            q.column_sums(0, P)
    with pytest.raises(ps_api.PlaysnarkError):
        q.column_sums(3, ps_api.Points.from_scalars(ctx, 1, ps_api.Poly.upload(ctx, ks)))
    q.free()
