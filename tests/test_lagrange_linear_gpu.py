"""ps_points_monomial_to_lagrange as what it is: a linear map on arrays of subgroup points.

For the input P_i = s_i G the output must be L_j = (sum_i c_{j,i} s_i) G, where l_j(X) = sum_i c_{j,i} X^i is the Lagrange
basis on the nodes (1..n for nodes = 0; the n-1 nodes n+1..2n-1 for nodes = 1).  The other tests of the conversion feed it
{x^i P} for a random x: all points distinct, none the identity, no butterfly P +- wQ of k_ec_ntt_stage and no step
T[i+1] - c_k T[i] of k_ec_base_step that ever degenerates.  The structured inputs here put identity, doubling and
cancellation operands into those kernels (and into k_ec_scale, k_ec_take_right, k_ec_pad and the closing
k_batch_to_affine) at every level: all points the identity, one real point among identities, all points equal, the "secret
point" equal to an interpolation node (the output is G at that node and the identity everywhere else), G, -G, G, ...

Reference: c_{j,.} in Fr with Python integers -- the master polynomial M divided by X - node_j and scaled by 1 / M'(node_j),
O(n^2) in all --, the sums reduced mod r, and the points, input and expected output alike, from the C oracle's Mul.
Sizes: n = 4 (no tree level), 68 (np = 128, one level), 200 (np = 256, two levels)."""
import pytest

pytestmark = pytest.mark.gpu

SIZES = [4, 68, 200]
FAMILIES = ["zero", "e_first", "e_last", "all_equal", "node_power_lo", "node_power_mid", "node_power_hi", "minus_one_powers",
            "half_zero", "pairs_cancel", "random"]
KEPT_AT_200_G2 = ("node_power_lo", "node_power_mid", "node_power_hi", "all_equal", "random")


def _nodes(n, nodes):
    return list(range(1, n + 1)) if nodes == 0 else list(range(n + 1, 2 * n))


def _basis(R, xs):
    """c[j][i]: coefficient of X^i in the Lagrange basis polynomial l_j on the nodes xs"""
    m = [1]  # the master polynomial, lowest degree first
    for x in xs:
        m = [((m[i - 1] if i else 0) - x * (m[i] if i < len(m) else 0)) % R for i in range(len(m) + 1)]
    out = []
    for x in xs:
        q = [0] * len(xs)  # M / (X - x) by synthetic division from the top
        carry = 0
        for i in range(len(xs), 0, -1):
            carry = (m[i] + carry * x) % R
            q[i - 1] = carry
        at = 0
        for c in reversed(q):
            at = (at * x + c) % R
        inv = pow(at, R - 2, R)
        out.append([c * inv % R for c in q])
    return out


def _family(pr, rng, name, n, nodes, cnt):
    """the scalars s_0 .. s_{cnt-1} of one family"""
    R = pr.R
    if name == "zero":
        return [0] * cnt
    if name == "e_first":
        return [1] + [0] * (cnt - 1)
    if name == "e_last":
        return [0] * (cnt - 1) + [1]
    if name == "all_equal":
        return [rng.fr()] * cnt
    if name.startswith("node_power"):
        k = {0: {"lo": 1, "mid": 2, "hi": n}, 1: {"lo": n + 1, "hi": 2 * n - 1}}[nodes][name.rsplit("_", 1)[1]]
        return [pow(k, i, R) for i in range(cnt)]
    if name == "minus_one_powers":
        return [1 if i % 2 == 0 else R - 1 for i in range(cnt)]
    if name == "half_zero":
        return [rng.fr() if i < cnt // 2 else 0 for i in range(cnt)]
    if name == "pairs_cancel":
        s = rng.fr()
        return [s if i % 2 == 0 else R - s for i in range(cnt)]
    return [rng.fr() for _ in range(cnt)]


@pytest.fixture(scope="module")
def env(ps_api, ctx, co, pr):
    """per n: the circuit on the device; per (n, nodes): the basis; per (group, scalar): the oracle's k G.  Made on first use."""
    from oracle import restate as rs

    qaps, bases, muls = {}, {}, {}

    def qap(n):
        if n not in qaps:
            c = rs.toy_circuit()[0] if n == 4 else rs.synthetic_circuit(n)[0]
            assert c.nbGates == n
            qaps[n] = ps_api.QAP(ctx, c.nbVars, c.nbIO, c.left, c.right, c.out)
        return qaps[n]

    def basis(n, nodes):
        if (n, nodes) not in bases:
            xs = _nodes(n, nodes)
            c = _basis(pr.R, xs)
            for j in (0, len(xs) - 1):  # l_j(node_k) = [j == k], on the rows at both ends
                for k, x in enumerate(xs):
                    assert sum(cj * pow(x, i, pr.R) for i, cj in enumerate(c[j])) % pr.R == (j == k)
            bases[n, nodes] = c
        return bases[n, nodes]

    def mul(group, k):
        if (group, k) not in muls:
            og = getattr(co, group)
            muls[group, k] = og.to_b(og.mul(k) if k else None)
        return muls[group, k]

    return qap, basis, mul


def _cases():
    """every size, node set, group and family -- but three kinds of input at the largest size over G2 (node powers, all equal,
    the control), and no third node power on the nodes n+1..2n-1, which are taken at both ends"""
    for n in SIZES:
        for nodes in (0, 1):
            for group in ("G1", "G2"):
                for family in FAMILIES:
                    if n == 200 and group == "G2" and family not in KEPT_AT_200_G2:
                        continue
                    if nodes == 1 and family == "node_power_mid":
                        continue
                    yield pytest.param(n, nodes, group, family, id="n%d-nodes%d-%s-%s" % (n, nodes, group, family))


@pytest.mark.parametrize("n,nodes,group,family", list(_cases()))
def test_conversion_is_the_linear_map_of_the_lagrange_basis(ps_api, ctx, co, pr, env, n, nodes, group, family):
    qap, basis, mul = env
    R = pr.R
    cnt = n if nodes == 0 else n - 1
    rng = pr.SplitMix64(0x1A6 + 1000 * n + 10 * nodes + FAMILIES.index(family))
    s = _family(pr, rng, family, n, nodes, cnt)
    assert len(s) == cnt
    c = basis(n, nodes)
    want_k = [sum(cji * si for cji, si in zip(cj, s)) % R for cj in c]
    if family.startswith("node_power"):  # the secret point is a node: G there, the identity everywhere else
        assert want_k == [int(x == s[1]) for x in _nodes(n, nodes)]  # s[1] is the node itself
    if family == "zero":
        assert not any(want_k)
    og = getattr(co, group)
    gid = ps_api.G1 if group == "G1" else ps_api.G2
    mono = ps_api.Points.upload(ctx, gid, b"".join(mul(group, k) for k in s))
    got = mono.to_lagrange(qap(n), nodes).download()
    assert len(got) == cnt * og.nb
    bad = [j for j in range(cnt) if got[j * og.nb:(j + 1) * og.nb] != mul(group, want_k[j])]
    assert not bad, (bad[:20], len(bad))
