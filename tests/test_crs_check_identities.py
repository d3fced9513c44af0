"""CPU: the equations of ps_groth16_crs_check_from_srs and ps_points_lagrange_check in the exponent, in Python integers.

Every group element is replaced by its discrete logarithm -- T1[i] = x^i, A[i] = alpha x^i, B[i] = beta x^i, the key's scalars
as restate.groth16_setup computes them from the toxic waste -- and a pairing e(P, Q) by the product of the two logarithms.  This
pins the index conventions the device code follows: which weights go with which array, the node sets 1..n and n+1..2n-1, the
length of rho * z, and the split of the variables at diff = nbVars - nbIO.  n = 4 (the toy circuit) and n = 5."""
import pytest

SIZES = (4, 5)


def _toxic(pr):
    rng = pr.SplitMix64(20161016)
    return {k: rng.fr() for k in ("alpha", "beta", "delta", "x", "gamma")}


def _circuit(n):
    from oracle import restate as rs

    return rs.toy_circuit()[0] if n == 4 else rs.synthetic_circuit(n)[0]


def _weights(pr, seed, count):
    rng = pr.SplitMix64(seed)
    return [(rng.next() << 64 | rng.next()) or 1 for _ in range(count)]


def _interpolate_on(pr, nodes, ys):
    """Coefficients of the polynomial of degree < len(nodes) with p(nodes[j]) = ys[j]"""
    R = pr.R
    acc = [0]
    for j, xj in enumerate(nodes):
        basis, den = [1], 1
        for m, xm in enumerate(nodes):
            if m != j:
                basis = pr.poly_mul(basis, [(-xm) % R, 1])
                den = den * pr.fr_inv((xj - xm) % R) % R
        acc = pr.poly_add(acc, [c * den % R * ys[j] % R for c in basis])
    return acc


def _basis_at(pr, nodes, x):
    """l_j(x) for the Lagrange basis of `nodes`"""
    R = pr.R
    out = []
    for j, xj in enumerate(nodes):
        v = 1
        for m, xm in enumerate(nodes):
            if m != j:
                v = v * ((x - xm) % R) % R * pr.fr_inv((xj - xm) % R) % R
        out.append(v)
    return out


def _dot(pr, a, b):
    assert len(a) == len(b)
    return sum(u * v for u, v in zip(a, b)) % pr.R


@pytest.mark.parametrize("n", SIZES)
def test_lagrange_form_against_monomial_form_on_both_node_sets(pr, n):
    """sum_j rho_j l_j(x) = sum_i c_i x^i with c the interpolant of rho: on 1..n (cnt = n) and on n+1..2n-1 (cnt = n-1)"""
    from oracle import restate as rs

    x = _toxic(pr)["x"]
    rho = _weights(pr, n, n)
    for nodes in (list(range(1, n + 1)), list(range(n + 1, 2 * n))):
        cnt = len(nodes)
        lagr = _basis_at(pr, nodes, x)
        mono = [pow(x, i, pr.R) for i in range(cnt)]
        c = _interpolate_on(pr, nodes, rho[:cnt])
        assert len(c) == cnt
        assert _dot(pr, rho[:cnt], lagr) == _dot(pr, c, mono)
        # the form on the other node set does not satisfy it
        other = _basis_at(pr, [v + 1 for v in nodes], x)
        assert _dot(pr, rho[:cnt], other) != _dot(pr, c, mono)
    assert _basis_at(pr, list(range(1, n + 1)), x) == rs.lagrange_at(n, x)[0]
    assert _interpolate_on(pr, list(range(1, n + 1)), rho) == pr.interpolate(rho)


@pytest.mark.parametrize("n", SIZES)
def test_xi_t_against_the_string(pr, n):
    """delta * sum_{i<n-1} rho_i xi_t[i] = sum_{m<2n-1} (rho * z)_m x^m, z = prod_{j=1..n} (X - j); and lxi_t against xi_t"""
    from oracle import restate as rs

    R, tw = pr.R, _toxic(pr)
    x, delta = tw["x"], tw["delta"]
    z = [1]
    for j in range(1, n + 1):
        z = pr.poly_mul(z, [(-j) % R, 1])
    zx = rs.lagrange_at(n, x)[1]
    assert pr.poly_eval(z, x) == zx
    txd = pr.fr_div(zx, delta)
    xi_t = [pow(x, i, R) * txd % R for i in range(n - 1)]  # groth16.go:94-97
    rho = _weights(pr, n, n)[:n - 1]
    rz = pr.poly_mul(rho, z)
    assert len(rz) == 2 * n - 1
    t1 = [pow(x, m, R) for m in range(2 * n - 1)]
    assert delta * _dot(pr, rho, xi_t) % R == _dot(pr, rz, t1)
    nodes = list(range(n + 1, 2 * n))
    lxi_t = [v * txd % R for v in _basis_at(pr, nodes, x)]
    assert _dot(pr, rho, lxi_t) == _dot(pr, _interpolate_on(pr, nodes, rho), xi_t)


@pytest.mark.parametrize("n", SIZES)
def test_io_and_nio_parts_against_the_string(pr, co, n):
    """gamma * sum_{i<diff} rho_i IoLP[i] = E_io and delta * sum_{i>=diff} rho_i NioLP[i-diff] = E_nio with
    E_S = <cU, B> + <cV, A> + <cW, T1[:n]>, cU, cV, cW the interpolants on 1..n of L rho_S, R rho_S, O rho_S"""
    from oracle import restate as rs

    R, tw = pr.R, _toxic(pr)
    c = _circuit(n)
    assert c.nbGates == n
    key = rs.groth16_setup(c, tw["alpha"], tw["beta"], tw["delta"], tw["x"], tw["gamma"])
    diff = c.nbVars - c.nbIO
    assert 0 < diff < c.nbVars and len(key.tw.IoLP) == diff and len(key.tw.NioLP) == c.nbVars - diff
    rho = _weights(pr, n, max(c.nbVars, n))[:c.nbVars]
    t1 = [pow(tw["x"], i, R) for i in range(n)]
    a, b = [tw["alpha"] * p % R for p in t1], [tw["beta"] * p % R for p in t1]

    def e_of(rho_s):
        cu, cv, cw = (pr.interpolate(y) for y in c.values(rho_s))
        return (_dot(pr, cu, b) + _dot(pr, cv, a) + _dot(pr, cw, t1)) % R

    rho_io = rho[:diff] + [0] * (c.nbVars - diff)
    rho_nio = [0] * diff + rho[diff:]
    assert tw["gamma"] * _dot(pr, rho[:diff], key.tw.IoLP) % R == e_of(rho_io)
    assert tw["delta"] * _dot(pr, rho[diff:], key.tw.NioLP) % R == e_of(rho_nio)
    # the split sits at diff and nowhere else: moving one variable to the other part breaks both equations
    moved = rho[:diff - 1] + [0] * (c.nbVars - diff + 1)
    assert tw["gamma"] * _dot(pr, rho[:diff], key.tw.IoLP) % R != e_of(moved)
