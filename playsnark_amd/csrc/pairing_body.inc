// The BLS12-381 ate pairing over a base field `Base` and its quadratic extension `Base2` (typedefs of the including
// namespace, which also supplies canon_wide): tower arithmetic, Miller loops, final exponentiations.  Included twice by
// pairing_math.inc -- over the device representation (Fp / Fp2: what the sanitizer build drives to check the lazy-limb
// contract through three levels of tower) and over the host field (Fq / Fq2, hostfield.inc: what the verifiers run).
struct Fp6 { Base2 c0, c1, c2; };
struct Fp12 { Fp6 c0, c1; };

PS_TOWER_HD static inline Base2 mul_xi(const Base2& a) {  // * (1 + u)
    return f_norm(Base2{f_sub(a.c0, a.c1), f_add(a.c0, a.c1)});
}
PS_TOWER_HD static inline Fp6 f6_add(const Fp6& a, const Fp6& b) { return Fp6{f_add(a.c0, b.c0), f_add(a.c1, b.c1), f_add(a.c2, b.c2)}; }
PS_TOWER_HD static inline Fp6 f6_sub(const Fp6& a, const Fp6& b) { return Fp6{f_sub(a.c0, b.c0), f_sub(a.c1, b.c1), f_sub(a.c2, b.c2)}; }
PS_TOWER_HD static inline Fp6 f6_neg(const Fp6& a) { return Fp6{f_neg(a.c0), f_neg(a.c1), f_neg(a.c2)}; }
PS_TOWER_HD static inline Fp6 f6_norm(const Fp6& a) { return Fp6{f_norm(a.c0), f_norm(a.c1), f_norm(a.c2)}; }
PS_TOWER_HD static inline Fp6 f6_zero() { Base2 z = f_zero((const Base2*)0); return Fp6{z, z, z}; }
PS_TOWER_HD static inline Fp6 f6_one() { Base2 z = f_zero((const Base2*)0); return Fp6{f_one((const Base2*)0), z, z}; }
PS_TOWER_HD PS_TOWER_F6 static Fp6 f6_mul(const Fp6& a, const Fp6& b) {  // v^3 = xi
    Base2 a0b0 = f_mul(a.c0, b.c0), a1b1 = f_mul(a.c1, b.c1), a2b2 = f_mul(a.c2, b.c2);
    Base2 c0 = f_add(a0b0, mul_xi(f_norm(f_add(f_mul(a.c1, b.c2), f_mul(a.c2, b.c1)))));
    Base2 c1 = f_add(f_add(f_mul(a.c0, b.c1), f_mul(a.c1, b.c0)), mul_xi(a2b2));
    Base2 c2 = f_add(f_add(f_mul(a.c0, b.c2), a1b1), f_mul(a.c2, b.c0));
    return f6_norm(Fp6{c0, c1, c2});
}
PS_TOWER_HD static inline Fp6 f6_mul_v(const Fp6& a) { return Fp6{mul_xi(a.c2), a.c0, a.c1}; }
static Fp6 f6_inv(const Fp6& a) {
    Base2 t0 = f_norm(f_sub(f_sqr(a.c0), mul_xi(f_mul(a.c1, a.c2))));
    Base2 t1 = f_norm(f_sub(mul_xi(f_sqr(a.c2)), f_mul(a.c0, a.c1)));
    Base2 t2 = f_norm(f_sub(f_sqr(a.c1), f_mul(a.c0, a.c2)));
    Base2 d = f_norm(f_add(f_mul(a.c0, t0), mul_xi(f_norm(f_add(f_mul(a.c2, t1), f_mul(a.c1, t2))))));
    Base2 di = f_inv(d);
    return Fp6{f_mul(t0, di), f_mul(t1, di), f_mul(t2, di)};
}
PS_TOWER_HD static inline Fp12 f12_one() { return Fp12{f6_one(), f6_zero()}; }
PS_TOWER_HD static Fp12 f12_mul(const Fp12& a, const Fp12& b) {  // w^2 = v
    Fp6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    Fp6 c0 = f6_norm(f6_add(t0, f6_mul_v(t1)));
    Fp6 c1 = f6_norm(f6_add(f6_mul(a.c0, b.c1), f6_mul(a.c1, b.c0)));
    return Fp12{c0, c1};
}
static inline Fp12 f12_conj(const Fp12& a) { return Fp12{a.c0, f6_norm(f6_neg(a.c1))}; }
static Fp12 f12_inv(const Fp12& a) {
    Fp6 d = f6_norm(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    Fp6 di = f6_inv(d);
    return Fp12{f6_mul(a.c0, di), f6_norm(f6_neg(f6_mul(a.c1, di)))};
}
static bool f2_is_zero_mod(const Base2& a) { return f_is_zero(a); }
static bool f12_eq(const Fp12& a, const Fp12& b) {
    const Base2* x[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    const Base2* y[6] = {&b.c0.c0, &b.c0.c1, &b.c0.c2, &b.c1.c0, &b.c1.c1, &b.c1.c2};
    for (int i = 0; i < 6; i++)
        if (!f2_is_zero_mod(f_sub(*x[i], *y[i]))) return false;
    return true;
}

// line through the twist points, evaluated at P = (xp, yp) in E(Base), scaled by w^3 (a subfield
// factor the final exponentiation removes):  l = (lam*xt - yt) + (-lam*xp) w^2 + yp w^3,
// with w^2 = v and w^3 = v*w in the tower.
static Fp12 line_value(const Base2& lam, const Base2& xt, const Base2& yt, const Base& xp, const Base& yp) {
    Base2 z = f_zero((const Base2*)0);
    Base2 c00 = f_norm(f_sub(f_mul(lam, xt), yt));
    Base2 lxp = Base2{f_mul(lam.c0, xp), f_mul(lam.c1, xp)};
    Fp12 l;
    l.c0 = Fp6{c00, f_norm(f_neg(lxp)), z};
    l.c1 = Fp6{z, Base2{yp, f_zero((const Base*)0)}, z};
    return l;
}

// Miller loop f_{|z|,Q}(P) with an affine running point (one Base2 inversion per step): the first, literal version, kept as
// the reference the projective loop below is tested against (tests/host_limb_check.cpp).  Identity in either slot -> one
static Fp12 miller_affine(const Affine<Base>& P, const Affine<Base2>& Q) {
    if (affine_is_identity<Base>(P) || affine_is_identity<Base2>(Q)) return f12_one();
    Fp12 f = f12_one();
    Base2 tx = Q.x, ty = Q.y;
    const unsigned long long z = PS_BLS_Z_ABS;
    for (int i = 62; i >= 0; i--) {
        // doubling step
        Base2 xx = f_sqr(tx);
        Base2 lam = f_mul(f_norm(f_add(f_add(xx, xx), xx)), f_inv(f_norm(f_add(ty, ty))));
        f = f12_mul(f12_mul(f, f), line_value(lam, tx, ty, P.x, P.y));
        Base2 nx = canon_wide(f_sub(f_sub(f_sqr(lam), tx), tx));
        Base2 ny = canon_wide(f_sub(f_mul(lam, f_sub(tx, nx)), ty));
        tx = nx; ty = ny;
        if ((z >> i) & 1) {  // addition step (T != +-Q throughout: T = kQ, 1 < k < r)
            Base2 lam2 = f_mul(f_norm(f_sub(ty, Q.y)), f_inv(f_norm(f_sub(tx, Q.x))));
            f = f12_mul(f, line_value(lam2, tx, ty, P.x, P.y));
            Base2 ax = canon_wide(f_sub(f_sub(f_sqr(lam2), tx), Q.x));
            Base2 ay = canon_wide(f_sub(f_mul(lam2, f_sub(tx, ax)), ty));
            tx = ax; ty = ay;
        }
    }
    return f;
}

// f^((p^12 - 1) / r) by square-and-multiply over the 2030-bit exponent (p^6 + 1) / r: the literal version, kept as the
// reference for final_exp below (which computes its cube)
static Fp12 final_exp_generic(const Fp12& f) {
    Fp12 base = f12_mul(f12_conj(f), f12_inv(f));  // f^(p^6 - 1)
    static const u32 e[PS_FINAL_EXP_WORDS] = PS_FINAL_EXP;
    Fp12 acc = f12_one();
    for (int i = PS_FINAL_EXP_BITS - 1; i >= 0; i--) {
        acc = f12_mul(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = f12_mul(acc, base);
    }
    return acc;
}

// ---- the fast path: inversion-free Miller loop, sparse line products, final exponentiation by the x-chain ----
// (a0 + a1 w)^2 = (a0^2 + v a1^2) + 2 a0 a1 w, two Fp6 products
PS_TOWER_HD static Fp12 f12_sqr(const Fp12& a) {
    Fp6 t = f6_mul(a.c0, a.c1);
    Fp6 s = f6_mul(f6_norm(f6_add(a.c0, a.c1)), f6_norm(f6_add(a.c0, f6_mul_v(a.c1))));
    Fp6 c0 = f6_norm(f6_sub(f6_sub(s, t), f6_mul_v(t)));
    return Fp12{c0, f6_norm(f6_add(t, t))};
}
// x * (a + b v) and x * (c v) in Fp6
PS_TOWER_HD PS_TOWER_F6 static Fp6 f6_mul_01(const Fp6& x, const Base2& a, const Base2& b) {
    Base2 c0 = f_add(f_mul(x.c0, a), mul_xi(f_mul(x.c2, b)));
    Base2 c1 = f_add(f_mul(x.c0, b), f_mul(x.c1, a));
    Base2 c2 = f_add(f_mul(x.c1, b), f_mul(x.c2, a));
    return f6_norm(Fp6{c0, c1, c2});
}
PS_TOWER_HD static Fp6 f6_mul_1(const Fp6& x, const Base2& c) { return Fp6{mul_xi(f_mul(x.c2, c)), f_mul(x.c0, c), f_mul(x.c1, c)}; }
// f * (a + b w^2 + c w^3): the shape of a line value (w^2 = v, w^3 = v w): 15 Base2 products instead of 18
PS_TOWER_HD static Fp12 f12_mul_line(const Fp12& f, const Base2& a, const Base2& b, const Base2& c) {
    Fp6 t0 = f6_mul_01(f.c0, a, b), t1 = f6_mul_1(f.c1, c);
    Fp6 m = f6_mul_01(f6_norm(f6_add(f.c0, f.c1)), a, f_norm(f_add(b, c)));
    return Fp12{f6_norm(f6_add(t0, f6_mul_v(t1))), f6_norm(f6_sub(f6_sub(m, t0), t1))};
}
PS_TOWER_HD static inline Base2 f2_scale(const Base2& a, const Base& k) { return Base2{f_mul(f_norm(a.c0), k), f_mul(f_norm(a.c1), k)}; }

// Running point T = (X : Y : Z) on the twist, x = X/Z, y = Y/Z.  A line value may be scaled by any non-zero element of
// Base2 (the final exponentiation kills proper subfields), so with the slope lam = N / D the affine line
// (lam x_T - y_T) - lam x_P w^2 + y_P w^3 becomes (N X - Y D) - (N Z) x_P w^2 + (D Z) y_P w^3 for a doubling (N = 3 X^2,
// D = 2 Y Z) and (u x_Q - v y_Q) - u x_P w^2 + v y_P w^3 for an addition of the affine Q (u = y_Q Z - Y, v = x_Q Z - X).
// Point formulas: dbl-2007-bl (a = 0) and madd-1998-cmo.  Every stored coordinate is a product or a short sum of
// products, so the lazy limbs stay bounded without re-canonicalising.
PS_TOWER_HD static Fp12 miller(const Affine<Base>& P, const Affine<Base2>& Q) {
    if (affine_is_identity<Base>(P) || affine_is_identity<Base2>(Q)) return f12_one();
    Fp12 f = f12_one();
    Base2 X = Q.x, Y = Q.y, Z = f_one((const Base2*)0);
    const unsigned long long z = PS_BLS_Z_ABS;
    for (int i = 62; i >= 0; i--) {
        {
            Base2 XX = f_sqr(X);
            Base2 N = f_norm(f_add(f_add(XX, XX), XX));
            Base2 YZ = f_mul(Y, Z);
            Base2 D = f_norm(f_add(YZ, YZ));
            Base2 la = f_norm(f_sub(f_mul(N, X), f_mul(Y, D)));
            Base2 lb = f_norm(f_neg(f2_scale(f_mul(N, Z), P.x)));
            Base2 lc = f2_scale(f_mul(D, Z), P.y);
            f = f12_mul_line(f12_sqr(f), la, lb, lc);
            Base2 ss = f_sqr(D), sss = f_mul(D, ss), R = f_mul(Y, D), RR = f_sqr(R);
            Base2 B = f_norm(f_sub(f_sub(f_sqr(f_norm(f_add(X, R))), XX), RR));
            Base2 h = f_norm(f_sub(f_sub(f_sqr(N), B), B));
            X = f_mul(h, D);
            Y = f_norm(f_sub(f_sub(f_mul(N, f_norm(f_sub(B, h))), RR), RR));
            Z = sss;
        }
        if ((z >> i) & 1) {  // addition step (T != +-Q throughout: T = kQ, 1 < k < r)
            Base2 u = f_norm(f_sub(f_mul(Q.y, Z), Y)), v = f_norm(f_sub(f_mul(Q.x, Z), X));
            Base2 la = f_norm(f_sub(f_mul(u, Q.x), f_mul(v, Q.y)));
            Base2 lb = f_norm(f_neg(f2_scale(u, P.x)));
            Base2 lc = f2_scale(v, P.y);
            f = f12_mul_line(f, la, lb, lc);
            Base2 uu = f_sqr(u), vv = f_sqr(v), vvv = f_mul(v, vv), R = f_mul(vv, X);
            Base2 A = f_norm(f_sub(f_sub(f_sub(f_mul(uu, Z), vvv), R), R));
            Base2 nY = f_norm(f_sub(f_mul(u, f_norm(f_sub(R, A))), f_mul(vvv, Y)));
            X = f_mul(v, A);
            Z = f_mul(vvv, Z);
            Y = nY;
        }
    }
    return f;
}

// Frobenius x -> x^p on Fp12 = Base2[w] / (w^6 - xi): the coefficient of w^k is conjugated and multiplied by g^k,
// g = w^(p-1) = xi^((p-1)/6) (an element of Base2, computed once).
struct FrobTable { Base2 g[6]; };
static FrobTable make_frob_table() {
    u32 e[12];
    for (int i = 0; i < 12; i++) e[i] = FpParams::mod(i);
    e[0] -= 1;  // p - 1 (p is odd)
    unsigned long long rem = 0;
    for (int i = 11; i >= 0; i--) {  // / 6
        unsigned long long cur = (rem << 32) | e[i];
        e[i] = (u32)(cur / 6);
        rem = cur % 6;
    }
    Base2 xi = Base2{f_one((const Base*)0), f_one((const Base*)0)}, acc = f_one((const Base2*)0), base = xi;
    for (int i = 0; i < 381; i++) {
        if ((e[i >> 5] >> (i & 31)) & 1) acc = f_mul(acc, base);
        base = f_sqr(base);
    }
    FrobTable t;
    t.g[0] = f_one((const Base2*)0);
    for (int k = 1; k < 6; k++) t.g[k] = f_mul(t.g[k - 1], acc);
    return t;
}
static inline Base2 f2_conj(const Base2& a) { return Base2{a.c0, f_norm(f_neg(a.c1))}; }
static Fp12 f12_frob(const Fp12& a) {
    static const FrobTable t = make_frob_table();
    Fp12 r;
    r.c0.c0 = f2_conj(a.c0.c0);
    r.c1.c0 = f_mul(f2_conj(a.c1.c0), t.g[1]);
    r.c0.c1 = f_mul(f2_conj(a.c0.c1), t.g[2]);
    r.c1.c1 = f_mul(f2_conj(a.c1.c1), t.g[3]);
    r.c0.c2 = f_mul(f2_conj(a.c0.c2), t.g[4]);
    r.c1.c2 = f_mul(f2_conj(a.c1.c2), t.g[5]);
    return r;
}
// m^x for the (negative) curve parameter x = -|z|, m in the cyclotomic subgroup (inverse = conjugate)
static Fp12 f12_pow_x(const Fp12& m) {
    const unsigned long long z = PS_BLS_Z_ABS;
    Fp12 acc = m;
    for (int i = 62; i >= 0; i--) {
        acc = f12_sqr(acc);
        if ((z >> i) & 1) acc = f12_mul(acc, m);
    }
    return f12_conj(acc);
}
// f^(3 (p^12 - 1) / r): easy part (p^6 - 1)(p^2 + 1), then 3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3
// (Hayashida, Hayasaka, Teruya 2020; the identity is checked on integers in tests/test_oracle_golden.py).  3 is prime to r,
// so "== 1" means what it means for the plain exponent; five exponentiations by |x| instead of a 2030-bit one.
static Fp12 final_exp(const Fp12& f) {
    Fp12 m = f12_mul(f12_conj(f), f12_inv(f));   // f^(p^6 - 1)
    m = f12_mul(f12_frob(f12_frob(m)), m);       // ^(p^2 + 1): now in the cyclotomic subgroup
    Fp12 a = f12_mul(f12_pow_x(m), f12_conj(m));             // m^(x - 1)
    a = f12_mul(f12_pow_x(a), f12_conj(a));                  // m^((x - 1)^2)
    Fp12 b = f12_mul(f12_pow_x(a), f12_frob(a));             // ^(x + p)
    Fp12 c = f12_mul(f12_mul(f12_pow_x(f12_pow_x(b)), f12_frob(f12_frob(b))), f12_conj(b));  // ^(x^2 + p^2 - 1)
    return f12_mul(c, f12_mul(f12_sqr(m), m));               // * m^3
}

// prod_i e(P_i, Q_i) == 1 ?
// The Miller loops are independent: one host thread each (the field code is pure), one final
// exponentiation for the product.
static bool pairing_product_is_one(const std::vector<std::pair<Affine<Base>, Affine<Base2>>>& pairs) {
    std::vector<std::future<Fp12>> loops;
    for (size_t i = 1; i < pairs.size(); i++)
        loops.push_back(std::async(std::launch::async, [&pairs, i] { return miller(pairs[i].first, pairs[i].second); }));
    Fp12 f = pairs.empty() ? f12_one() : miller(pairs[0].first, pairs[0].second);
    for (auto& l : loops) f = f12_mul(f, l.get());
    return f12_eq(final_exp(f), f12_one());
}

static Affine<Base> neg_g1(const Affine<Base>& a) {
    Affine<Base> r = a;
    if (!affine_is_identity<Base>(a)) r.y = fp_canon(f_neg(a.y));
    return r;
}

