// Host side of lagrange.hpp: ps_points_monomial_to_lagrange (included by capi.hip after prove.inc).

static Fr fr_inv2pow_host(int k) {  // 2^-k in Montgomery form (the constants the inverse NTT scales with)
    static const i32 tab[33][10] = PS_FR28_INV2POW;
    Fr r;
    for (int j = 0; j < FR_L; j++) r.l[j] = tab[k][j];
    return r;
}

// NTT over points: all p stages, in place (forward: natural -> bit-reversed; inverse: back, unscaled)
template <class F, bool INV>
static void ec_ntt(const NttTables& tb, hipStream_t st, Xyzz<F>* buf, u32 total, int p) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    for (int s = 0; s < p; s++) {
        const int logh = INV ? s : p - 1 - s;
        hipLaunchKernelGGL((k_ec_ntt_stage<KF, INV>), dim3(nblocks((size_t)(total / 2) * LN)), dim3(256), 0, st, buf, total, p, logh,
                           (const Fr*)(INV ? tb.inv : tb.fwd), tb.log_tab);
    }
}

// "<who>: <what>: <the HIP error>" as PS_ERR_HIP
static int fail_hip(const char* who, const char* what, hipError_t err) { return fail(PS_ERR_HIP, std::string(who) + ": " + what + ": " + hipGetErrorString(err)); }

template <class F>
static int monomial_to_lagrange_t(ps_ctx* c, const ps_qap* q, const ps_points* mono, bool shifted, ps_points** out) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const QapTables& qt = q->qt;
    const size_t n = q->n, cnt = shifted ? n - 1 : n;
    const u64 np = shifted ? qt.np_h : qt.np;
    const int lognp = shifted ? qt.lognp_h : qt.lognp;
    const std::vector<Fr*>& zhat = shifted ? qt.zhat_h : qt.zhat;
    const u64 off = shifted ? n : 0;
    hipStream_t st = c->stream;
    NttTables& tb = *ctx_tabs(c);
    hipError_t e = ntt_tables_ensure(tb, lognp + 1, st);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_points_monomial_to_lagrange: twiddles: ") + hipGetErrorString(e));
    const char* who = "ps_points_monomial_to_lagrange";
    Scope scope(st);
    int rc = points_alloc(c, mono->group, cnt, scope.result(out));
    if (rc) return rc;
    Xyzz<F>*A = nullptr, *B = nullptr, *E = nullptr;
    Fr *t1 = nullptr, *t2 = nullptr;
    if ((e = scope.device(&A, 2 * np)) != hipSuccess || (e = scope.device(&B, np)) != hipSuccess || (e = scope.device(&E, np)) != hipSuccess ||
        (e = scope.device(&t1, 2 * np)) != hipSuccess || (e = scope.device(&t2, 2 * np)) != hipSuccess)
        return fail_hip(who, "hipMalloc", e);
    if (storage_wait_ready(mono->st, st)) return fail(PS_ERR_HIP, "event wait failed");
    const u32 npu = (u32)np;
    // g = the monomial points, the identity beyond cnt
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks((size_t)np * LN)), dim3(256), 0, st, (const Affine<F>*)points_ptr(mono), (u32)cnt, npu, A);
    // ---- T_s^T, s = np .. 128 ----
    for (int logs = lognp; logs >= 7; logs--) {
        // stored transform of the left children, read backwards: hhat = NTT(rev(INTT(zhat))) / s
        if ((e = hipMemcpyAsync(t1, zhat[logs], sizeof(Fr) * np, hipMemcpyDeviceToDevice, st)) != hipSuccess) return fail_hip(who, "copy", e);
        if ((e = ntt_run<true>(tb, st, t1, np, logs)) != hipSuccess) return fail_hip(who, "ntt", e);
        hipLaunchKernelGGL(k_fr_rev_mod, dim3(nblk(np)), dim3(256), 0, st, t2, (const Fr*)t1, np, logs);
        if ((e = ntt_run<false>(tb, st, t2, np, logs)) != hipSuccess) return fail_hip(who, "ntt", e);
        hipLaunchKernelGGL(k_fr_scale, dim3(nblk(np)), dim3(256), 0, st, t2, (const Fr*)t2, fr_inv2pow_host(logs), np);
        if ((e = hipMemcpyAsync(B, A, sizeof(Xyzz<F>) * np, hipMemcpyDeviceToDevice, st)) != hipSuccess) return fail_hip(who, "copy", e);
        ec_ntt<F, false>(tb, st, B, npu, logs);
        hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks((size_t)np * LN)), dim3(256), 0, st, B, npu, (const Fr*)t2, ~0ull);
        ec_ntt<F, true>(tb, st, B, npu, logs);
        hipLaunchKernelGGL(k_ec_take_right<KF>, dim3(nblocks((size_t)(np / 2) * LN)), dim3(256), 0, st, A, (const Xyzz<F>*)B, npu, logs);
        if ((e = hipGetLastError()) != hipSuccess) return fail_hip(who, "level", e);
    }
    // ---- B^T on the blocks of 64 ----
    {
        Xyzz<F>*tin = A, *tout = B;
        for (int k = 0; k < 64; k++) {
            hipLaunchKernelGGL(k_ec_base_step<KF>, dim3(nblocks((size_t)np * LN)), dim3(256), 0, st, (const Xyzz<F>*)tin, tout, E, npu, k, off,
                               (u32)(np / 64));
            std::swap(tin, tout);
        }
        if ((e = hipGetLastError()) != hipSuccess) return fail_hip(who, "base", e);
    }
    // ---- C^T: correlation with v_k = (-1)^k / k! over 2 np, then D^T: times 1 / j! ----
    hipLaunchKernelGGL(k_ec_pad<KF>, dim3(nblocks((size_t)2 * np * LN)), dim3(256), 0, st, (const Xyzz<F>*)E, (u32)cnt, 2 * npu, A);
    hipLaunchKernelGGL(k_fr_v_rev, dim3(nblk(2 * np)), dim3(256), 0, st, t1, (const Fr*)qt.invfact, np);
    if ((e = ntt_run<false>(tb, st, t1, 2 * np, lognp + 1)) != hipSuccess) return fail_hip(who, "ntt", e);
    hipLaunchKernelGGL(k_fr_scale, dim3(nblk(2 * np)), dim3(256), 0, st, t1, (const Fr*)t1, fr_inv2pow_host(lognp + 1), 2 * np);
    ec_ntt<F, false>(tb, st, A, 2 * npu, lognp + 1);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks((size_t)2 * np * LN)), dim3(256), 0, st, A, 2 * npu, (const Fr*)t1, ~0ull);
    ec_ntt<F, true>(tb, st, A, 2 * npu, lognp + 1);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks((size_t)cnt * LN)), dim3(256), 0, st, A, (u32)cnt, (const Fr*)qt.invfact, ~0ull);
    // canonical affine points (the chain products of the batch normalisation go behind the cnt points: A holds 2 np)
    batch_to_affine<F>(c->stream, (char*)A, cnt, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail_hip(who, "kernels", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail_hip(who, "run", e);
    return scope.finish(PS_OK);
}

extern "C" int ps_points_monomial_to_lagrange(ps_ctx* c, const ps_qap* q, const ps_points* mono, int nodes, ps_points** out) {
    if (!c || !q || !mono || !out) return fail(PS_ERR_ARG, "ps_points_monomial_to_lagrange: NULL argument");
    *out = nullptr;
    if (nodes != 0 && nodes != 1) return fail(PS_ERR_ARG, "ps_points_monomial_to_lagrange: nodes must be 0 (1..n) or 1 (n+1..2n-1)");
    if (q->n < 2) return fail(PS_ERR_ARG, "ps_points_monomial_to_lagrange: needs at least 2 gates");
    const size_t want = nodes ? q->n - 1 : q->n;
    if (mono->n != want)  // the array is a polynomial basis of exactly that degree bound (algebra.go:350-352's rule)
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(want) + " and blinded eval points " + std::to_string(mono->n));
    HIP_TRY(hipSetDevice(c->device));
    return mono->group == PS_G1 ? monomial_to_lagrange_t<Fp>(c, q, mono, nodes == 1, out) : monomial_to_lagrange_t<Fp2>(c, q, mono, nodes == 1, out);
}

// out[i] = k[i] * pts[i], k: one Montgomery scalar per point, on the device (the caller orders their producer before c->stream's
// next kernel).  The scalar multiplication the conversion above uses (ec_mul_glv: GLV split, fixed signed windows): the points
// must lie in the subgroup of order r.  Canonical affine output; returns when the result is complete.
template <class F>
static int points_scale_each_t(ps_ctx* c, const ps_points* pts, const Fr* k_mont, ps_points** out) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = pts->n;
    hipStream_t st = c->stream;
    const char* who = "scaling a point array";
    Scope scope(st);
    int rc = points_alloc(c, pts->group, n, scope.result(out));
    if (rc || n == 0) return scope.finish(rc);
    char* buf = nullptr;  // n XYZZ points, then batch_to_affine's chain products
    hipError_t e;
    if ((e = scope.device(&buf, batch_affine_tmp_bytes(n, sizeof(Xyzz<F>)))) != hipSuccess) return fail_hip(who, "hipMalloc", e);
    if (storage_wait_ready(pts->st, st)) return fail_hip(who, "event wait", hipErrorUnknown);
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks(n * LN)), dim3(256), 0, st, (const Affine<F>*)points_ptr(pts), (u32)n, (u32)n, (Xyzz<F>*)buf);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks(n * LN)), dim3(256), 0, st, (Xyzz<F>*)buf, (u32)n, k_mont, ~0ull);
    batch_to_affine<F>(c->stream, buf, n, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail_hip(who, "kernels", e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail_hip(who, "run", e);
    return scope.finish(PS_OK);
}
static int points_scale_each(ps_ctx* c, const ps_points* pts, const Fr* k_mont, ps_points** out) {
    return pts->group == PS_G1 ? points_scale_each_t<Fp>(c, pts, k_mont, out) : points_scale_each_t<Fp2>(c, pts, k_mont, out);
}

// Test hook (not in the header, like ps_debug_pair_add_probe): out[i] = k[i] * pts[i] for plain scalars -- so that the edge
// scalars of ec_mul_glv (0, 1, lambda - 1, lambda, r - 1, digits of -8 ...) are checked against the oracle one by one, not only
// through random twiddles (tests/test_prover_gpu.py).
static int debug_points_scale(ps_ctx* c, const ps_points* pts, const ps_scalars* sc, ps_points** out) {
    const size_t n = pts->n;
    Scope scope(c->stream);
    Fr* km = nullptr;
    hipError_t e = scope.device(&km, n);
    if (e != hipSuccess) return fail_hip("ps_debug_points_scale", "hipMalloc", e);
    if (storage_wait_ready(sc->st, c->stream)) return fail(PS_ERR_HIP, "ps_debug_points_scale: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(n)), dim3(256), 0, c->stream, km, scalars_ptr(sc), (u64)n);
    return points_scale_each(c, pts, km, out);
}
extern "C" int ps_debug_points_scale(ps_ctx* c, const ps_points* pts, const ps_scalars* sc, ps_points** out) {
    if (!c || !pts || !sc || !out) return fail(PS_ERR_ARG, "ps_debug_points_scale: NULL argument");
    *out = nullptr;
    if (pts->n != sc->n || pts->n == 0) return fail(PS_ERR_LENGTH, "ps_debug_points_scale: one scalar per point, at least one");
    HIP_TRY(hipSetDevice(c->device));
    return debug_points_scale(c, pts, sc, out);
}
