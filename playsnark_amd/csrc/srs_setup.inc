// A circuit's Groth16 key from a powers-of-tau string, and the delta / gamma shares folded into it afterwards (included by
// capi.hip after verify_batch.inc):
//   ps_qap_column_sums          out[i] = sum_j M[j][i] P[j]   (ec_spmv.hpp: the sparse matrix over points)
//   ps_groth16_setup_from_srs   NewGroth16TrustedSetup (groth16.go:64-101) with delta = gamma = 1 and NO toxic waste
//   ps_groth16_crs_contribute   delta *= d, gamma *= g
//   ps_groth16_crs_check_update was `after` made from `before` by some such fold?
// Everything but the column sums is the existing machinery: the conversion of lagrange.inc, its NTT over points, the uniform
// form of k_ec_scale, the sums and ps_pairing_product_is_one.

template <class F>
static int column_sums_t(ps_ctx* c, const ps_qap* q, int which, const ps_points* p, ps_points** out) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const DevCsr& t = q->matT[which];
    const size_t m = q->m, nnz = t.nnz;
    hipStream_t st = c->stream;
    Scope scope(st);
    int rc = points_alloc(c, p->group, m, scope.result(out));
    if (rc) return rc;
    char* buf = nullptr;  // m XYZZ points, then batch_to_affine's chain products
    u64* mag = nullptr;
    u32* cs = nullptr;
    const bool wide = q->wide[which] != 0;  // (ec_spmv.hpp: four magnitude words per entry instead of one)
    hipError_t e;
    if ((e = scope.device(&buf, batch_affine_tmp_bytes(m, sizeof(Xyzz<F>)))) != hipSuccess ||
        (e = scope.device(&mag, (wide ? 4 : 1) * std::max<size_t>(nnz, 1))) != hipSuccess || (e = scope.device(&cs, nnz)) != hipSuccess)
        return fail(PS_ERR_HIP, std::string("ps_qap_column_sums: hipMalloc: ") + hipGetErrorString(e));
    if (storage_wait_ready(p->st, st)) return fail(PS_ERR_HIP, "ps_qap_column_sums: event wait failed");
    const Affine<F>* pts = (const Affine<F>*)points_ptr(p);
    if (!wide) {
        if (nnz) hipLaunchKernelGGL(k_colsum_coef, dim3(nblk(nnz)), dim3(256), 0, st, (const Fr*)t.val, (const u32*)t.col, (u32)nnz, mag, cs);
        hipLaunchKernelGGL(k_colsum_rows<KF>, dim3(nblocks(m * LN)), dim3(256), 0, st, (const u32*)t.row_ptr, (const u64*)mag, (const u32*)cs, pts, (u32)m,
                           (Xyzz<F>*)buf);
        if (t.n_long)
            hipLaunchKernelGGL(k_colsum_long<KF>, dim3(t.n_long), dim3(COLSUM_LONG_THREADS), sizeof(Xyzz<F>) * (COLSUM_LONG_THREADS / LN), st,
                               (const u32*)t.row_ptr, (const u64*)mag, (const u32*)cs, pts, (const u32*)t.long_rows, (Xyzz<F>*)buf);
    } else {
        hipLaunchKernelGGL(k_colsum_coef_wide, dim3(nblk(nnz)), dim3(256), 0, st, (const Fr*)t.val, (const u32*)t.col, (u32)nnz, mag, cs);
        hipLaunchKernelGGL(k_colsum_rows_wide<KF>, dim3(nblocks(m * LN)), dim3(256), 0, st, (const u32*)t.row_ptr, (const u64*)mag, (const u32*)cs,
                           (u32)nnz, pts, (u32)m, (Xyzz<F>*)buf);
        if (t.n_long_narrow)  // long rows without a wide entry: one workgroup each, at most 64 planes
            hipLaunchKernelGGL(k_colsum_long_wide<KF>, dim3(t.n_long_narrow), dim3(COLSUM_LONG_THREADS), sizeof(Xyzz<F>) * (COLSUM_LONG_THREADS / LN), st,
                               (const u32*)t.row_ptr, (const u64*)mag, (const u32*)cs, (u32)nnz, pts, (const u32*)t.long_narrow, (Xyzz<F>*)buf);
        for (size_t k = 0; k < t.long_wide_h.size(); k += 3)  // long rows with one: the identity here, their sum below
            if ((e = hipMemsetAsync(buf + sizeof(Xyzz<F>) * t.long_wide_h[k], 0, sizeof(Xyzz<F>), st)) != hipSuccess)
                return fail(PS_ERR_HIP, std::string("ps_qap_column_sums: hipMemsetAsync: ") + hipGetErrorString(e));
    }
    batch_to_affine<F>(c->stream, buf, m, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_qap_column_sums: kernels: ") + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_qap_column_sums: run: ") + hipGetErrorString(e));
    // A long row that holds a wide entry is a multi-scalar multiplication, sum_e v_e P[col_e], of thousands of full-width
    // terms (every round constant of a hash multiplies `const`).  k_colsum_long_wide took 1.33 s for the 65 528 wide entries of
    // R's `const` column of a 2^16-gate MiMC circuit, 2 000 x all other work of the three column sums; the library's own sum
    // takes 3.3 ms for it, gather and conversion included (profiles/column_sums_wide.txt).  So: the row's points gathered
    // (k_gather_words), its coefficients as the scalars, ps_msm -- bit-exact on identities, repeated and opposite points.
    if (wide)
        for (size_t k = 0; k < t.long_wide_h.size(); k += 3) {
            const u32 row = t.long_wide_h[k], first = t.long_wide_h[k + 1], len = t.long_wide_h[k + 2];
            constexpr u32 W = sizeof(Affine<F>) / 4;
            Scope row_scope;  // (freed row by row: a circuit may have many such rows)
            ps_points** gp = row_scope.points();
            ps_scalars** sc = row_scope.scalars();
            uint8_t wire[192];
            if ((rc = points_alloc(c, p->group, len, gp))) return rc;
            hipLaunchKernelGGL(k_gather_words, dim3(nblocks((size_t)len * W)), dim3(256), 0, st, (const u32*)pts, (const u32*)t.col + first, len, (u64)W,
                               (u64)0, W, (u32*)(*gp)->st->p);
            if ((rc = scalars_from_mont(c, t.val + first, len, sc)) || (rc = ps_msm(c, *gp, *sc, wire))) return rc;
            Affine<F> sum;
            if (!read_affine(sum, wire)) return fail(PS_ERR_HIP, "ps_qap_column_sums: the sum of a long row is no point");
            if ((e = hipMemcpy((char*)(*out)->st->p + sizeof(Affine<F>) * row, &sum, sizeof sum, hipMemcpyHostToDevice)) != hipSuccess)
                return fail(PS_ERR_HIP, std::string("ps_qap_column_sums: hipMemcpy: ") + hipGetErrorString(e));
        }
    return scope.finish(PS_OK);
}

extern "C" int ps_qap_column_sums(ps_ctx* c, const ps_qap* q, int which, const ps_points* p, ps_points** out) {
    if (!c || !q || !p || !out) return fail(PS_ERR_ARG, "ps_qap_column_sums: NULL argument");
    *out = nullptr;
    if (which < 0 || which > 2) return fail(PS_ERR_ARG, "ps_qap_column_sums: which must be 0 (left), 1 (right) or 2 (out)");
    if (p->n != q->n)  // one point per gate (algebra.go:350-352's rule)
        return fail(PS_ERR_LENGTH, "mismatch of length between gates " + std::to_string(q->n) + " and points " + std::to_string(p->n));
    HIP_TRY(hipSetDevice(c->device));
    return p->group == PS_G1 ? column_sums_t<Fp>(c, q, which, p, out) : column_sums_t<Fp2>(c, q, which, p, out);
}

// out[i] = k * pts[i] for ONE scalar k (Montgomery form): k_ec_scale with every index masked to the first scalar.  The points
// must lie in the subgroup of order r (ec_mul_glv).
template <class F>
static int points_scale_uniform_t(ps_ctx* c, const ps_points* pts, const Fr& k_mont, ps_points** out) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = pts->n;
    hipStream_t st = c->stream;
    Scope scope(st);
    int rc = points_alloc(c, pts->group, n, scope.result(out));
    if (rc || n == 0) return scope.finish(rc);
    char* buf = nullptr;
    Fr* km = nullptr;
    hipError_t e;
    if ((e = scope.device(&buf, batch_affine_tmp_bytes(n, sizeof(Xyzz<F>)))) != hipSuccess || (e = scope.device(&km, 1)) != hipSuccess ||
        (e = hipMemcpy(km, &k_mont, sizeof(Fr), hipMemcpyHostToDevice)) != hipSuccess)
        return fail(PS_ERR_HIP, std::string("scaling a point array: ") + hipGetErrorString(e));
    if (storage_wait_ready(pts->st, st)) return fail(PS_ERR_HIP, "scaling a point array: event wait failed");
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks(n * LN)), dim3(256), 0, st, (const Affine<F>*)points_ptr(pts), (u32)n, (u32)n, (Xyzz<F>*)buf);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks(n * LN)), dim3(256), 0, st, (Xyzz<F>*)buf, (u32)n, (const Fr*)km, 0ull);
    batch_to_affine<F>(c->stream, buf, n, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, std::string("scaling a point array: kernels: ") + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(PS_ERR_HIP, std::string("scaling a point array: run: ") + hipGetErrorString(e));
    return scope.finish(PS_OK);
}
static int points_scale_uniform(ps_ctx* c, const ps_points* pts, const Fr& k_mont, ps_points** out) {
    return pts->group == PS_G1 ? points_scale_uniform_t<Fp>(c, pts, k_mont, out) : points_scale_uniform_t<Fp2>(c, pts, k_mont, out);
}

// XiT without x: xi_t[i] = sum_k z_k tau[i + k], i < n - 1, z = prod_{j=1..n} (X - j) -- the correlation of 2n - 1 points with n + 1
// scalars.  The C^T step of monomial_to_lagrange_t with another multiplier: NTT over points, times the stored transform of z read
// backwards (the inverse's 2^-p rides in it), inverse NTT.  Size 2^p >= 2n - 1: i + k <= 2n - 2 never wraps.
static int srs_xi_t(ps_ctx* c, const ps_qap* q, const ps_points* tau, ps_points** out) {
    typedef Fp F;
    typedef KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = q->n, cnt = n - 1, len = 2 * n - 1;
    const int p = ilog2_ceil(len);
    const u32 S = 1u << p;
    hipStream_t st = c->stream;
    NttTables& tb = *ctx_tabs(c);
    hipError_t e = ntt_tables_ensure(tb, p, st);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_setup_from_srs: twiddles: ") + hipGetErrorString(e));
    Scope scope(st);
    int rc = points_alloc(c, PS_G1, cnt, scope.result(out));
    if (rc) return rc;
    Xyzz<F>* A = nullptr;  // S points; the chain products of the batch normalisation go behind the first cnt < S / 2
    Fr* t1 = nullptr;
    if ((e = scope.device(&A, S)) != hipSuccess || (e = scope.device(&t1, S)) != hipSuccess)
        return fail(PS_ERR_HIP, std::string("ps_groth16_setup_from_srs: hipMalloc: ") + hipGetErrorString(e));
    if (storage_wait_ready(tau->st, st)) return fail(PS_ERR_HIP, "ps_groth16_setup_from_srs: event wait failed");
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks((size_t)S * LN)), dim3(256), 0, st, (const Affine<F>*)points_ptr(tau), (u32)len, S, A);
    hipLaunchKernelGGL(k_fr_rev_pad, dim3(nblk(S)), dim3(256), 0, st, t1, (const Fr*)q->qt.z, (u64)(n + 1), p);
    if ((e = ntt_run<false>(tb, st, t1, S, p)) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_setup_from_srs: ntt: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(k_fr_scale, dim3(nblk(S)), dim3(256), 0, st, t1, (const Fr*)t1, fr_inv2pow_host(p), (u64)S);
    ec_ntt<F, false>(tb, st, A, S, p);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks((size_t)S * LN)), dim3(256), 0, st, A, S, (const Fr*)t1, ~0ull);
    ec_ntt<F, true>(tb, st, A, S, p);
    batch_to_affine<F>(c->stream, (char*)A, cnt, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_setup_from_srs: kernels: ") + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_setup_from_srs: run: ") + hipGetErrorString(e));
    return scope.finish(PS_OK);
}

static void crs_release(ps_groth16_crs* k) {
    for (ps_points* p : {k->xi, k->xi2, k->io_lp, k->nio_lp, k->xi_t, k->lxi, k->lxi2, k->lxi_t}) ps_points_free(p);
    memset(k, 0, sizeof *k);
}
// a key that is complete or empty: an error releases what `out` holds by then and keeps its text
static int crs_or_nothing(int rc, ps_groth16_crs* out) {
    if (rc) {
        KeepError keep;
        crs_release(out);
    }
    return rc;
}
template <class F>
static void generator_bytes(uint8_t* out) {
    const Affine<F> g = generator((const F*)0);
    write_affine(out, xyzz_from_affine<F>(g.x, g.y));
}
// a fresh array holding [first, first + n) of `p`
static int points_copy(ps_ctx* c, const ps_points* p, size_t first, size_t n, ps_points** out) {
    if (storage_wait_ready(p->st, c->stream)) return fail(PS_ERR_HIP, "event wait failed");
    return points_concat(c, p->group, {{(const char*)points_ptr(p) + first * point_bytes(p->group), n}}, out);
}

// The key's arrays into a zeroed `out`, arguments validated; on an error `out` is left as far as it got (crs_or_nothing).
static int setup_from_srs_run(ps_ctx* c, const ps_qap* q, const ps_groth16_srs* srs, ps_groth16_crs* out) {
    const size_t n = q->n, m = q->m, diff = q->m - q->nio;
    Scope scope(c->stream);
    ps_points **la = scope.points(), **lb = scope.points(), **sums[3] = {scope.points(), scope.points(), scope.points()}, **lin = scope.points();
    scope.in_flight();  // the temporaries are freed with the stream idle, on an error too
    int rc;
    // Alpha, Beta: the first points of the scaled arrays; Beta2 as given; Delta, Delta2, Gamma: the generators   (groth16.go:67-76)
    if ((rc = ps_points_download(c, srs->alpha_tau_g1, 0, 1, out->alpha))) return rc;
    if ((rc = ps_points_download(c, srs->beta_tau_g1, 0, 1, out->beta))) return rc;
    memcpy(out->beta2, srs->beta_g2, 192);
    generator_bytes<Fp>(out->delta);
    generator_bytes<Fp2>(out->delta2);
    generator_bytes<Fp2>(out->gamma);
    // Xi, Xi2: the first n powers, and their Lagrange forms                                                    (groth16.go:79-80)
    if ((rc = points_copy(c, srs->tau_g1, 0, n, &out->xi))) return rc;
    if ((rc = points_copy(c, srs->tau_g2, 0, n, &out->xi2))) return rc;
    if ((rc = ps_points_monomial_to_lagrange(c, q, out->xi, 0, &out->lxi))) return rc;
    if ((rc = ps_points_monomial_to_lagrange(c, q, out->xi2, 0, &out->lxi2))) return rc;
    // IoLP | NioLP = {(beta u_i(x) + alpha v_i(x) + w_i(x)) G1}: L over {beta l_j(x) G1}, R over {alpha l_j(x) G1}, O over
    // {l_j(x) G1}                                                                                       (groth16.go:86-91, 254-264)
    if ((rc = ps_points_monomial_to_lagrange(c, q, srs->beta_tau_g1, 0, lb))) return rc;
    if ((rc = ps_points_monomial_to_lagrange(c, q, srs->alpha_tau_g1, 0, la))) return rc;
    if ((rc = ps_qap_column_sums(c, q, 0, *lb, sums[0]))) return rc;
    if ((rc = ps_qap_column_sums(c, q, 1, *la, sums[1]))) return rc;
    if ((rc = ps_qap_column_sums(c, q, 2, out->lxi, sums[2]))) return rc;
    if ((rc = points_alloc(c, PS_G1, m, lin))) return rc;
    hipLaunchKernelGGL(k_points_add3<Fp>, dim3(nblocks(m)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(*sums[0]),
                       (const Affine<Fp>*)points_ptr(*sums[1]), (const Affine<Fp>*)points_ptr(*sums[2]), (u32)m, (Affine<Fp>*)(*lin)->st->p);
    if (hipGetLastError() != hipSuccess) return fail(PS_ERR_HIP, "ps_groth16_setup_from_srs: the sum of the three column sums failed to launch");
    if ((rc = points_copy(c, *lin, 0, diff, &out->io_lp))) return rc;
    if ((rc = points_copy(c, *lin, diff, m - diff, &out->nio_lp))) return rc;
    // XiT = {x^i t(x) G1}, i < n - 1, and its Lagrange form on the nodes n+1..2n-1                              (groth16.go:94-97)
    if ((rc = srs_xi_t(c, q, srs->tau_g1, &out->xi_t))) return rc;
    if ((rc = ps_points_monomial_to_lagrange(c, q, out->xi_t, 1, &out->lxi_t))) return rc;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(PS_ERR_HIP, "ps_groth16_setup_from_srs: the device reported an error");
    return PS_OK;
}

extern "C" int ps_groth16_setup_from_srs(ps_ctx* c, const ps_qap* q, const ps_groth16_srs* srs, ps_groth16_crs* out) {
    if (!c || !q || !srs || !out || !srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1)
        return fail(PS_ERR_ARG, "ps_groth16_setup_from_srs: NULL argument");
    memset(out, 0, sizeof *out);
    const size_t n = q->n;
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_setup_from_srs: needs at least 2 gates");
    if (srs->tau_g1->group != PS_G1 || srs->tau_g2->group != PS_G2 || srs->alpha_tau_g1->group != PS_G1 || srs->beta_tau_g1->group != PS_G1)
        return fail(PS_ERR_ARG, "ps_groth16_setup_from_srs: tau_g2 is a G2 array, the other three are G1 arrays");
    if (c->q_len) return fail(PS_ERR_ARG, "ps_groth16_setup_from_srs: sums are pending on this context (ps_msm_finish them first)");
    const struct { const ps_points* p; size_t want; const char* name; } lens[4] = {
        {srs->tau_g1, 2 * n - 1, "tau_g1"}, {srs->tau_g2, n, "tau_g2"}, {srs->alpha_tau_g1, n, "alpha_tau_g1"}, {srs->beta_tau_g1, n, "beta_tau_g1"}};
    for (const auto& l : lens)
        if (l.p->n != l.want)  // BlindEval's panic (algebra.go:350-352)
            return fail(PS_ERR_LENGTH, std::string("mismatch of length between ") + l.name + " " + std::to_string(l.p->n) + " and the " + std::to_string(l.want) +
                                           " powers a circuit of " + std::to_string(n) + " gates needs");
    {
        Affine<Fp2> b2;
        if (!read_affine(b2, srs->beta_g2)) return fail(PS_ERR_ENCODING, "ps_groth16_setup_from_srs: beta_g2 is not a canonical point on the curve");
    }
    HIP_TRY(hipSetDevice(c->device));
    return crs_or_nothing(setup_from_srs_run(c, q, srs, out), out);
}

static int crs_contribute_run(ps_ctx* c, const ps_groth16_crs* in, const uint8_t* d_be32, const uint8_t* g_be32, const Fr& dinv, const Fr& ginv,
                              ps_groth16_crs* out) {
    int rc;
    memcpy(out->alpha, in->alpha, 96);
    memcpy(out->beta, in->beta, 96);
    memcpy(out->beta2, in->beta2, 192);
    if ((rc = ps_points_lincomb(PS_G1, in->delta, d_be32, 1, out->delta))) return rc;
    if ((rc = ps_points_lincomb(PS_G2, in->delta2, d_be32, 1, out->delta2))) return rc;
    if ((rc = ps_points_lincomb(PS_G2, in->gamma, g_be32, 1, out->gamma))) return rc;
    // NioLP, XiT (and its Lagrange form) carry 1 / delta, IoLP carries 1 / gamma   (groth16.go:86-97)
    if ((rc = points_scale_uniform(c, in->nio_lp, dinv, &out->nio_lp))) return rc;
    if ((rc = points_scale_uniform(c, in->xi_t, dinv, &out->xi_t))) return rc;
    if (in->lxi_t && (rc = points_scale_uniform(c, in->lxi_t, dinv, &out->lxi_t))) return rc;
    if ((rc = points_scale_uniform(c, in->io_lp, ginv, &out->io_lp))) return rc;
    // the arrays no share touches: views of the input's storage
    if ((rc = ps_points_slice(in->xi, 0, in->xi->n, &out->xi))) return rc;
    if ((rc = ps_points_slice(in->xi2, 0, in->xi2->n, &out->xi2))) return rc;
    if (in->lxi && (rc = ps_points_slice(in->lxi, 0, in->lxi->n, &out->lxi))) return rc;
    if (in->lxi2 && (rc = ps_points_slice(in->lxi2, 0, in->lxi2->n, &out->lxi2))) return rc;
    return PS_OK;
}
extern "C" int ps_groth16_crs_contribute(ps_ctx* c, const ps_groth16_crs* in, const uint8_t* d_be32, const uint8_t* g_be32, ps_groth16_crs* out) {
    if (!c || !in || !d_be32 || !g_be32 || !out || in == out) return fail(PS_ERR_ARG, "ps_groth16_crs_contribute: NULL argument (or out == in)");
    if (!in->xi || !in->xi2 || !in->io_lp || !in->nio_lp || !in->xi_t) return fail(PS_ERR_ARG, "ps_groth16_crs_contribute: the key lacks an array");
    memset(out, 0, sizeof *out);
    const Fr d = fr_mont_from_be32(d_be32), g = fr_mont_from_be32(g_be32);
    if (fr_is_zero(d) || fr_is_zero(g)) return fail(PS_ERR_ARG, "ps_groth16_crs_contribute: the shares d and g must be non-zero");
    HIP_TRY(hipSetDevice(c->device));
    return crs_or_nothing(crs_contribute_run(c, in, d_be32, g_be32, fr_inv(d), fr_inv(g), out), out);
}

// -P for an affine encoding that has been validated
static void g1_negated(uint8_t* out, const uint8_t* in) {
    bool ok = true;
    write_affine(out, xyzz_neg<Fp>(host_point<Fp>(in, ok)));
}
// e(a1, b1) == e(a2, b2) through ps_pairing_product_is_one on two uploaded pairs: e(a1, b1) e(-a2, b2) == 1
static int pairing_pair_equal(ps_ctx* c, const uint8_t* a1, const uint8_t* b1, const uint8_t* a2, const uint8_t* b2, int* equal) {
    uint8_t g1[2 * 96], g2[2 * 192];
    memcpy(g1, a1, 96);
    g1_negated(g1 + 96, a2);
    memcpy(g2, b1, 192);
    memcpy(g2 + 192, b2, 192);
    Scope scope;
    ps_points **p1 = scope.points(), **p2 = scope.points();
    int rc = ps_points_upload(c, PS_G1, g1, 2, PS_FMT_AFFINE, p1);
    if (!rc) rc = ps_points_upload(c, PS_G2, g2, 2, PS_FMT_AFFINE, p2);
    if (!rc) rc = ps_pairing_product_is_one(c, *p1, *p2, 1, equal);
    return rc;
}
static bool points_same_view(const ps_points* a, const ps_points* b) { return a->st == b->st && a->first == b->first && a->n == b->n && a->group == b->group; }
static int points_bytes_equal(ps_ctx* c, const ps_points* a, const ps_points* b, bool* equal) {
    *equal = false;
    if (!a || !b) { *equal = a == b; return PS_OK; }
    if (a->n != b->n || a->group != b->group) return PS_OK;
    if (points_same_view(a, b)) { *equal = true; return PS_OK; }
    const size_t bytes = wire_bytes(a->group) * a->n;
    std::vector<uint8_t> ha(bytes), hb(bytes);
    int rc = ps_points_download(c, a, 0, a->n, ha.data());
    if (!rc) rc = ps_points_download(c, b, 0, b->n, hb.data());
    if (!rc) *equal = ha == hb;
    return rc;
}

extern "C" int ps_groth16_crs_check_update(ps_ctx* c, const ps_groth16_crs* before, const ps_groth16_crs* after, const uint8_t* rho_be32, size_t nrho,
                                           int* ok) {
    if (!c || !before || !after || !ok || (nrho && !rho_be32)) return fail(PS_ERR_ARG, "ps_groth16_crs_check_update: NULL argument");
    *ok = 0;
    for (const ps_groth16_crs* k : {before, after})
        if (!k->xi || !k->xi2 || !k->io_lp || !k->nio_lp || !k->xi_t) return fail(PS_ERR_ARG, "ps_groth16_crs_check_update: a key lacks an array");
    if (c->q_len) return fail(PS_ERR_ARG, "ps_groth16_crs_check_update: sums are pending on this context (ps_msm_finish them first)");
    // the arrays a share scales, with the G2 point that carries the inverse factor
    struct Scaled { const ps_points *was, *is; const uint8_t *was2, *is2; };
    const Scaled scaled[4] = {{before->nio_lp, after->nio_lp, before->delta2, after->delta2},
                              {before->xi_t, after->xi_t, before->delta2, after->delta2},
                              {before->lxi_t, after->lxi_t, before->delta2, after->delta2},
                              {before->io_lp, after->io_lp, before->gamma, after->gamma}};
    size_t longest = 0;
    for (const Scaled& s : scaled) {
        if (!s.was != !s.is) return PS_OK;  // (lxi_t is optional: on both sides or on neither)
        if (!s.was) continue;
        if (s.was->n != s.is->n) return PS_OK;
        longest = std::max(longest, s.was->n);
    }
    if (nrho < longest)
        return fail(PS_ERR_LENGTH, "ps_groth16_crs_check_update: " + std::to_string(nrho) + " weights for arrays of up to " + std::to_string(longest) + " points");
    for (size_t i = 0; i < longest; i++) {
        u32 w[8];
        if (!be32_to_words(w, rho_be32 + 32 * i)) return fail(PS_ERR_ENCODING, "ps_groth16_crs_check_update: rho[" + std::to_string(i) + "] is not below r");
    }
    HIP_TRY(hipSetDevice(c->device));
    // what no share touches is byte-equal
    if (memcmp(before->alpha, after->alpha, 96) || memcmp(before->beta, after->beta, 96) || memcmp(before->beta2, after->beta2, 192)) return PS_OK;
    const std::pair<const ps_points*, const ps_points*> same[4] = {
        {before->xi, after->xi}, {before->xi2, after->xi2}, {before->lxi, after->lxi}, {before->lxi2, after->lxi2}};
    for (const auto& s : same) {
        bool eq = false;
        int rc = points_bytes_equal(c, s.first, s.second, &eq);
        if (rc) return rc;
        if (!eq) return PS_OK;
    }
    // e(delta', G2) == e(G1, delta2'): the two forms of the new delta agree
    uint8_t gen1[96], gen2[192];
    generator_bytes<Fp>(gen1);
    generator_bytes<Fp2>(gen2);
    int eq = 0;
    int rc = pairing_pair_equal(c, after->delta, gen2, gen1, after->delta2, &eq);
    if (rc) return rc;
    if (!eq) return PS_OK;
    // e(sum rho_i N'_i, delta2') == e(sum rho_i N_i, delta2), and likewise IoLP against gamma: one random linear combination per array
    Scope scope;
    ps_scalars** rho = scope.scalars();
    if (longest && (rc = ps_scalars_upload(c, rho_be32, longest, rho))) return rc;
    for (const Scaled& s : scaled) {
        if (!s.was || !s.was->n) continue;
        ps_scalars** view = scope.scalars();
        uint8_t was_sum[96], is_sum[96];
        if ((rc = ps_scalars_slice(*rho, 0, s.was->n, view)) || (rc = ps_msm(c, s.was, *view, was_sum)) || (rc = ps_msm(c, s.is, *view, is_sum)) ||
            (rc = pairing_pair_equal(c, is_sum, s.is2, was_sum, s.was2, &eq)) || !eq)
            return rc;
    }
    *ok = 1;
    return PS_OK;
}
