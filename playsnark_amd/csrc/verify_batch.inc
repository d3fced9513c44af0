// Pairing products on the device and the batch verifier built on them (included by capi.hip after pairing.inc and
// pairing_dev.hpp):
//   ps_pairing_product_is_one   prod_i e(P_i, Q_i) == 1 for device-resident arrays
//   ps_groth16_verify_batch     Groth16Verify (groth16.go:214-233) for N proofs under one key by a random linear combination
// The N Miller loops with distinct G2 arguments and their product run on the device (k_miller_batch, k_f12_product); the
// three loops whose G2 argument is a key point, and the ONE final exponentiation, run on the host as in pairing.inc.
// Staging memory is context buffers (DevBuf), not the stream-ordered pool: see batch_to_affine in capi.hip.
// The body of ps_groth16_verify_batch is verify_batch_impl, which ps_groth16_verify_batch_locate (verify_locate.inc) calls too.

constexpr size_t PS_VERIFY_BATCH_MAX = (size_t)1 << 24;

// SIMDs of the context's device (four per compute unit on CDNA)
static int ctx_simds(ps_ctx* c, u32* out) {
    if (!c->simds) {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->simds = (u32)std::max(1, cus) * 4u;
    }
    *out = c->simds;
    return PS_OK;
}

// Wall clock of the stages of the last ps_groth16_verify_batch on a context with ps_ctx_set_timing on (the stream is then
// drained at every stage boundary, so the stages do not overlap and the call is slower than an untimed one):
// [0] key checks, upload and subgroup tests of A, B, C  [1] rho, rho_i A_i  [2] k_miller_batch  [3] the product tree
// [4] column sums and the two sums over points  [5] host: download, three Miller loops, final exponentiation.
// Test / measurement hook, not in the header (like ps_debug_points_scale).
constexpr int PS_VB_STAGES = 6;
struct VbClock {
    ps_ctx* c;
    float* ms;  // the stage times of the entry point this clock serves (c->vb_ms; c->pvb_ms for ps_phgr13_verify_batch)
    std::chrono::steady_clock::time_point t0;
    VbClock(ps_ctx* ctx, float* stage_ms, int stages) : c(ctx), ms(stage_ms), t0(std::chrono::steady_clock::now()) {
        if (c->timing) for (int i = 0; i < stages; i++) ms[i] = 0;
    }
    void mark(int stage) {  // everything enqueued so far belongs to `stage`
        if (!c->timing) return;
        (void)hipStreamSynchronize(c->stream);
        const auto t1 = std::chrono::steady_clock::now();
        ms[stage] += std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};
extern "C" int ps_debug_verify_batch_stage_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "ps_debug_verify_batch_stage_ms: NULL argument");
    for (int i = 0; i < PS_VB_STAGES; i++) ms[i] = c->vb_ms[i];
    return PS_OK;
}

// prod_i miller(g1[i], g2[i]) for device arrays of n >= 1 pairs: enqueue on c->stream (the value stays on the device, *res),
// then fetch it into the host field.  Work enqueued between the two overlaps the download's wait.
static int miller_product_launch(ps_ctx* c, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, const pairing_dev::Fp12** res,
                                 VbClock* clk = nullptr) {
    typedef pairing_dev::Fp12 D12;
    u32 simds = 0;
    int rc = ctx_simds(c, &simds);
    if (rc) return rc;
    const size_t half = (n + 1) / 2;
    if ((rc = c->vb_f12.ensure(sizeof(D12) * (n + half)))) return rc;
    D12* a = (D12*)c->vb_f12.p;
    D12* b = a + n;
    u32 lpw = pairing_dev::spread_lanes(n, simds);
    hipLaunchKernelGGL(k_miller_batch, dim3((unsigned)((n + lpw - 1) / lpw)), dim3(64), 0, c->stream, g1, g2, (u32)n, lpw, a);
    if (clk) clk->mark(2);
    size_t m = n;
    while (m > 1) {  // tree product, ping-pong between the two parts of the buffer
        const size_t h = (m + 1) / 2;
        lpw = pairing_dev::spread_lanes(h, simds);
        hipLaunchKernelGGL(k_f12_product, dim3((unsigned)((h + lpw - 1) / lpw)), dim3(64), 0, c->stream, (const D12*)a, (u32)m, lpw, b);
        std::swap(a, b);
        m = h;
    }
    HIP_TRY(hipGetLastError());
    if (clk) clk->mark(3);
    *res = a;
    return PS_OK;
}
static int miller_product_fetch(ps_ctx* c, const pairing_dev::Fp12* res, pairing::Fp12* out) {
    pairing_dev::Fp12 f;
    HIP_TRY(hipMemcpyAsync(&f, res, sizeof(f), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = f12_to_host(f);
    return PS_OK;
}
static int miller_product(ps_ctx* c, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, pairing::Fp12* out) {
    const pairing_dev::Fp12* res = nullptr;
    int rc = miller_product_launch(c, g1, g2, n, &res);
    return rc ? rc : miller_product_fetch(c, res, out);
}

extern "C" int ps_pairing_product_is_one(ps_ctx* c, const ps_points* g1, const ps_points* g2, int check, int* is_one) {
    if (!c || !g1 || !g2 || !is_one) return fail(PS_ERR_ARG, "ps_pairing_product_is_one: NULL argument");
    *is_one = 0;
    if (g1->group != PS_G1 || g2->group != PS_G2) return fail(PS_ERR_ARG, "ps_pairing_product_is_one: needs a G1 array and a G2 array");
    if (g1->n != g2->n)
        return fail(PS_ERR_LENGTH, "ps_pairing_product_is_one: " + std::to_string(g1->n) + " G1 points against " + std::to_string(g2->n) + " G2 points");
    if (g1->n > PS_VERIFY_BATCH_MAX) return fail(PS_ERR_ARG, "ps_pairing_product_is_one: more than 2^24 pairs");
    if (g1->n == 0) { *is_one = 1; return PS_OK; }
    HIP_TRY(hipSetDevice(c->device));
    if (check) {
        for (const ps_points* p : {g1, g2}) {
            int ok = 0;
            int rc = ps_points_check_subgroup(c, p, &ok);
            if (rc) return rc;
            if (!ok) return fail(PS_ERR_ENCODING, std::string("ps_pairing_product_is_one: a ") + (p == g1 ? "G1" : "G2") + " point is outside the order-r subgroup");
        }
    }
    if (storage_wait_ready(g1->st, c->stream) || storage_wait_ready(g2->st, c->stream))
        return fail(PS_ERR_HIP, "ps_pairing_product_is_one: event wait failed");
    pairing::Fp12 f;
    int rc = miller_product(c, (const Affine<Fp>*)points_ptr(g1), (const Affine<Fp2>*)points_ptr(g2), g1->n, &f);
    if (rc) return rc;
    *is_one = pairing::f12_eq(pairing::final_exp(f), pairing::f12_one()) ? 1 : 0;
    return PS_OK;
}

// out[i] = k[i] * pts[i] (G1, affine in, affine out) by the GLV multiplication of the key conversion (k_ec_scale)
static int points_scale_g1(ps_ctx* c, const ps_points* pts, const Fr* k_mont, ps_points** out) {
    typedef KernelField<Fp>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = pts->n;
    int rc = c->vb_xyzz.ensure(batch_affine_tmp_bytes(n, sizeof(Xyzz<Fp>)));
    if (rc) return rc;
    Scope scope;
    if ((rc = points_alloc(c, PS_G1, n, scope.result(out)))) return rc;
    Xyzz<Fp>* buf = (Xyzz<Fp>*)c->vb_xyzz.p;
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks(n * LN)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(pts), (u32)n, (u32)n, buf);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks(n * LN)), dim3(256), 0, c->stream, buf, (u32)n, k_mont, ~0ull);
    batch_to_affine<Fp>(c->stream, (char*)buf, n, (char*)(*out)->st->p, (u32)sizeof(Affine<Fp>));
    if (hipGetLastError() != hipSuccess) return fail(PS_ERR_HIP, "ps_groth16_verify_batch: scaling kernels failed to launch");
    return scope.finish(PS_OK);
}

// t_j = sum_i w_i m_ij over a rows x cols matrix of plain scalars on the device; the result is row 0 of *res
static int weighted_columns(ps_ctx* c, const Fr* w_mont, const u32* m, size_t rows, size_t cols, const u32** res) {
    // Chunks of at least 64 rows, and no more chunks than it takes to put ~2^16 threads to work: a wide matrix (many public
    // inputs) is parallel over its columns already and gets few chunks, so the workspace stays near 32 B x 2^16 per pass.
    const size_t max_chunks = std::max<size_t>(1, std::min<size_t>(4096, (65536 + cols - 1) / cols));
    auto rows_per_chunk = [max_chunks](size_t r) { return std::max<size_t>(64, (r + max_chunks - 1) / max_chunks); };
    size_t total = 0;  // rows of every pass together: the buffer is sized once, nothing moves while kernels read it
    for (size_t r = rows;;) {
        const size_t chunks = (r + rows_per_chunk(r) - 1) / rows_per_chunk(r);
        total += chunks;
        if (chunks == 1) break;
        r = chunks;
    }
    int rc = c->vb_cols.ensure(32 * cols * total);
    if (rc) return rc;
    const u32* src = m;
    const Fr* w = w_mont;
    size_t r = rows, off = 0;
    while (true) {
        const size_t per = rows_per_chunk(r), chunks = (r + per - 1) / per;
        u32* dst = (u32*)c->vb_cols.p + 8 * cols * off;
        hipLaunchKernelGGL(k_fr_weighted_columns, dim3(nblocks(cols), (unsigned)chunks), dim3(256), 0, c->stream, w, src, (u32)r, (u32)cols,
                           (u32)per, dst);
        HIP_TRY(hipGetLastError());
        *res = dst;
        if (chunks == 1) return PS_OK;
        src = dst;
        w = nullptr;
        off += chunks;
        r = chunks;
    }
}

static bool be32_to_words(u32* w, const uint8_t* be) {  // false: not below r
    for (int i = 0; i < 8; i++) w[i] = ((u32)be[28 - 4 * i] << 24) | ((u32)be[29 - 4 * i] << 16) | ((u32)be[30 - 4 * i] << 8) | (u32)be[31 - 4 * i];
    for (int i = 7; i >= 0; i--)
        if (w[i] != FrParams::mod(i)) return w[i] < FrParams::mod(i);
    return false;
}
static void words_add_mod_r(u32* acc, const u32* x) {  // both below r < 2^255
    u64 carry = 0;
    for (int i = 0; i < 8; i++) { u64 s = (u64)acc[i] + x[i] + carry; acc[i] = (u32)s; carry = s >> 32; }
    u32 d[8];
    u64 borrow = 0;
    for (int i = 0; i < 8; i++) { u64 t = (u64)acc[i] - FrParams::mod(i) - borrow; d[i] = (u32)t; borrow = (t >> 63) & 1; }
    if (!borrow) memcpy(acc, d, sizeof(d));
}

// The weights of a batch: every rho_i canonical (PS_ERR_ENCODING) and non-zero (PS_ERR_ARG); sum = their sum mod r
static int batch_weights(const std::string& fn, const uint8_t* rho_be32, size_t n, u32* sum) {
    memset(sum, 0, 32);
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        if (!be32_to_words(w, rho_be32 + 32 * i)) return fail(PS_ERR_ENCODING, fn + ": rho[" + std::to_string(i) + "] is not below r");
        u32 any = 0;
        for (int k = 0; k < 8; k++) any |= w[k];
        if (!any) return fail(PS_ERR_ARG, fn + ": rho[" + std::to_string(i) + "] is zero (the proof would not be checked)");
        words_add_mod_r(sum, w);
    }
    return PS_OK;
}

// out = sum_j t_j pts_j with t_j = sum_i w_i io_ij over `rows` rows of pts->n plain scalars: ONE sum over the key's points
// instead of one per proof (pts->n == 0: the identity).  t lives in the caller's scope: freeing it here would synchronise
// the device, and the Miller loops enqueued before this sum are meant to run beside what follows it.
static int weighted_io_sum(ps_ctx* c, const std::string& fn, Scope& scope, const Fr* w_mont, const ps_scalars* io, size_t rows, const ps_points* pts,
                           uint8_t* out) {
    const size_t diff = pts->n;
    if (!diff) { write_identity(pts->group, out); return PS_OK; }
    if (storage_wait_ready(io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
    ps_scalars** t = scope.scalars();
    const u32* tw = nullptr;
    int rc = weighted_columns(c, w_mont, scalars_ptr(io), rows, diff, &tw);
    if (rc) return rc;
    if ((rc = scalars_alloc(c, diff, t))) return rc;
    if (hipMemcpyAsync((*t)->st->p, tw, 32 * diff, hipMemcpyDeviceToDevice, c->stream) != hipSuccess || storage_mark_ready((*t)->st, c->stream))
        return fail(PS_ERR_HIP, fn + ": copy of the column sums failed");
    return ps_msm(c, pts, *t, out);
}

template <class F>
static size_t first_bad_encoding(const std::vector<uint8_t>& raw, size_t n, size_t wb) {
    for (size_t i = 0; i < n; i++) {
        Affine<F> a;
        if (!read_affine(a, raw.data() + wb * i)) return i;
    }
    return n;
}

// What a REJECTED batch hands to the descent of ps_groth16_verify_batch_locate (verify_locate.inc) instead of freeing it:
// the C_i and rho on the device (owned by the holder from then on; rho in Montgomery form stays in c->vb_rho until the
// next call), and the key's points in the host field.
struct VbKeep {
    ps_points* c_pts = nullptr;
    ps_scalars* rho = nullptr;
    Affine<Fq> alpha;
    Affine<Fq2> g2[3];  // beta2, gamma, delta2
};
// verify_locate.inc: k_miller_batch and the product tree with every level kept (c->lc_f12); *res is the root
static int locate_miller_levels(ps_ctx* c, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, const pairing_dev::Fp12** res, VbClock* clk);

// The batch check behind ps_groth16_verify_batch (fn = its name, max_n = 2^24) and ps_groth16_verify_batch_locate (its own
// name and cap; keep != nullptr: the levels of the product tree are retained and a rejected batch fills *keep).  The
// caller has checked its pointers and set *ok = 0.
static int verify_batch_impl(ps_ctx* c, const std::string& fn, size_t max_n, const char* max_what, const ps_groth16_vk* vk, const ps_scalars* io,
                             const uint8_t* proofs, size_t nproofs, const uint8_t* rho_be32, int* ok, VbKeep* keep) {
    VbClock clk(c, c->vb_ms, PS_VB_STAGES);
    if (c->q_len) return fail(PS_ERR_ARG, fn + ": sums are pending on this context (ps_msm_finish them first)");
    if (nproofs > max_n) return fail(PS_ERR_ARG, fn + ": more than " + max_what + " proofs in one batch");
    const size_t N = nproofs, diff = vk->io_lp->n;
    if (io->n != N * diff)
        return fail(PS_ERR_LENGTH, fn + ": " + std::to_string(io->n) + " public inputs for " + std::to_string(N) + " proofs of " +
                                       std::to_string(diff) + " each");
    if (N == 0) { *ok = 1; return PS_OK; }
    // weights: canonical, non-zero; their sum for the alpha term
    u32 rho_sum[8];
    int rc = batch_weights(fn, rho_be32, N, rho_sum);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the key: as in ps_groth16_verify
    if ((rc = vk_array_in_subgroup(c, vk->io_lp, fn.c_str()))) return rc;
    Affine<Fp> alpha;
    Affine<Fp2> beta2, gamma, delta2;
    if (!read_g1(alpha, vk->alpha) || !read_g2(beta2, vk->beta2) || !read_g2(gamma, vk->gamma) || !read_g2(delta2, vk->delta2))
        return fail(PS_ERR_ENCODING, fn + ": bad point encoding in the verification key");
    if (!all_in_subgroup({&alpha}, {&beta2, &gamma, &delta2}))
        return fail(PS_ERR_ENCODING, fn + ": verification-key point outside the order-r subgroup");
    // the proofs: three arrays through the validating upload, then [r]P on the device
    std::vector<uint8_t> raw[3];
    const size_t wbs[3] = {96, 192, 96}, offs[3] = {0, 96, 288};
    const int groups[3] = {PS_G1, PS_G2, PS_G1};
    const char* names[3] = {"A", "B", "C"};
    Scope scope;
    ps_points** arr[3] = {scope.points(), scope.points(), scope.points()};
    ps_points** ra = scope.points();
    ps_scalars** rho = scope.scalars();
    for (int k = 0; k < 3; k++) {
        raw[k].resize(wbs[k] * N);
        for (size_t i = 0; i < N; i++) memcpy(raw[k].data() + wbs[k] * i, proofs + 384 * i + offs[k], wbs[k]);
        rc = ps_points_upload(c, groups[k], raw[k].data(), N, PS_FMT_AFFINE, arr[k]);
        if (rc == PS_ERR_ENCODING) {
            const size_t bad = groups[k] == PS_G1 ? first_bad_encoding<Fp>(raw[k], N, 96) : first_bad_encoding<Fp2>(raw[k], N, 192);
            return fail(PS_ERR_ENCODING, fn + ": " + names[k] + " of proof " + std::to_string(bad) +
                                                  " is not a canonical point on the curve");
        }
        if (rc) return rc;
    }
    for (int k = 0; k < 3; k++) {
        int in = 0;
        if ((rc = ps_points_check_subgroup(c, *arr[k], &in))) return rc;
        if (!in) return fail(PS_ERR_ENCODING, fn + ": a proof's " + names[k] + " is outside the order-r subgroup");
    }
    clk.mark(0);
    // rho on the device: plain words for the sum over C, Montgomery form for the scaling of A and the column sums
    if ((rc = ps_scalars_upload(c, rho_be32, N, rho))) return rc;
    if ((rc = c->vb_rho.ensure(sizeof(Fr) * N))) return rc;
    Fr* rho_m = (Fr*)c->vb_rho.p;
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(N)), dim3(256), 0, c->stream, rho_m, scalars_ptr(*rho), (u64)N);
    // the device's share: prod_i miller(rho_i A_i, B_i)
    if ((rc = points_scale_g1(c, *arr[0], rho_m, ra))) return rc;
    clk.mark(1);
    const pairing_dev::Fp12* fdev = nullptr;
    rc = keep ? locate_miller_levels(c, (const Affine<Fp>*)points_ptr(*ra), (const Affine<Fp2>*)points_ptr(*arr[1]), N, &fdev, &clk)
              : miller_product_launch(c, (const Affine<Fp>*)points_ptr(*ra), (const Affine<Fp2>*)points_ptr(*arr[1]), N, &fdev, &clk);
    if (rc) return rc;
    // (the loops are only enqueued: the column sums and the two sums below queue up behind them while they run, and the
    // product is fetched after the sums)
    // X = sum_j (sum_i rho_i io_ij) IoLP_j and sum_i rho_i C_i: two sums instead of N
    uint8_t xb[96], cb[96];
    if ((rc = weighted_io_sum(c, fn, scope, rho_m, io, N, vk->io_lp, xb))) return rc;
    if ((rc = ps_msm(c, *arr[2], *rho, cb))) return rc;
    clk.mark(4);
    pairing::Fp12 f;
    if ((rc = miller_product_fetch(c, fdev, &f))) return rc;
    Affine<Fp> x, sc;
    if (!read_g1(x, xb) || !read_g1(sc, cb)) return fail(PS_ERR_ENCODING, fn + ": bad point from a sum");
    // the host's share: (-(sum rho) alpha, beta2), (-X, gamma), (-sum rho_i C_i, delta2), one final exponentiation
    typedef Affine<Fq> H1;
    H1 sa;
    {
        const H1 ha = affine_to_host<Fp>(alpha);
        sa.x = f_zero((const Fq*)0); sa.y = f_zero((const Fq*)0);
        if (!affine_is_identity<Fq>(ha)) {
            Xyzz<Fq> p = xyzz_mul_scalar<Fq>(xyzz_from_affine<Fq>(ha.x, ha.y), rho_sum);
            if (!xyzz_to_affine<Fq>(p, sa.x, sa.y)) { sa.x = f_zero((const Fq*)0); sa.y = f_zero((const Fq*)0); }
        }
    }
    const std::pair<H1, Affine<Fq2>> tail[3] = {{pairing::neg_g1(sa), affine_to_host<Fp2>(beta2)},
                                                {pairing::neg_g1(affine_to_host<Fp>(x)), affine_to_host<Fp2>(gamma)},
                                                {pairing::neg_g1(affine_to_host<Fp>(sc)), affine_to_host<Fp2>(delta2)}};
    std::future<pairing::Fp12> loops[3];
    for (int k = 0; k < 3; k++) loops[k] = std::async(std::launch::async, [&tail, k] { return pairing::miller(tail[k].first, tail[k].second); });
    for (auto& l : loops) f = pairing::f12_mul(f, l.get());
    *ok = pairing::f12_eq(pairing::final_exp(f), pairing::f12_one()) ? 1 : 0;
    clk.mark(5);
    if (keep && !*ok) {
        keep->c_pts = *arr[2];  // out of the scope's slots: the holder's from here on
        keep->rho = *rho;
        *arr[2] = nullptr;
        *rho = nullptr;
        keep->alpha = affine_to_host<Fp>(alpha);
        for (int k = 0; k < 3; k++) keep->g2[k] = tail[k].second;
    }
    return PS_OK;
}

extern "C" int ps_groth16_verify_batch(ps_ctx* c, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t* proofs, size_t nproofs,
                                       const uint8_t* rho_be32, int* ok) {
    if (!c || !vk || !io || !ok || !vk->io_lp || (nproofs && (!proofs || !rho_be32))) return fail(PS_ERR_ARG, "ps_groth16_verify_batch: NULL argument");
    *ok = 0;
    return verify_batch_impl(c, "ps_groth16_verify_batch", PS_VERIFY_BATCH_MAX, "2^24", vk, io, proofs, nproofs, rho_be32, ok, nullptr);
}
