// KZG polynomial commitments over the powers-of-tau string (included by capi.hip behind crs_check.inc):
//   ps_poly_scan_tile       the tile of the scan, for tests that sit on its edges
//   ps_poly_eval            y[j] = p(z_j)                                       <- Poly.Eval (algebra.go:107-115)
//   ps_poly_div_linear      q_j = (p - p(z_j)) / (X - z_j), rem[j] = p(z_j)     <- Poly.Div  (algebra.go:119-137) by (1, -z)
//   ps_kzg_commit           sum_i p_i tau_g1[i]                                 <- Poly.Commit: ps_msm over a slice
//   ps_kzg_open             values and proofs [q_j(tau)] G1 of k points: the scan, then ONE ps_msm_batch of the k quotient rows
//   ps_kzg_verify           e(C - y G1 + z pi, G2) == e(pi, tau G2), on the host (pairing.inc)
//   ps_kzg_verify_batch     k openings under one string by random linear combination: two sums, one two-pair product
// The only kernels are the three of poly_scan.hpp; everything else is made of existing entry points.

// {z_j^(2^i)}, i < POLY_SCAN_POWERS, for k canonical points (PS_ERR_ENCODING otherwise)
static int poly_scan_tables(const char* who, const uint8_t* z_be32, size_t k, std::vector<FrPow2Table>* tabs) {
    tabs->assign(k, FrPow2Table());
    for (size_t j = 0; j < k; j++) {
        FrPow2Table& t = (*tabs)[j];  // (the entries the kernels do not read stay zero)
        if (!fr_mont_from_canonical_be32(&t.p[0], z_be32 + 32 * j)) return fail(PS_ERR_ENCODING, std::string(who) + ": z[" + std::to_string(j) + "] is not below r");
        for (int i = 1; i < POLY_SCAN_POWERS; i++) t.p[i] = fr_mul(t.p[i - 1], t.p[i - 1]);
    }
    return PS_OK;
}
static void words_to_be32(uint8_t* be, const u32* w) {
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) be[31 - 4 * i - b] = (uint8_t)(w[i] >> (8 * b));
}

// The three launches for k points over p (n >= 1 coefficients): y_be32[j] = p(z_j); q_words != nullptr (n >= 2): row j of
// q_words = the n - 1 quotient coefficients by (X - z_j).  Returns with the stream idle.
static int poly_scan_run(ps_ctx* c, const char* who, const ps_scalars* p, const std::vector<FrPow2Table>& tabs, u32* q_words, uint8_t* y_be32) {
    const u64 n = p->n, k = tabs.size();
    const u32 tiles = (u32)poly_scan_tiles(n);
    hipStream_t st = c->stream;
    Scope scope(st);
    FrPow2Table* d_tabs = nullptr;
    Fr *totals = nullptr, *carries = nullptr;
    u32* d_y = nullptr;
    hipError_t e;
    if ((e = scope.device(&d_tabs, k)) != hipSuccess || (e = scope.device(&totals, poly_scan_total_elems(n, k))) != hipSuccess ||
        (e = scope.device(&carries, poly_scan_total_elems(n, k))) != hipSuccess || (e = scope.device(&d_y, poly_scan_value_words(k))) != hipSuccess)
        return fail(PS_ERR_HIP, std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    if (storage_wait_ready(p->st, st)) return fail(PS_ERR_HIP, std::string(who) + ": event wait failed");
    if ((e = hipMemcpyAsync(d_tabs, tabs.data(), sizeof(FrPow2Table) * k, hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(PS_ERR_HIP, std::string(who) + ": copy of the power tables: " + hipGetErrorString(e));
    const u32* coef = scalars_ptr(p);
    for (u64 j0 = 0; j0 < k; j0 += POLY_SCAN_MAX_POINTS_PER_LAUNCH) {  // blockIdx.y picks the point
        const u32 kb = (u32)std::min<u64>(k - j0, POLY_SCAN_MAX_POINTS_PER_LAUNCH);
        Fr* tot = totals + j0 * tiles;
        Fr* car = carries + j0 * tiles;
        hipLaunchKernelGGL(k_poly_scan_tile<false>, dim3(tiles, kb), dim3(POLY_SCAN_THREADS), 0, st, coef, n, tiles, (const FrPow2Table*)(d_tabs + j0), tot,
                           (const Fr*)nullptr, (u32*)nullptr);
        hipLaunchKernelGGL(k_poly_scan_carries, dim3(kb), dim3(POLY_SCAN_THREADS), 0, st, (const Fr*)tot, car, tiles, (const FrPow2Table*)(d_tabs + j0),
                           d_y + 8 * j0);
        if (q_words)
            hipLaunchKernelGGL(k_poly_scan_tile<true>, dim3(tiles, kb), dim3(POLY_SCAN_THREADS), 0, st, coef, n, tiles, (const FrPow2Table*)(d_tabs + j0),
                               (Fr*)nullptr, (const Fr*)car, q_words + 8 * j0 * (n - 1));
    }
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, std::string(who) + ": kernels: " + hipGetErrorString(e));
    std::vector<u32> y(8 * k);
    if ((e = hipMemcpyAsync(y.data(), d_y, 32 * k, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(PS_ERR_HIP, std::string(who) + ": run: " + hipGetErrorString(e));
    for (u64 j = 0; j < k; j++) words_to_be32(y_be32 + 32 * j, y.data() + 8 * j);
    return scope.finish(PS_OK);
}

// Arguments shared by ps_poly_eval, ps_poly_div_linear and ps_kzg_open; *skip: k == 0, nothing to do
static int poly_scan_args(const char* who, const ps_ctx* c, const ps_scalars* p, const uint8_t* z_be32, size_t k, const uint8_t* y_be32, bool* skip) {
    *skip = false;
    if (!c || !p) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    if (p->n == 0) return fail(PS_ERR_LENGTH, std::string(who) + ": empty polynomial");
    if (k == 0) { *skip = true; return PS_OK; }
    if (!z_be32 || !y_be32) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    if (!poly_scan_total_ok(p->n, k))
        return fail(PS_ERR_ARG, std::string(who) + ": " + std::to_string(k) + " points x " + std::to_string(p->n) + " coefficients reach 2^32 (split the points)");
    return PS_OK;
}

extern "C" int ps_poly_scan_tile(void) { return POLY_SCAN_TILE; }

extern "C" int ps_poly_eval(ps_ctx* c, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32) {
    const char* who = "ps_poly_eval";
    bool skip;
    int rc = poly_scan_args(who, c, p, z_be32, k, y_be32, &skip);
    if (rc || skip) return rc;
    std::vector<FrPow2Table> tabs;
    if ((rc = poly_scan_tables(who, z_be32, k, &tabs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return poly_scan_run(c, who, p, tabs, nullptr, y_be32);
}

// a fresh vector of `count` scalars, contents unspecified
static int scalars_fresh(ps_ctx* c, const char* who, u64 count, ps_scalars** out) {
    void* raw = nullptr;
    hipError_t e = hipMalloc(&raw, std::max<size_t>(32 * count, 32));
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string(who) + ": hipMalloc of " + std::to_string(32 * count) + " bytes: " + hipGetErrorString(e));
    *out = scalars_adopt(c, raw, count);
    return PS_OK;
}

extern "C" int ps_poly_div_linear(ps_ctx* c, const ps_scalars* p, const uint8_t* z_be32, size_t k, ps_scalars** q, uint8_t* rem_be32) {
    const char* who = "ps_poly_div_linear";
    if (!q) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    *q = nullptr;
    bool skip;
    int rc = poly_scan_args(who, c, p, z_be32, k, rem_be32, &skip);
    if (rc) return rc;
    if (p->n < 2) return fail(PS_ERR_LENGTH, std::string(who) + ": a constant has no quotient to hold (ps_poly_eval gives its value)");
    std::vector<FrPow2Table> tabs;
    if (!skip && (rc = poly_scan_tables(who, z_be32, k, &tabs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    if ((rc = scalars_fresh(c, who, (u64)k * (p->n - 1), scope.result(q)))) return rc;  // k == 0: an empty vector
    if (!skip && (rc = poly_scan_run(c, who, p, tabs, (u32*)(*q)->st->p, rem_be32))) return rc;
    return scope.finish(PS_OK);
}

static int kzg_string_args(const char* who, const ps_ctx* c, const ps_points* tau_g1, const ps_scalars* p) {
    if (!c || !tau_g1 || !p) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    if (tau_g1->group != PS_G1) return fail(PS_ERR_ARG, std::string(who) + ": tau_g1 is a G1 array");
    if (p->n == 0) return fail(PS_ERR_LENGTH, std::string(who) + ": empty polynomial");
    if (tau_g1->n < p->n)  // BlindEval's panic (algebra.go:350-352)
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(p->n) + " and the " + std::to_string(tau_g1->n) + " powers of the string");
    if (c->q_len) return fail(PS_ERR_ARG, std::string(who) + ": sums are pending on this context (ps_msm_finish them first)");
    return PS_OK;
}

extern "C" int ps_kzg_commit(ps_ctx* c, const ps_points* tau_g1, const ps_scalars* p, uint8_t* out) {
    int rc = kzg_string_args("ps_kzg_commit", c, tau_g1, p);
    if (rc) return rc;
    if (!out) return fail(PS_ERR_ARG, "ps_kzg_commit: NULL argument");
    Scope scope;
    ps_points** head = scope.points();
    if ((rc = ps_points_slice(tau_g1, 0, p->n, head))) return rc;
    return ps_msm(c, *head, p, out);
}

extern "C" int ps_kzg_open(ps_ctx* c, const ps_points* tau_g1, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32, uint8_t* proofs) {
    const char* who = "ps_kzg_open";
    int rc = kzg_string_args(who, c, tau_g1, p);
    if (rc) return rc;
    bool skip;
    if ((rc = poly_scan_args(who, c, p, z_be32, k, y_be32, &skip)) || skip) return rc;
    if (!proofs) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    std::vector<FrPow2Table> tabs;
    if ((rc = poly_scan_tables(who, z_be32, k, &tabs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = p->n;
    if (n == 1) {  // a constant: its own value at every point, and the quotient is zero
        if ((rc = ps_scalars_download(c, p, 0, 1, y_be32))) return rc;
        for (size_t j = 0; j < k; j++) {
            if (j) memcpy(y_be32 + 32 * j, y_be32, 32);
            write_identity(PS_G1, proofs + 96 * j);
        }
        return PS_OK;
    }
    Scope scope(c->stream);
    ps_scalars** q = scope.scalars();
    ps_points** head = scope.points();
    if ((rc = scalars_fresh(c, who, (u64)k * (n - 1), q))) return rc;
    if ((rc = poly_scan_run(c, who, p, tabs, (u32*)(*q)->st->p, y_be32))) return rc;
    if ((rc = ps_points_slice(tau_g1, 0, n - 1, head))) return rc;
    return scope.finish(ps_msm_batch(c, *head, *q, k, proofs));  // the quotient rows never leave the device
}

// (r - v) mod r for a canonical v, as big-endian bytes
static void be32_negated(uint8_t* out, const uint8_t* v_be32) {
    Fr v;
    (void)fr_mont_from_canonical_be32(&v, v_be32);
    fr_mont_to_be32(out, fr_neg(v));
}

extern "C" int ps_kzg_verify(const uint8_t* tau_g2_1, const uint8_t* commit, const uint8_t* z_be32, const uint8_t* y_be32, const uint8_t* proof, int* ok) {
    const char* who = "ps_kzg_verify";
    if (!tau_g2_1 || !commit || !z_be32 || !y_be32 || !proof || !ok) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    *ok = 0;
    u32 w[8];
    if (!be32_to_words(w, z_be32) || !be32_to_words(w, y_be32)) return fail(PS_ERR_ENCODING, std::string(who) + ": z and y must be below r");
    Affine<Fp> cm, pi, lhs;
    Affine<Fp2> t2;
    if (!read_g1(cm, commit) || !read_g1(pi, proof) || !read_g2(t2, tau_g2_1))
        return fail(PS_ERR_ENCODING, std::string(who) + ": a point is not a canonical point on the curve");
    if (!all_in_subgroup({&cm, &pi}, {&t2})) return PS_OK;
    // C - y G1 + z pi
    uint8_t pts[3 * 96], sc[3 * 32], sum[96];
    memcpy(pts, commit, 96);
    generator_bytes<Fp>(pts + 96);
    memcpy(pts + 192, proof, 96);
    memset(sc, 0, 32);
    sc[31] = 1;
    be32_negated(sc + 32, y_be32);
    memcpy(sc + 64, z_be32, 32);
    int rc = ps_points_lincomb(PS_G1, pts, sc, 3, sum);
    if (rc) return rc;
    if (!read_g1(lhs, sum)) return fail(PS_ERR_ENCODING, std::string(who) + ": internal: the combined point does not decode");
    *ok = product_is_one({{lhs, generator((const Fp2*)0)}, {pairing_dev::neg_g1(pi), t2}}) ? 1 : 0;
    return PS_OK;
}

extern "C" int ps_kzg_verify_batch(ps_ctx* c, const uint8_t* tau_g2_1, const uint8_t* commits, const uint8_t* z_be32, const uint8_t* y_be32,
                                   const uint8_t* proofs, const uint8_t* rho_be32, size_t k, int check_subgroup, int* ok) {
    const std::string who = "ps_kzg_verify_batch";
    if (!c || !tau_g2_1 || !ok || (k && (!commits || !z_be32 || !y_be32 || !proofs || !rho_be32))) return fail(PS_ERR_ARG, who + ": NULL argument");
    *ok = 0;
    if (k > PS_VERIFY_BATCH_MAX) return fail(PS_ERR_ARG, who + ": more than 2^24 openings (split the batch: the verdicts of the parts AND together)");
    if (c->q_len) return fail(PS_ERR_ARG, who + ": sums are pending on this context (ps_msm_finish them first)");
    Affine<Fp2> t2;
    if (!read_g2(t2, tau_g2_1)) return fail(PS_ERR_ENCODING, who + ": tau_g2_1 is not a canonical point on the curve");
    u32 rho_sum[8];
    int rc = batch_weights(who, rho_be32, k, rho_sum);
    if (rc) return rc;
    // the scalars of the two sums, [rho_j | rho_j z_j], and s = sum_j rho_j y_j, on the host
    std::vector<uint8_t> sc(64 * k);
    Fr s = fr_zero();
    for (size_t j = 0; j < k; j++) {
        Fr z, y;
        if (!fr_mont_from_canonical_be32(&z, z_be32 + 32 * j) || !fr_mont_from_canonical_be32(&y, y_be32 + 32 * j))
            return fail(PS_ERR_ENCODING, who + ": z[" + std::to_string(j) + "] or y[" + std::to_string(j) + "] is not below r");
        const Fr rho = fr_mont_from_be32(rho_be32 + 32 * j);
        memcpy(sc.data() + 32 * j, rho_be32 + 32 * j, 32);
        fr_mont_to_be32(sc.data() + 32 * (k + j), fr_mul(rho, z));
        s = fr_reduce(fr_add(s, fr_mul(rho, y)));
    }
    if (k == 0) { *ok = 1; return PS_OK; }
    HIP_TRY(hipSetDevice(c->device));
    // the points [C_0 .. C_{k-1} | pi_0 .. pi_{k-1}]: the upload validates encodings and the curve equation
    std::vector<uint8_t> raw(2 * 96 * k);
    memcpy(raw.data(), commits, 96 * k);
    memcpy(raw.data() + 96 * k, proofs, 96 * k);
    Scope scope;
    ps_points **all = scope.points(), **pis = scope.points();
    ps_scalars **w = scope.scalars(), **rho = scope.scalars();
    if ((rc = ps_points_upload(c, PS_G1, raw.data(), 2 * k, PS_FMT_AFFINE, all))) return rc;
    if (check_subgroup) {
        int in = 0;
        if (!all_in_subgroup({}, {&t2})) return PS_OK;
        if ((rc = ps_points_check_subgroup(c, *all, &in)) || !in) return rc;
    }
    if ((rc = ps_scalars_upload(c, sc.data(), 2 * k, w)) || (rc = ps_points_slice(*all, k, k, pis)) || (rc = ps_scalars_slice(*w, 0, k, rho))) return rc;
    // A = sum_j rho_j (C_j + z_j pi_j) - s G1,  B = sum_j rho_j pi_j:   e(A, G2) e(-B, tau G2) == 1
    uint8_t two[2 * 96], coef[2 * 32], a_bytes[96], b_bytes[96];
    if ((rc = ps_msm(c, *all, *w, two)) || (rc = ps_msm(c, *pis, *rho, b_bytes))) return rc;
    generator_bytes<Fp>(two + 96);
    memset(coef, 0, 32);
    coef[31] = 1;
    fr_mont_to_be32(coef + 32, fr_neg(s));
    if ((rc = ps_points_lincomb(PS_G1, two, coef, 2, a_bytes))) return rc;
    Affine<Fp> a, b;
    if (!read_g1(a, a_bytes) || !read_g1(b, b_bytes)) return fail(PS_ERR_ENCODING, who + ": internal: a sum does not decode");
    *ok = product_is_one({{a, generator((const Fp2*)0)}, {pairing_dev::neg_g1(b), t2}}) ? 1 : 0;
    return PS_OK;
}
