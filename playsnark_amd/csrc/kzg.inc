// KZG polynomial commitments over the powers-of-tau string (included by capi.hip behind crs_check.inc):
//   ps_poly_scan_tile       the tile of the scan, for tests that sit on its edges
//   ps_poly_eval            y[j] = p(z_j)                                       <- Poly.Eval (algebra.go:107-115)
//   ps_poly_div_linear      q_j = (p - p(z_j)) / (X - z_j), rem[j] = p(z_j)     <- Poly.Div  (algebra.go:119-137) by (1, -z)
//   ps_kzg_commit           sum_i p_i tau_g1[i]                                 <- Poly.Commit: ps_msm over a slice
//   ps_kzg_open             values and proofs [q_j(tau)] G1 of k points: the scan, then ONE ps_msm_batch of the k quotient rows
//   ps_kzg_verify           e(C - y G1 + z pi, G2) == e(pi, tau G2), on the host (pairing.inc)
//   ps_kzg_verify_batch     k openings under one string by random linear combination: two sums, one two-pair product
//   ps_poly_div_roots       q = (p - r) / prod_j (X - z_j), the values, the remainder  <- Poly.Div  (algebra.go:119-137) by Z_S
//   ps_kzg_open_set         values and ONE proof [q(tau)] G1 for a set of k points: the scan's totals and carries, the set apply
//                           pass (poly_scan_set.hpp), then ONE lone ps_msm
//   ps_kzg_verify_set       e(C - [r(tau)] G1, G2) e(-pi, [Z_S(tau)] G2) == 1: r and Z_S on the host, two short sums, one product
//   ps_poly_lagrange_tile        the tile of the value-form kernels, for tests that sit on its edges
//   ps_qap_gate_values           the n values of (L|R|O).sol on the domain 1..n: ps_qap_interpolate without its interpolation
//   ps_poly_eval_lagrange        y[j] = p(z_j) from the n VALUES of p on 1..n: one inversion per workgroup, no interpolation
//   ps_poly_div_linear_lagrange  the values on 1..n of (p - p(z_j)) / (X - z_j), z_j on the domain or off it
//   ps_kzg_commit_lagrange       sum_i v_i lag_g1[i]: ps_msm over the Lagrange-form string
//   ps_kzg_open_lagrange         values and proofs of k points from the values: those rows, then the lone ps_msm (k = 1) or ONE
//                                ps_msm_batch over lag_g1 -- ps_kzg_open's bytes for the interpolated coefficients
//   ps_poly_lagrange_set_group   the points of a set that share one inversion per tile, for tests that sit on its edges
//   ps_poly_div_roots_lagrange   the values on 1..n of (p - r) / Z_S from the values of p: the k linear quotients folded into one row
//   ps_kzg_open_set_lagrange     values and ONE proof for a set of k points from the values: that row, then ONE lone ps_msm over
//                                lag_g1 -- ps_kzg_open_set's bytes for the interpolated coefficients
//   ps_kzg_all_key_lagrange      K_m = sum_i kappa(m - i) lag_g1[i], m = 1 .. n: the part of the proofs of all nodes that depends on
//                                the string alone -- one correlation over points (ec_correlate)
//   ps_kzg_open_all_lagrange     the proofs of ALL n nodes from the values: the scalar side, one correlation over points, one
//                                combining pass -- ps_kzg_open_lagrange's bytes at z = 1 .. n
// The kernels are the three of poly_scan.hpp, k_fr_lincomb (fr_lincomb.hpp), k_poly_scan_set_apply (poly_scan_set.hpp), the
// three of poly_lagrange.hpp, k_lagr_fold (poly_lagrange_set.hpp) and the five of kzg_all.hpp around the transforms of ntt.hpp
// and lagrange.hpp; everything else is made of existing entry points.

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
// row_len != 0: p holds k rows of row_len coefficients and point j meets ROW j -- the same kernels, launched once per row with a
// grid of one point, every pointer moved to the row's own (3 k launches; k is small where sums of milliseconds follow).
static int poly_scan_run(ps_ctx* c, const char* who, const ps_scalars* p, const std::vector<FrPow2Table>& tabs, u32* q_words, uint8_t* y_be32,
                         u64 row_len = 0) {
    const u64 n = row_len ? row_len : p->n, k = tabs.size();
    const u64 per_launch = row_len ? 1 : POLY_SCAN_MAX_POINTS_PER_LAUNCH;
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
    for (u64 j0 = 0; j0 < k; j0 += per_launch) {  // blockIdx.y picks the point
        const u32 kb = (u32)std::min<u64>(k - j0, per_launch);
        const u32* coef = scalars_ptr(p) + 8 * j0 * row_len;
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
    for (u64 j = 0; y_be32 && j < k; j++) words_to_be32(y_be32 + 32 * j, y.data() + 8 * j);
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

// The core of the combined checks: with the points [C_0 .. C_{nc-1} | pi_0 .. pi_{np-1}] and the scalars sc = [a_0 .. a_{nc+np-1} | ..]
// whose np entries from rho_at on are the weights rho_j,
//     A = sum_i a_i pts_i - s G1,  B = sum_j rho_j pi_j:   *ok = (e(A, G2) e(-B, tau G2) == 1)
// -- two sums over the uploaded points, one two-pair product.  The upload validates encodings and the curve equation.
static int kzg_check_sums(ps_ctx* c, const std::string& who, const Affine<Fp2>& t2, const uint8_t* commits, size_t nc, const uint8_t* proofs, size_t np,
                          const std::vector<uint8_t>& sc, size_t rho_at, const Fr& s, int check_subgroup, int* ok) {
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<uint8_t> raw(96 * (nc + np));
    memcpy(raw.data(), commits, 96 * nc);
    memcpy(raw.data() + 96 * nc, proofs, 96 * np);
    Scope scope;
    ps_points **all = scope.points(), **pis = scope.points();
    ps_scalars **w = scope.scalars(), **a = scope.scalars(), **rho = scope.scalars();
    if ((rc = ps_points_upload(c, PS_G1, raw.data(), nc + np, PS_FMT_AFFINE, all))) return rc;
    if (check_subgroup) {
        int in = 0;
        if (!all_in_subgroup({}, {&t2})) return PS_OK;
        if ((rc = ps_points_check_subgroup(c, *all, &in)) || !in) return rc;
    }
    if ((rc = ps_scalars_upload(c, sc.data(), sc.size() / 32, w)) || (rc = ps_points_slice(*all, nc, np, pis)) ||
        (rc = ps_scalars_slice(*w, 0, nc + np, a)) || (rc = ps_scalars_slice(*w, rho_at, np, rho)))
        return rc;
    uint8_t two[2 * 96], coef[2 * 32], a_bytes[96], b_bytes[96];
    if ((rc = ps_msm(c, *all, *a, two)) || (rc = ps_msm(c, *pis, *rho, b_bytes))) return rc;
    generator_bytes<Fp>(two + 96);
    memset(coef, 0, 32);
    coef[31] = 1;
    fr_mont_to_be32(coef + 32, fr_neg(s));
    if ((rc = ps_points_lincomb(PS_G1, two, coef, 2, a_bytes))) return rc;
    Affine<Fp> pa, pb;
    if (!read_g1(pa, a_bytes) || !read_g1(pb, b_bytes)) return fail(PS_ERR_ENCODING, who + ": internal: a sum does not decode");
    *ok = product_is_one({{pa, generator((const Fp2*)0)}, {pairing_dev::neg_g1(pb), t2}}) ? 1 : 0;
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
    // A = sum_j rho_j (C_j + z_j pi_j) - s G1,  B = sum_j rho_j pi_j:   e(A, G2) e(-B, tau G2) == 1
    return kzg_check_sums(c, who, t2, commits, k, proofs, k, sc, 0, s, check_subgroup, ok);
}

// ---- many polynomials at shared points: one proof per point ----

// An m x t matrix of canonical coefficients (PS_ERR_ENCODING otherwise) as the table k_fr_lincomb reads
static int lincomb_coefs(const std::string& who, const uint8_t* coef_be32, size_t m, size_t t, std::vector<FrLincombCoef>* out) {
    out->assign(m * t, FrLincombCoef());
    for (size_t e = 0; e < m * t; e++) {
        Fr v;
        if (!fr_mont_from_canonical_be32(&v, coef_be32 + 32 * e))
            return fail(PS_ERR_ENCODING, who + ": coefficient [" + std::to_string(e / t) + "][" + std::to_string(e % t) + "] is not below r");
        const Fr cv = fr_canon(v);
        u32 any = 0;
        for (int k = 0; k < FR_L; k++) { (*out)[e].l[k] = cv.l[k]; any |= (u32)cv.l[k]; }
        (*out)[e].nonzero = any ? 1 : 0;
    }
    return PS_OK;
}

// the checks on the inputs of a combination; *N = the longest
static int lincomb_inputs(const std::string& who, const ps_scalars* const* v, size_t m, u64* N) {
    if (!v || m == 0) return fail(PS_ERR_ARG, who + (v ? ": no input" : ": NULL argument"));
    *N = 0;
    for (size_t l = 0; l < m; l++) {
        if (!v[l]) return fail(PS_ERR_ARG, who + ": input " + std::to_string(l) + " is NULL");
        if (v[l]->n == 0) return fail(PS_ERR_LENGTH, who + ": input " + std::to_string(l) + " is empty");
        *N = std::max<u64>(*N, v[l]->n);
    }
    return PS_OK;
}
static int lincomb_size(const std::string& who, u64 m, u64 t, u64 N) {
    if (fr_lincomb_size_ok(m, t, N)) return PS_OK;
    return fail(PS_ERR_ARG, who + ": " + std::to_string(t) + " rows x " + std::to_string(N) + " scalars reach 2^32, or " + std::to_string(m) + " x " +
                                std::to_string(t) + " coefficients exceed 2^20 (split the rows)");
}

extern "C" int ps_scalars_lincomb(ps_ctx* c, const ps_scalars* const* v, size_t m, const uint8_t* coef_be32, size_t t, ps_scalars** out) {
    const std::string who = "ps_scalars_lincomb";
    if (!c || !out) return fail(PS_ERR_ARG, who + ": NULL argument");
    *out = nullptr;
    u64 N;
    int rc = lincomb_inputs(who, v, m, &N);
    if (rc) return rc;
    if (t && !coef_be32) return fail(PS_ERR_ARG, who + ": NULL argument");
    if ((rc = lincomb_size(who, m, t, N))) return rc;
    std::vector<FrLincombCoef> coefs;
    if ((rc = lincomb_coefs(who, coef_be32, m, t, &coefs))) return rc;
    std::vector<FrLincombInput> ins(m);
    for (size_t l = 0; l < m; l++) ins[l] = FrLincombInput{scalars_ptr(v[l]), v[l]->n};
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    Scope scope(st);
    if ((rc = scalars_fresh(c, who.c_str(), (u64)t * N, scope.result(out)))) return rc;
    if (t == 0) return scope.finish(PS_OK);  // an empty vector
    FrLincombInput* d_in = nullptr;
    FrLincombCoef* d_coef = nullptr;
    hipError_t e;
    if ((e = scope.device(&d_in, m)) != hipSuccess || (e = scope.device(&d_coef, m * t)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
    for (size_t l = 0; l < m; l++)
        if (storage_wait_ready(v[l]->st, st)) return fail(PS_ERR_HIP, who + ": event wait failed");
    if ((e = hipMemcpyAsync(d_in, ins.data(), sizeof(FrLincombInput) * m, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(d_coef, coefs.data(), sizeof(FrLincombCoef) * m * t, hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": copy of the tables: " + hipGetErrorString(e));
    const u64 groups = fr_lincomb_groups(t);
    for (u64 k = 0; k < fr_lincomb_launches(groups); k++)  // blockIdx.y picks the group of rows
        hipLaunchKernelGGL(k_fr_lincomb, dim3((u32)fr_lincomb_blocks(N), (u32)fr_lincomb_launch_groups(groups, k)), dim3(FR_LINCOMB_THREADS), 0, st,
                           (const FrLincombInput*)d_in, (u32)m, (const FrLincombCoef*)d_coef, (u32)t, (u32)(k * FR_LINCOMB_MAX_GROUPS_PER_LAUNCH), N,
                           (u32*)(*out)->st->p);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": run: " + hipGetErrorString(e));
    return scope.finish(PS_OK);
}

extern "C" int ps_kzg_open_multi(ps_ctx* c, const ps_points* tau_g1, const ps_scalars* const* polys, size_t m, const uint8_t* z_be32, size_t t,
                                 const uint8_t* coef_be32, uint8_t* y_be32, uint8_t* proofs) {
    const std::string who = "ps_kzg_open_multi";
    if (!c || !tau_g1) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (tau_g1->group != PS_G1) return fail(PS_ERR_ARG, who + ": tau_g1 is a G1 array");
    u64 N;
    int rc = lincomb_inputs(who, polys, m, &N);
    if (rc) return rc;
    if (tau_g1->n < N)
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(N) + " and the " + std::to_string(tau_g1->n) + " powers of the string");
    if (c->q_len) return fail(PS_ERR_ARG, who + ": sums are pending on this context (ps_msm_finish them first)");
    if (t == 0) return PS_OK;
    if (!z_be32 || !coef_be32 || !y_be32 || !proofs) return fail(PS_ERR_ARG, who + ": NULL argument");
    if ((rc = lincomb_size(who, m, t, N))) return rc;
    std::vector<FrLincombCoef> coefs;
    std::vector<FrPow2Table> tabs, mine;
    if ((rc = lincomb_coefs(who, coef_be32, m, t, &coefs)) || (rc = poly_scan_tables(who.c_str(), z_be32, t, &tabs))) return rc;
    for (size_t j = 0; j < t; j++) {
        bool any = false;
        for (size_t i = 0; i < m && !any; i++) any = coefs[i * t + j].nonzero != 0;
        if (!any) return fail(PS_ERR_ARG, who + ": no polynomial is opened at z[" + std::to_string(j) + "] (its column of coefficients is zero)");
    }
    HIP_TRY(hipSetDevice(c->device));
    // 1. values: one evaluation per polynomial, over the points of its non-zero entries
    memset(y_be32, 0, 32 * m * t);
    std::vector<size_t> at;
    std::vector<uint8_t> ys;
    for (size_t i = 0; i < m; i++) {
        at.clear();
        mine.clear();
        for (size_t j = 0; j < t; j++)
            if (coefs[i * t + j].nonzero) { at.push_back(j); mine.push_back(tabs[j]); }
        if (at.empty()) continue;
        ys.resize(32 * at.size());
        if ((rc = poly_scan_run(c, who.c_str(), polys[i], mine, nullptr, ys.data()))) return rc;
        for (size_t a = 0; a < at.size(); a++) memcpy(y_be32 + 32 * (i * t + at[a]), ys.data() + 32 * a, 32);
    }
    if (N == 1) {  // constants: every quotient is zero
        for (size_t j = 0; j < t; j++) write_identity(PS_G1, proofs + 96 * j);
        return PS_OK;
    }
    // 2. the rows f_j, 3. their quotients by (X - z_j), 4. ONE batched sum of the t quotient rows; nothing leaves the device
    Scope scope(c->stream);
    ps_scalars **f = scope.scalars(), **q = scope.scalars();
    ps_points** head = scope.points();
    if ((rc = ps_scalars_lincomb(c, polys, m, coef_be32, t, f))) return rc;
    if ((rc = scalars_fresh(c, who.c_str(), (u64)t * (N - 1), q))) return rc;
    if ((rc = poly_scan_run(c, who.c_str(), *f, tabs, (u32*)(*q)->st->p, nullptr, N))) return rc;
    if ((rc = ps_points_slice(tau_g1, 0, N - 1, head))) return rc;
    return scope.finish(ps_msm_batch(c, *head, *q, t, proofs));
}

extern "C" int ps_kzg_verify_multi(ps_ctx* c, const uint8_t* tau_g2_1, const uint8_t* commits, size_t m, const uint8_t* z_be32, size_t t,
                                   const uint8_t* coef_be32, const uint8_t* y_be32, const uint8_t* proofs, const uint8_t* rho_be32, int check_subgroup,
                                   int* ok) {
    const std::string who = "ps_kzg_verify_multi";
    if (!c || !tau_g2_1 || !ok || (t && (!commits || !z_be32 || !coef_be32 || !y_be32 || !proofs || !rho_be32))) return fail(PS_ERR_ARG, who + ": NULL argument");
    *ok = 0;
    if (m > PS_VERIFY_BATCH_MAX || t > PS_VERIFY_BATCH_MAX || m + t > PS_VERIFY_BATCH_MAX)
        return fail(PS_ERR_ARG, who + ": more than 2^24 commitments and points (split the points: the verdicts of the parts AND together)");
    if (c->q_len) return fail(PS_ERR_ARG, who + ": sums are pending on this context (ps_msm_finish them first)");
    Affine<Fp2> t2;
    if (!read_g2(t2, tau_g2_1)) return fail(PS_ERR_ENCODING, who + ": tau_g2_1 is not a canonical point on the curve");
    u32 rho_sum[8];
    int rc = batch_weights(who, rho_be32, t, rho_sum);
    if (rc) return rc;
    if (t == 0) { *ok = 1; return PS_OK; }
    // the scalars [w_i | rho_j z_j | rho_j] with w_i = sum_j rho_j c_ij, and s = sum_j rho_j sum_i c_ij y_ij, on the host
    std::vector<uint8_t> sc(32 * (m + 2 * t));
    std::vector<Fr> w(m, fr_zero());
    Fr s = fr_zero();
    for (size_t j = 0; j < t; j++) {
        Fr z;
        if (!fr_mont_from_canonical_be32(&z, z_be32 + 32 * j)) return fail(PS_ERR_ENCODING, who + ": z[" + std::to_string(j) + "] is not below r");
        const Fr rho = fr_mont_from_be32(rho_be32 + 32 * j);
        fr_mont_to_be32(sc.data() + 32 * (m + j), fr_mul(rho, z));
        memcpy(sc.data() + 32 * (m + t + j), rho_be32 + 32 * j, 32);
        Fr col = fr_zero();  // sum_i c_ij y_ij
        bool any = false;
        for (size_t i = 0; i < m; i++) {
            const std::string at = "[" + std::to_string(i) + "][" + std::to_string(j) + "]";
            Fr cv, y;
            if (!fr_mont_from_canonical_be32(&cv, coef_be32 + 32 * (i * t + j))) return fail(PS_ERR_ENCODING, who + ": coefficient " + at + " is not below r");
            if (fr_is_zero(cv)) continue;  // nothing is opened here: y is not read
            any = true;
            if (!fr_mont_from_canonical_be32(&y, y_be32 + 32 * (i * t + j))) return fail(PS_ERR_ENCODING, who + ": y" + at + " is not below r");
            w[i] = fr_reduce(fr_add(w[i], fr_mul(rho, cv)));
            col = fr_reduce(fr_add(col, fr_mul(cv, y)));
        }
        if (!any) return fail(PS_ERR_ARG, who + ": no polynomial is opened at z[" + std::to_string(j) + "] (its column of coefficients is zero)");
        s = fr_reduce(fr_add(s, fr_mul(rho, col)));
    }
    for (size_t i = 0; i < m; i++) fr_mont_to_be32(sc.data() + 32 * i, w[i]);
    // A = sum_i w_i C_i + sum_j rho_j z_j pi_j - s G1,  B = sum_j rho_j pi_j:   e(A, G2) e(-B, tau G2) == 1
    return kzg_check_sums(c, who, t2, commits, m, proofs, t, sc, m + t, s, check_subgroup, ok);
}

// ---- one polynomial at a SET of points: one quotient, one proof ----

// What the host derives from the k points of a set, all in Montgomery form:
//   z[j], w[j] = 1 / prod_{l != j} (z_j - z_l)  (canonical limbs: the kernel's weights; k^2 products and ONE inversion, the
//   denominators being inverted together), and with want_zs: zs = Z_S = prod_j (X - z_j), k + 1 coefficients lowest first
//   (k^2 products more; the verifier and the remainder need it, the opening does not) -- hence PS_KZG_SET_MAX.
struct KzgSet {
    std::vector<Fr> z, w, zs;
};
static int kzg_set_prepare(const std::string& who, const uint8_t* z_be32, size_t k, bool want_zs, KzgSet* s) {
    s->z.assign(k, fr_zero());
    s->w.assign(k, fr_zero());
    for (size_t j = 0; j < k; j++)
        if (!fr_mont_from_canonical_be32(&s->z[j], z_be32 + 32 * j)) return fail(PS_ERR_ENCODING, who + ": z[" + std::to_string(j) + "] is not below r");
    for (size_t j = 0; j < k; j++)
        for (size_t l = 0; l < j; l++)
            if (!memcmp(z_be32 + 32 * l, z_be32 + 32 * j, 32))
                return fail(PS_ERR_ARG, who + ": z[" + std::to_string(l) + "] and z[" + std::to_string(j) +
                                            "] are equal (a set has distinct points; the single-point openings take repeated ones)");
    std::vector<Fr> d(k), pre(k);  // d_j = prod_{l != j} (z_j - z_l), non-zero: the points are distinct; pre_j = d_0 .. d_j
    for (size_t j = 0; j < k; j++) {
        d[j] = fr_one();
        for (size_t l = 0; l < k; l++)
            if (l != j) d[j] = fr_mul(d[j], fr_sub(s->z[j], s->z[l]));  // a difference of two products' values: class 1, |V| < 10r/8
        pre[j] = j ? fr_mul(pre[j - 1], d[j]) : d[j];
    }
    Fr inv = fr_inv(pre[k - 1]);
    for (size_t j = k; j-- > 0;) {
        s->w[j] = fr_canon(j ? fr_mul(inv, pre[j - 1]) : inv);
        inv = fr_mul(inv, d[j]);
    }
    if (!want_zs) return PS_OK;
    s->zs.assign(k + 1, fr_zero());
    s->zs[0] = fr_one();
    for (size_t j = 0; j < k; j++)  // times (X - z_j), from the top down: new[i + 1] = old[i] - z_j old[i + 1], in two steps
        for (size_t i = j + 1; i-- > 0;) {
            s->zs[i + 1] = fr_reduce(fr_add(s->zs[i + 1], s->zs[i]));
            s->zs[i] = fr_neg(fr_mul(s->zs[i], s->z[j]));
        }
    return PS_OK;
}
// The interpolant of (z_j, y_j): r = sum_j y_j w_j Z_S / (X - z_j), k coefficients lowest first, Montgomery form; s.zs is
// there.  Two products per (j, i).  Lazy ranges: b_{i-1} = c_i + z_j b_i is a Horner step -- a coefficient in (-9r/8, 9r/8) plus a
// product, limbs at class 2 at most, straight into the next product; the sums over j are fr_norm'ed after every addition and
// reduced behind every 32nd, as the device accumulators are (|V| < 38 r between two reductions).
static std::vector<Fr> kzg_set_interpolate(const KzgSet& s, const std::vector<Fr>& y) {
    const size_t k = s.z.size();
    std::vector<Fr> r(k, fr_zero()), b(k);
    for (size_t j = 0; j < k; j++) {
        b[k - 1] = s.zs[k];  // synthetic division of Z_S by (X - z_j)
        for (size_t i = k - 1; i >= 1; i--) b[i - 1] = fr_add(s.zs[i], fr_mul(s.z[j], b[i]));
        const Fr c = fr_mul(y[j], s.w[j]);
        const bool reduce = poly_scan_set_reduce_after(j) || j + 1 == k;
        for (size_t i = 0; i < k; i++) {
            r[i] = fr_norm(fr_add(r[i], fr_mul(c, b[i])));
            if (reduce) r[i] = fr_reduce(r[i]);
        }
    }
    return r;
}

// Arguments shared by ps_poly_div_roots and ps_kzg_open_set
static int kzg_set_args(const std::string& who, const ps_ctx* c, const ps_scalars* p, const uint8_t* z_be32, size_t k, const uint8_t* y_be32) {
    if (!c || !p || !z_be32 || !y_be32) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (p->n == 0) return fail(PS_ERR_LENGTH, who + ": empty polynomial");
    if (k == 0) return fail(PS_ERR_ARG, who + ": an empty set (division by the constant 1 is a copy and is not offered)");
    if (!poly_scan_set_points_ok(k)) return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points, at most " + std::to_string(PS_KZG_SET_MAX) + " in a set");
    if (!poly_scan_set_size_ok(p->n, k))
        return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points x " + std::to_string(p->n) + " coefficients reach 2^32");
    return PS_OK;
}

// *q = the n - k coefficients of (p - r) / Z_S and y_be32[j] = p(z_j), for n > k: totals, carries, the set apply pass into
// ceil(k / G) partial rows, and their sum by k_fr_lincomb with unit weights where there is more than one.  *q is the caller's.
static int kzg_set_quotient(ps_ctx* c, const std::string& who, const ps_scalars* p, const KzgSet& s, const std::vector<FrPow2Table>& tabs, uint8_t* y_be32,
                            ps_scalars** q) {
    const u64 n = p->n, k = tabs.size(), nq = poly_scan_set_quotient_len(n, k), groups = poly_scan_set_groups(k);
    const u32 tiles = (u32)poly_scan_tiles(n);
    hipStream_t st = c->stream;
    Scope scope(st);
    if (int rc = scalars_fresh(c, who.c_str(), nq, scope.result(q))) return rc;
    FrPow2Table* d_tabs = nullptr;
    Fr *totals = nullptr, *carries = nullptr, *d_w = nullptr;
    u32 *d_y = nullptr, *partial = (u32*)(*q)->st->p;
    hipError_t e;
    if ((e = scope.device(&d_tabs, k)) != hipSuccess || (e = scope.device(&totals, poly_scan_total_elems(n, k))) != hipSuccess ||
        (e = scope.device(&carries, poly_scan_total_elems(n, k))) != hipSuccess || (e = scope.device(&d_y, poly_scan_value_words(k))) != hipSuccess ||
        (e = scope.device(&d_w, poly_scan_set_weight_elems(k))) != hipSuccess ||
        (groups > 1 && (e = scope.device(&partial, poly_scan_set_partial_words(n, k))) != hipSuccess))
        return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
    if (storage_wait_ready(p->st, st)) return fail(PS_ERR_HIP, who + ": event wait failed");
    if ((e = hipMemcpyAsync(d_tabs, tabs.data(), sizeof(FrPow2Table) * k, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(d_w, s.w.data(), sizeof(Fr) * k, hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": copy of the tables: " + hipGetErrorString(e));
    const u32* coef = scalars_ptr(p);
    hipLaunchKernelGGL(k_poly_scan_tile<false>, dim3(tiles, (u32)k), dim3(POLY_SCAN_THREADS), 0, st, coef, n, tiles, (const FrPow2Table*)d_tabs, totals,
                       (const Fr*)nullptr, (u32*)nullptr);
    hipLaunchKernelGGL(k_poly_scan_carries, dim3((u32)k), dim3(POLY_SCAN_THREADS), 0, st, (const Fr*)totals, carries, tiles, (const FrPow2Table*)d_tabs, d_y);
    hipLaunchKernelGGL(k_poly_scan_set_apply, dim3(tiles, (u32)groups), dim3(POLY_SCAN_THREADS), 0, st, coef, n, tiles, (u32)k, nq,
                       (const FrPow2Table*)d_tabs, (const Fr*)d_w, (const Fr*)carries, partial);
    std::vector<FrLincombInput> ins(groups);
    std::vector<FrLincombCoef> ones(groups);
    if (groups > 1) {  // q = the sum of the partial rows: the rows as inputs of one combination with the weights 1
        const Fr one = fr_canon(fr_one());
        for (u64 g = 0; g < groups; g++) {
            ins[g] = FrLincombInput{partial + poly_scan_set_partial_word(g, 0, nq), nq};
            for (int i = 0; i < FR_L; i++) ones[g].l[i] = one.l[i];
            ones[g].nonzero = 1;
            ones[g].pad = 0;
        }
        FrLincombInput* d_in = nullptr;
        FrLincombCoef* d_coef = nullptr;
        if ((e = scope.device(&d_in, groups)) != hipSuccess || (e = scope.device(&d_coef, groups)) != hipSuccess)
            return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
        if ((e = hipMemcpyAsync(d_in, ins.data(), sizeof(FrLincombInput) * groups, hipMemcpyHostToDevice, st)) != hipSuccess ||
            (e = hipMemcpyAsync(d_coef, ones.data(), sizeof(FrLincombCoef) * groups, hipMemcpyHostToDevice, st)) != hipSuccess)
            return fail(PS_ERR_HIP, who + ": copy of the tables: " + hipGetErrorString(e));
        hipLaunchKernelGGL(k_fr_lincomb, dim3((u32)fr_lincomb_blocks(nq), 1), dim3(FR_LINCOMB_THREADS), 0, st, (const FrLincombInput*)d_in, (u32)groups,
                           (const FrLincombCoef*)d_coef, 1u, 0u, nq, (u32*)(*q)->st->p);
    }
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, who + ": kernels: " + hipGetErrorString(e));
    std::vector<u32> y(8 * k);
    if ((e = hipMemcpyAsync(y.data(), d_y, 32 * k, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": run: " + hipGetErrorString(e));
    for (u64 j = 0; j < k; j++) words_to_be32(y_be32 + 32 * j, y.data() + 8 * j);
    return scope.finish(PS_OK);
}

extern "C" int ps_poly_scan_set_group(void) { return POLY_SCAN_SET_GROUP; }

extern "C" int ps_poly_div_roots(ps_ctx* c, const ps_scalars* p, const uint8_t* z_be32, size_t k, ps_scalars** q, uint8_t* y_be32, uint8_t* rem_be32) {
    const std::string who = "ps_poly_div_roots";
    if (!q) return fail(PS_ERR_ARG, who + ": NULL argument");
    *q = nullptr;
    int rc = kzg_set_args(who, c, p, z_be32, k, y_be32);
    if (rc) return rc;
    KzgSet s;
    std::vector<FrPow2Table> tabs;
    if ((rc = kzg_set_prepare(who, z_be32, k, rem_be32 != nullptr && p->n > k, &s)) || (rc = poly_scan_tables(who.c_str(), z_be32, k, &tabs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = p->n;
    Scope scope(c->stream);
    if (n <= k) {  // the quotient is empty and the remainder is p itself
        if ((rc = scalars_fresh(c, who.c_str(), 0, scope.result(q))) || (rc = poly_scan_run(c, who.c_str(), p, tabs, nullptr, y_be32))) return rc;
        if (rem_be32) {
            memset(rem_be32, 0, 32 * k);
            if ((rc = ps_scalars_download(c, p, 0, n, rem_be32))) return rc;
        }
        return scope.finish(PS_OK);
    }
    if ((rc = kzg_set_quotient(c, who, p, s, tabs, y_be32, scope.result(q)))) return rc;
    if (rem_be32) {
        std::vector<Fr> y(k);
        for (size_t j = 0; j < k; j++) (void)fr_mont_from_canonical_be32(&y[j], y_be32 + 32 * j);
        const std::vector<Fr> r = kzg_set_interpolate(s, y);
        for (size_t i = 0; i < k; i++) fr_mont_to_be32(rem_be32 + 32 * i, r[i]);
    }
    return scope.finish(PS_OK);
}

extern "C" int ps_kzg_open_set(ps_ctx* c, const ps_points* tau_g1, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32, uint8_t* proof) {
    const std::string who = "ps_kzg_open_set";
    int rc = kzg_string_args(who.c_str(), c, tau_g1, p);
    if (rc) return rc;
    if ((rc = kzg_set_args(who, c, p, z_be32, k, y_be32))) return rc;
    if (!proof) return fail(PS_ERR_ARG, who + ": NULL argument");
    KzgSet s;
    std::vector<FrPow2Table> tabs;
    if ((rc = kzg_set_prepare(who, z_be32, k, false, &s)) || (rc = poly_scan_tables(who.c_str(), z_be32, k, &tabs))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = p->n;
    if (n <= k) {  // p is its own interpolant: the quotient is zero
        if ((rc = poly_scan_run(c, who.c_str(), p, tabs, nullptr, y_be32))) return rc;
        write_identity(PS_G1, proof);
        return PS_OK;
    }
    Scope scope(c->stream);
    ps_scalars** q = scope.scalars();
    ps_points** head = scope.points();
    if ((rc = kzg_set_quotient(c, who, p, s, tabs, y_be32, q))) return rc;
    if ((rc = ps_points_slice(tau_g1, 0, n - k, head))) return rc;
    return scope.finish(ps_msm(c, *head, *q, proof));  // the lone sum; the quotient never leaves the device
}

extern "C" int ps_kzg_verify_set(ps_ctx* c, const ps_points* tau_g1, const ps_points* tau_g2, const uint8_t* commit, const uint8_t* z_be32,
                                 const uint8_t* y_be32, size_t k, const uint8_t* proof, int check_subgroup, int* ok) {
    const std::string who = "ps_kzg_verify_set";
    if (!c || !tau_g1 || !tau_g2 || !commit || !z_be32 || !y_be32 || !proof || !ok) return fail(PS_ERR_ARG, who + ": NULL argument");
    *ok = 0;
    if (tau_g1->group != PS_G1 || tau_g2->group != PS_G2) return fail(PS_ERR_ARG, who + ": tau_g1 is a G1 array and tau_g2 a G2 array");
    if (k == 0) return fail(PS_ERR_ARG, who + ": an empty set");
    if (!poly_scan_set_points_ok(k)) return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points, at most " + std::to_string(PS_KZG_SET_MAX) + " in a set");
    if (tau_g1->n < k)  // BlindEval's panic (algebra.go:350-352)
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(k) + " and the " + std::to_string(tau_g1->n) + " powers of the string");
    if (tau_g2->n < k + 1)
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(k + 1) + " and the " + std::to_string(tau_g2->n) + " powers of the string");
    if (c->q_len) return fail(PS_ERR_ARG, who + ": sums are pending on this context (ps_msm_finish them first)");
    KzgSet s;
    int rc = kzg_set_prepare(who, z_be32, k, true, &s);
    if (rc) return rc;
    std::vector<Fr> y(k);
    for (size_t j = 0; j < k; j++)
        if (!fr_mont_from_canonical_be32(&y[j], y_be32 + 32 * j)) return fail(PS_ERR_ENCODING, who + ": y[" + std::to_string(j) + "] is not below r");
    Affine<Fp> cm, pi, lhs;
    Affine<Fp2> zs2;
    if (!read_g1(cm, commit) || !read_g1(pi, proof)) return fail(PS_ERR_ENCODING, who + ": a point is not a canonical point on the curve");
    if (check_subgroup && !all_in_subgroup({&cm, &pi}, {})) return PS_OK;
    // the coefficients of r and of Z_S on the host; [r(tau)] G1 and [Z_S(tau)] G2 as two lone sums over the heads of the strings
    const std::vector<Fr> r = kzg_set_interpolate(s, y);
    std::vector<uint8_t> sc(32 * (2 * k + 1));
    for (size_t i = 0; i < k; i++) fr_mont_to_be32(sc.data() + 32 * i, r[i]);
    for (size_t i = 0; i <= k; i++) fr_mont_to_be32(sc.data() + 32 * (k + i), s.zs[i]);
    HIP_TRY(hipSetDevice(c->device));
    Scope scope;
    ps_scalars **all = scope.scalars(), **rc_s = scope.scalars(), **zc_s = scope.scalars();
    ps_points **h1 = scope.points(), **h2 = scope.points();
    uint8_t two[2 * 96], coef[2 * 32], sum[96], z2[192];
    if ((rc = ps_scalars_upload(c, sc.data(), 2 * k + 1, all)) || (rc = ps_scalars_slice(*all, 0, k, rc_s)) || (rc = ps_scalars_slice(*all, k, k + 1, zc_s)) ||
        (rc = ps_points_slice(tau_g1, 0, k, h1)) || (rc = ps_points_slice(tau_g2, 0, k + 1, h2)) || (rc = ps_msm(c, *h1, *rc_s, two + 96)) ||
        (rc = ps_msm(c, *h2, *zc_s, z2)))
        return rc;
    // C - R
    memcpy(two, commit, 96);
    memset(coef, 0, 32);
    coef[31] = 1;
    fr_mont_to_be32(coef + 32, fr_neg(fr_one()));
    if ((rc = ps_points_lincomb(PS_G1, two, coef, 2, sum))) return rc;
    if (!read_g1(lhs, sum) || !read_g2(zs2, z2)) return fail(PS_ERR_ENCODING, who + ": internal: a sum does not decode");
    *ok = product_is_one({{lhs, generator((const Fp2*)0)}, {pairing_dev::neg_g1(pi), zs2}}) ? 1 : 0;
    return scope.finish(PS_OK);
}

// ---- polynomials given by their values on the nodes 1 .. n (the Lagrange form): no interpolation, no division ----

// The k points as the kernels read them: z in Montgomery form and the node it is, if any (PS_ERR_ENCODING for a z not below r)
static int lagr_points(const std::string& who, const uint8_t* z_be32, size_t k, u64 n, std::vector<LagrPoint>* pts) {
    pts->assign(k, LagrPoint());
    for (size_t j = 0; j < k; j++) {
        u32 w[8];
        if (!be32_to_words(w, z_be32 + 32 * j)) return fail(PS_ERR_ENCODING, who + ": z[" + std::to_string(j) + "] is not below r");
        (*pts)[j].z = fr_to_mont(fr_from_words8(w));
        (*pts)[j].hit = (u32)poly_lagr_hit(w, n);
        (*pts)[j].pad = 0;
    }
    return PS_OK;
}

// Arguments shared by ps_poly_eval_lagrange, ps_poly_div_linear_lagrange and ps_kzg_open_lagrange; *skip: k == 0, nothing to do
static int lagr_args(const std::string& who, const ps_ctx* c, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k,
                     const uint8_t* y_be32, bool* skip) {
    *skip = false;
    if (!c || !q || !values) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (values->n != q->n)
        return fail(PS_ERR_LENGTH, who + ": " + std::to_string(values->n) + " values on a domain of " + std::to_string(q->n) + " nodes");
    if (k == 0) { *skip = true; return PS_OK; }
    if (!z_be32 || !y_be32) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (!poly_lagr_total_ok(q->n, k))
        return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points x " + std::to_string(q->n) + " values reach 2^32 (split the points)");
    return PS_OK;
}

// The launches for k points over the n values: y_be32[j] = p(z_j); rows != nullptr: row j of rows (n scalars each) = the values
// of (p - p(z_j)) / (X - z_j) on the nodes.  Returns with the stream idle.
// set != nullptr (a set of k < n distinct points, set->w its weights c_j): rows is ONE row of n scalars and gets the values of
// the set quotient sum_j c_j (p - p(z_j)) / (X - z_j) -- k_lagr_tile<false> and the walk as for the values alone, then k_lagr_fold
// (poly_lagrange_set.hpp) into ceil(k / G) partial rows and, where there is more than one, their sum by k_fr_lincomb with unit
// weights.
static int lagr_run(ps_ctx* c, const std::string& who, const ps_qap* q, const ps_scalars* values, const std::vector<LagrPoint>& pts, u32* rows,
                    uint8_t* y_be32, const KzgSet* set = nullptr) {
    const u64 n = q->n, k = pts.size(), groups = set ? poly_lagr_set_groups(k) : 0;
    const u32 tiles = (u32)poly_lagr_tiles(n);
    hipStream_t st = c->stream;
    std::vector<FrLincombInput> ins(groups);  // (the tables of the sum outlive the scope's wait for the stream)
    std::vector<FrLincombCoef> ones(groups);
    Scope scope(st);
    LagrPoint* d_pts = nullptr;
    Fr *parts = nullptr, *yq = nullptr, *d_w = nullptr;
    u32 *d_y = nullptr, *partial = rows;
    FrLincombInput* d_in = nullptr;
    FrLincombCoef* d_coef = nullptr;
    hipError_t e;
    if ((e = scope.device(&d_pts, k)) != hipSuccess || (e = scope.device(&parts, poly_lagr_part_elems(n, k))) != hipSuccess ||
        (e = scope.device(&yq, poly_lagr_yq_elems(k))) != hipSuccess || (e = scope.device(&d_y, poly_lagr_value_words(k))) != hipSuccess ||
        (set && (e = scope.device(&d_w, poly_lagr_set_weight_elems(k))) != hipSuccess) ||
        (groups > 1 && ((e = scope.device(&partial, poly_lagr_set_partial_words(n, k))) != hipSuccess || (e = scope.device(&d_in, groups)) != hipSuccess ||
                        (e = scope.device(&d_coef, groups)) != hipSuccess)))
        return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
    if (storage_wait_ready(values->st, st)) return fail(PS_ERR_HIP, who + ": event wait failed");
    if ((e = hipMemcpyAsync(d_pts, pts.data(), sizeof(LagrPoint) * k, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (set && (e = hipMemcpyAsync(d_w, set->w.data(), sizeof(Fr) * k, hipMemcpyHostToDevice, st)) != hipSuccess))
        return fail(PS_ERR_HIP, who + ": copy of the points: " + hipGetErrorString(e));
    const u32* v = scalars_ptr(values);
    const u64 plane = poly_lagr_plane_elems(n, k);
    for (u64 j0 = 0; j0 < k; j0 += POLY_LAGR_MAX_POINTS_PER_LAUNCH) {  // blockIdx.y picks the point
        const u32 kb = (u32)std::min<u64>(k - j0, POLY_LAGR_MAX_POINTS_PER_LAUNCH);
        Fr* part = parts + j0 * tiles;  // the planes stay `plane` apart
        u32* row = rows && !set ? rows + 8 * j0 * n : nullptr;
        if (row)
            hipLaunchKernelGGL(k_lagr_tile<true>, dim3(tiles, kb), dim3(POLY_LAGR_THREADS), 0, st, v, n, tiles, (const LagrPoint*)(d_pts + j0),
                               (const Fr*)q->qt.invfact, part, plane, row);
        else
            hipLaunchKernelGGL(k_lagr_tile<false>, dim3(tiles, kb), dim3(POLY_LAGR_THREADS), 0, st, v, n, tiles, (const LagrPoint*)(d_pts + j0),
                               (const Fr*)q->qt.invfact, part, plane, (u32*)nullptr);
        hipLaunchKernelGGL(k_lagr_walk, dim3(kb), dim3(POLY_LAGR_THREADS), 0, st, (const Fr*)part, plane, tiles, (const LagrPoint*)(d_pts + j0), v, n,
                           (const Fr*)q->qt.fact2, d_y + 8 * j0, yq + 2 * j0);
        if (row)
            hipLaunchKernelGGL(k_lagr_apply, dim3((u32)poly_lagr_apply_blocks(n), kb), dim3(POLY_LAGR_THREADS), 0, st, v, n,
                               (const LagrPoint*)(d_pts + j0), (const Fr*)(yq + 2 * j0), row);
    }
    if (set) {  // k <= POLY_LAGR_SET_MAX: the loop above ran once
        hipLaunchKernelGGL(k_lagr_fold, dim3(tiles, (u32)groups), dim3(POLY_LAGR_THREADS), 0, st, v, n, (u32)k, (const LagrPoint*)d_pts, (const Fr*)d_w,
                           (const Fr*)yq, partial);
        if (groups > 1) {  // the rows as inputs of one combination with the weights 1
            const Fr one = fr_canon(fr_one());
            for (u64 g = 0; g < groups; g++) {
                ins[g] = FrLincombInput{partial + poly_lagr_set_partial_word(g, 1, n), n};
                for (int i = 0; i < FR_L; i++) ones[g].l[i] = one.l[i];
                ones[g].nonzero = 1;
                ones[g].pad = 0;
            }
            if ((e = hipMemcpyAsync(d_in, ins.data(), sizeof(FrLincombInput) * groups, hipMemcpyHostToDevice, st)) != hipSuccess ||
                (e = hipMemcpyAsync(d_coef, ones.data(), sizeof(FrLincombCoef) * groups, hipMemcpyHostToDevice, st)) != hipSuccess)
                return fail(PS_ERR_HIP, who + ": copy of the tables: " + hipGetErrorString(e));
            hipLaunchKernelGGL(k_fr_lincomb, dim3((u32)fr_lincomb_blocks(n), 1), dim3(FR_LINCOMB_THREADS), 0, st, (const FrLincombInput*)d_in, (u32)groups,
                               (const FrLincombCoef*)d_coef, 1u, 0u, n, rows);
        }
    }
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, who + ": kernels: " + hipGetErrorString(e));
    std::vector<u32> y(8 * k);
    if ((e = hipMemcpyAsync(y.data(), d_y, 32 * k, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": run: " + hipGetErrorString(e));
    for (u64 j = 0; j < k; j++) words_to_be32(y_be32 + 32 * j, y.data() + 8 * j);
    return scope.finish(PS_OK);
}

extern "C" int ps_poly_lagrange_tile(void) { return POLY_LAGR_TILE; }

// The n values of (L|R|O).sol on the domain: ps_qap_interpolate without its interpolation
extern "C" int ps_qap_gate_values(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, int which, ps_scalars** out) {
    if (!c || !q || !sol || !out) return fail(PS_ERR_ARG, "ps_qap_gate_values: NULL argument");
    if (which < 0 || which > 2) return fail(PS_ERR_ARG, "ps_qap_gate_values: which must be 0 (left), 1 (right) or 2 (out)");
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (storage_wait_ready(sol->st, st)) return fail(PS_ERR_HIP, "ps_qap_gate_values: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, st, q->sol_m, scalars_ptr(sol), (u64)q->m);
    spmv_launch(st, q->mat[which], (const Fr*)q->sol_m, q->y[which], (u32)q->n);
    int rc = scalars_from_mont(c, q->y[which], q->n, out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return PS_OK;
}

extern "C" int ps_poly_eval_lagrange(ps_ctx* c, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, uint8_t* y_be32) {
    const std::string who = "ps_poly_eval_lagrange";
    bool skip;
    int rc = lagr_args(who, c, q, values, z_be32, k, y_be32, &skip);
    if (rc || skip) return rc;
    std::vector<LagrPoint> pts;
    if ((rc = lagr_points(who, z_be32, k, q->n, &pts))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return lagr_run(c, who, q, values, pts, nullptr, y_be32);
}

extern "C" int ps_poly_div_linear_lagrange(ps_ctx* c, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, ps_scalars** qv,
                                           uint8_t* y_be32) {
    const std::string who = "ps_poly_div_linear_lagrange";
    if (!qv) return fail(PS_ERR_ARG, who + ": NULL argument");
    *qv = nullptr;
    bool skip;
    int rc = lagr_args(who, c, q, values, z_be32, k, y_be32, &skip);
    if (rc) return rc;
    std::vector<LagrPoint> pts;
    if (!skip && (rc = lagr_points(who, z_be32, k, q->n, &pts))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    if ((rc = scalars_fresh(c, who.c_str(), (u64)k * q->n, scope.result(qv)))) return rc;  // k == 0: an empty vector
    if (!skip && (rc = lagr_run(c, who, q, values, pts, (u32*)(*qv)->st->p, y_be32))) return rc;
    return scope.finish(PS_OK);
}

// lag_g1 and values of one length, lag_g1 a G1 array, no sum pending
static int lagr_string_args(const std::string& who, const ps_ctx* c, const ps_points* lag_g1, const ps_scalars* values, size_t n) {
    if (!c || !lag_g1 || !values) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (lag_g1->group != PS_G1) return fail(PS_ERR_ARG, who + ": lag_g1 is a G1 array");
    if (lag_g1->n != n || values->n != n)
        return fail(PS_ERR_LENGTH, who + ": " + std::to_string(values->n) + " values and " + std::to_string(lag_g1->n) +
                                       " points of the Lagrange-form string on a domain of " + std::to_string(n) + " nodes");
    if (c->q_len) return fail(PS_ERR_ARG, who + ": sums are pending on this context (ps_msm_finish them first)");
    return PS_OK;
}

extern "C" int ps_kzg_commit_lagrange(ps_ctx* c, const ps_points* lag_g1, const ps_scalars* values, uint8_t* out) {
    const std::string who = "ps_kzg_commit_lagrange";
    int rc = lagr_string_args(who, c, lag_g1, values, lag_g1 ? lag_g1->n : 0);
    if (rc) return rc;
    if (!out) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (values->n == 0) return fail(PS_ERR_LENGTH, who + ": no values");
    return ps_msm(c, lag_g1, values, out);
}

extern "C" int ps_kzg_open_lagrange(ps_ctx* c, const ps_qap* q, const ps_points* lag_g1, const ps_scalars* values, const uint8_t* z_be32, size_t k,
                                    uint8_t* y_be32, uint8_t* proofs) {
    const std::string who = "ps_kzg_open_lagrange";
    if (!q) return fail(PS_ERR_ARG, who + ": NULL argument");
    int rc = lagr_string_args(who, c, lag_g1, values, q->n);
    if (rc) return rc;
    bool skip;
    if ((rc = lagr_args(who, c, q, values, z_be32, k, y_be32, &skip)) || skip) return rc;
    if (!proofs) return fail(PS_ERR_ARG, who + ": NULL argument");
    std::vector<LagrPoint> pts;
    if ((rc = lagr_points(who, z_be32, k, q->n, &pts))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    ps_scalars** rows = scope.scalars();
    if ((rc = scalars_fresh(c, who.c_str(), (u64)k * q->n, rows))) return rc;
    if ((rc = lagr_run(c, who, q, values, pts, (u32*)(*rows)->st->p, y_be32))) return rc;
    // the quotient rows never leave the device: the lone sum for one point (measured ahead of a one-row batch), else ONE batch
    if (k == 1) return scope.finish(ps_msm(c, lag_g1, *rows, proofs));
    return scope.finish(ps_msm_batch(c, lag_g1, *rows, k, proofs));
}

// ---- a value-form polynomial at a SET of points: the k linear quotients folded into one row of n values, one proof ----

// Arguments shared by ps_poly_div_roots_lagrange and ps_kzg_open_set_lagrange: the set section's and the Lagrange section's
static int lagr_set_args(const std::string& who, const ps_ctx* c, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k,
                         const uint8_t* y_be32) {
    if (!c || !q || !values || !z_be32 || !y_be32) return fail(PS_ERR_ARG, who + ": NULL argument");
    if (values->n != q->n)
        return fail(PS_ERR_LENGTH, who + ": " + std::to_string(values->n) + " values on a domain of " + std::to_string(q->n) + " nodes");
    if (k == 0) return fail(PS_ERR_ARG, who + ": an empty set (division by the constant 1 is a copy and is not offered)");
    if (!poly_lagr_set_points_ok(k))
        return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points, at most " + std::to_string(POLY_LAGR_SET_MAX) + " in a set");
    if (!poly_lagr_set_size_ok(q->n, k))
        return fail(PS_ERR_ARG, who + ": " + std::to_string(k) + " points x " + std::to_string(q->n) + " values reach 2^32");
    return PS_OK;
}

// *qv = the n values of (p - r) / Z_S on the nodes (zero for k >= n: p is its own interpolant) and y_be32[j] = p(z_j).  *qv is
// the caller's (a Scope result or slot).
static int lagr_set_quotient(ps_ctx* c, const std::string& who, const ps_qap* q, const ps_scalars* values, const std::vector<LagrPoint>& pts,
                             const KzgSet& s, uint8_t* y_be32, ps_scalars** qv) {
    const u64 n = q->n, k = pts.size();
    if (int rc = scalars_fresh(c, who.c_str(), n, qv)) return rc;
    u32* row = (u32*)(*qv)->st->p;
    if (!poly_lagr_set_zero(n, k)) return lagr_run(c, who, q, values, pts, row, y_be32, &s);
    hipError_t e = hipMemsetAsync(row, 0, 32 * n, c->stream);
    if (e != hipSuccess) return fail(PS_ERR_HIP, who + ": hipMemsetAsync: " + hipGetErrorString(e));
    return lagr_run(c, who, q, values, pts, nullptr, y_be32);
}

extern "C" int ps_poly_lagrange_set_group(void) { return POLY_LAGR_SET_GROUP; }

extern "C" int ps_poly_div_roots_lagrange(ps_ctx* c, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, ps_scalars** qv,
                                          uint8_t* y_be32, uint8_t* rem_be32) {
    const std::string who = "ps_poly_div_roots_lagrange";
    if (!qv) return fail(PS_ERR_ARG, who + ": NULL argument");
    *qv = nullptr;
    int rc = lagr_set_args(who, c, q, values, z_be32, k, y_be32);
    if (rc) return rc;
    KzgSet s;
    std::vector<LagrPoint> pts;
    if ((rc = kzg_set_prepare(who, z_be32, k, rem_be32 != nullptr, &s)) || (rc = lagr_points(who, z_be32, k, q->n, &pts))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    if ((rc = lagr_set_quotient(c, who, q, values, pts, s, y_be32, scope.result(qv)))) return rc;
    if (rem_be32) {  // the interpolant of the (z_j, y_j): for k >= n it is p itself, zero-extended
        std::vector<Fr> y(k);
        for (size_t j = 0; j < k; j++) (void)fr_mont_from_canonical_be32(&y[j], y_be32 + 32 * j);
        const std::vector<Fr> r = kzg_set_interpolate(s, y);
        for (size_t i = 0; i < k; i++) fr_mont_to_be32(rem_be32 + 32 * i, r[i]);
    }
    return scope.finish(PS_OK);
}

extern "C" int ps_kzg_open_set_lagrange(ps_ctx* c, const ps_qap* q, const ps_points* lag_g1, const ps_scalars* values, const uint8_t* z_be32, size_t k,
                                        uint8_t* y_be32, uint8_t* proof) {
    const std::string who = "ps_kzg_open_set_lagrange";
    if (!q) return fail(PS_ERR_ARG, who + ": NULL argument");
    int rc = lagr_string_args(who, c, lag_g1, values, q->n);
    if (rc) return rc;
    if ((rc = lagr_set_args(who, c, q, values, z_be32, k, y_be32))) return rc;
    if (!proof) return fail(PS_ERR_ARG, who + ": NULL argument");
    KzgSet s;
    std::vector<LagrPoint> pts;
    if ((rc = kzg_set_prepare(who, z_be32, k, false, &s)) || (rc = lagr_points(who, z_be32, k, q->n, &pts))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (poly_lagr_set_zero(q->n, k)) {  // p is its own interpolant: the quotient is zero
        if ((rc = lagr_run(c, who, q, values, pts, nullptr, y_be32))) return rc;
        write_identity(PS_G1, proof);
        return PS_OK;
    }
    Scope scope(c->stream);
    ps_scalars** row = scope.scalars();
    if ((rc = lagr_set_quotient(c, who, q, values, pts, s, y_be32, row))) return rc;
    return scope.finish(ps_msm(c, lag_g1, *row, proof));  // the lone sum; the row never leaves the device
}

// ---- a value-form polynomial at EVERY node of its domain: n proofs from two transforms over points (kzg_all.hpp) ----

// A <- the cyclic correlation of its S = 2^p points with a multiplier given as its stored transform khat (the order
// ntt_run<false> leaves, the inverse's 2^-p folded in): the NTT over points, the pointwise products, the inverse NTT -- what
// srs_xi_t and the C^T step of monomial_to_lagrange_t launch, once for the entries below.  marks: two events recorded around
// the pointwise pass (the stage split of tools/kzg_all_sweep.py), or nullptr.
template <class F>
static void ec_correlate(const NttTables& tb, hipStream_t st, Xyzz<F>* A, u32 S, int p, const Fr* khat, hipEvent_t* marks = nullptr) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    ec_ntt<F, false>(tb, st, A, S, p);
    if (marks) (void)hipEventRecord(marks[0], st);
    hipLaunchKernelGGL(k_ec_scale<KF>, dim3(nblocks((size_t)S * LN)), dim3(256), 0, st, A, S, khat, ~0ull);
    if (marks) (void)hipEventRecord(marks[1], st);
    ec_ntt<F, true>(tb, st, A, S, p);
}

// the checks both entries share; values == nullptr: the key entry, which takes none
static int kzg_all_args(const std::string& who, const ps_qap* q, const ps_points* lag_g1, const ps_points* all_key, const ps_scalars* values) {
    if (lag_g1->group != PS_G1 || (all_key && all_key->group != PS_G1)) return fail(PS_ERR_ARG, who + ": lag_g1 and all_key are G1 arrays");
    const size_t n = q->n;
    if (lag_g1->n != n || (values && values->n != n) || (all_key && all_key->n != n))
        return fail(PS_ERR_LENGTH, who + ": " + (values ? std::to_string(values->n) + " values, " : std::string()) + std::to_string(lag_g1->n) +
                                       " points of the Lagrange-form string" + (all_key ? " and " + std::to_string(all_key->n) + " of the key table" : std::string()) +
                                       " on a domain of " + std::to_string(n) + " nodes");
    if (!kzg_all_size_ok(n))
        return fail(PS_ERR_ARG, who + ": " + std::to_string(n) + " nodes, at most 2^30 (the transform of 2^p >= 2n - 1 points is indexed with 32 bits)");
    return PS_OK;
}

// one identity point: every answer on a domain of one node (the polynomial is a constant)
static int kzg_all_identity(ps_ctx* c, const std::string& who, ps_points** out) {
    int rc = points_alloc(c, PS_G1, 1, out);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync((*out)->st->p, 0, sizeof(Affine<Fp>), c->stream);
    if (e != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(PS_ERR_HIP, who + ": hipMemsetAsync: " + hipGetErrorString(e));
    return PS_OK;
}

// kh <- the stored transform of the wrapped kappa, unscaled (S = 2^p scalars, p >= 1)
static hipError_t kzg_all_kappa_hat(const NttTables& tb, hipStream_t st, const ps_qap* q, Fr* kh, int p) {
    hipLaunchKernelGGL(k_kzg_all_kappa, dim3(nblk(1ull << p)), dim3(256), 0, st, kh, (const Fr*)q->qt.fact2, (const Fr*)q->qt.invfact, (u64)q->n, p);
    return ntt_run<false>(tb, st, kh, 1ull << p, p);
}

// *out (the caller's scope owns it) = K_m, m = 1 .. n.  Arguments validated.  Returns with the stream idle.
static int kzg_all_key_run(ps_ctx* c, const std::string& who, const ps_qap* q, const ps_points* lag_g1, ps_points** out) {
    typedef Fp F;
    typedef KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = q->n;
    if (n == 1) return kzg_all_identity(c, who, out);
    const int p = kzg_all_log(n);
    const u32 S = (u32)kzg_all_size(n);
    hipStream_t st = c->stream;
    NttTables& tb = *ctx_tabs(c);
    hipError_t e = ntt_tables_ensure(tb, p, st);
    if (e != hipSuccess) return fail(PS_ERR_HIP, who + ": twiddles: " + hipGetErrorString(e));
    int rc = points_alloc(c, PS_G1, n, out);
    if (rc) return rc;
    Scope scope(st);
    Xyzz<F>* A = nullptr;  // S points; the chain products of the batch normalisation go behind the first n (kzg_all_normalise_fits)
    Fr* kh = nullptr;
    if ((e = scope.device(&A, kzg_all_point_elems(n))) != hipSuccess || (e = scope.device(&kh, kzg_all_kappa_elems(n))) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
    if (storage_wait_ready(lag_g1->st, st)) return fail(PS_ERR_HIP, who + ": event wait failed");
    if ((e = kzg_all_kappa_hat(tb, st, q, kh, p)) != hipSuccess) return fail(PS_ERR_HIP, who + ": ntt: " + hipGetErrorString(e));
    hipLaunchKernelGGL(k_fr_scale, dim3(nblk(S)), dim3(256), 0, st, kh, (const Fr*)kh, fr_inv2pow_host(p), (u64)S);
    hipLaunchKernelGGL(k_ec_from_affine<KF>, dim3(nblocks((size_t)S * LN)), dim3(256), 0, st, (const Affine<F>*)points_ptr(lag_g1), (u32)n, S, A);
    ec_correlate<F>(tb, st, A, S, p, kh);
    batch_to_affine<F>(st, (char*)A, n, (char*)(*out)->st->p, (u32)sizeof(Affine<F>));
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, who + ": kernels: " + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(PS_ERR_HIP, who + ": run: " + hipGetErrorString(e));
    return scope.finish(PS_OK);
}

enum { KZG_ALL_STAGES = 7 };  // the scalar side, load, forward, pointwise, inverse, combine, normalise
struct KzgAllMarks {
    hipEvent_t ev[KZG_ALL_STAGES + 1] = {};
    bool on = false;
    hipError_t create() {
        on = true;
        for (hipEvent_t& x : ev)
            if (hipError_t e = hipEventCreate(&x)) return e;
        return hipSuccess;
    }
    void mark(int i, hipStream_t st) { if (on) (void)hipEventRecord(ev[i], st); }
    ~KzgAllMarks() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); }
};

// *proofs (the caller's scope owns it) = pi_m, m = 1 .. n, over a key table that is there.  Arguments validated.  Returns with the
// stream idle.  stage_ms != nullptr: KZG_ALL_STAGES times from events between the stages.
static int kzg_all_open_run(ps_ctx* c, const std::string& who, const ps_qap* q, const ps_points* lag_g1, const ps_points* key, const ps_scalars* values,
                            ps_points** proofs, float* stage_ms = nullptr) {
    typedef Fp F;
    typedef KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = q->n;
    const int p = kzg_all_log(n);
    const u32 S = (u32)kzg_all_size(n);
    hipStream_t st = c->stream;
    NttTables& tb = *ctx_tabs(c);
    hipError_t e = ntt_tables_ensure(tb, p, st);
    if (e != hipSuccess) return fail(PS_ERR_HIP, who + ": twiddles: " + hipGetErrorString(e));
    int rc = points_alloc(c, PS_G1, n, proofs);
    if (rc) return rc;
    KzgAllMarks marks;
    if (stage_ms && (e = marks.create()) != hipSuccess) return fail(PS_ERR_HIP, who + ": hipEventCreate: " + hipGetErrorString(e));
    Scope scope(st);
    Xyzz<F>* A = nullptr;  // S points: v_i L_i, then U_m, then pi_m; the chain products of the normalisation go behind the first n
    Fr *kh = nullptr, *x = nullptr, *vm = nullptr, *g = nullptr;
    if ((e = scope.device(&A, kzg_all_point_elems(n))) != hipSuccess || (e = scope.device(&kh, kzg_all_kappa_elems(n))) != hipSuccess ||
        (e = scope.device(&x, kzg_all_scalar_elems(n))) != hipSuccess || (e = scope.device(&vm, kzg_all_value_elems(n))) != hipSuccess ||
        (e = scope.device(&g, kzg_all_value_elems(n))) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": hipMalloc: " + hipGetErrorString(e));
    if (storage_wait_ready(lag_g1->st, st) || storage_wait_ready(key->st, st) || storage_wait_ready(values->st, st))
        return fail(PS_ERR_HIP, who + ": event wait failed");
    const Affine<F>*lag = (const Affine<F>*)points_ptr(lag_g1), *kp = (const Affine<F>*)points_ptr(key);
    marks.mark(0, st);
    // the scalar side: kappa's stored transform, [w.v | w] convolved with it as a batch of two, g; then 2^-p into the stored
    // transform for the inverse over points, which does not scale
    if ((e = kzg_all_kappa_hat(tb, st, q, kh, p)) != hipSuccess) return fail(PS_ERR_HIP, who + ": ntt: " + hipGetErrorString(e));
    hipLaunchKernelGGL(k_kzg_all_weights, dim3(nblk(kzg_all_scalar_elems(n))), dim3(256), 0, st, x, vm, scalars_ptr(values), (const Fr*)q->qt.invfact, (u64)n, p);
    if ((e = ntt_conv(tb, st, x, kzg_all_scalar_elems(n), p, NttFuse(), NttFuse(), kh, (u64)S - 1)) != hipSuccess)
        return fail(PS_ERR_HIP, who + ": ntt: " + hipGetErrorString(e));
    hipLaunchKernelGGL(k_kzg_all_finish, dim3(nblk(n)), dim3(256), 0, st, g, (const Fr*)x, (const Fr*)vm, (const Fr*)q->qt.fact2, (u64)n, p);
    hipLaunchKernelGGL(k_fr_scale, dim3(nblk(S)), dim3(256), 0, st, kh, (const Fr*)kh, fr_inv2pow_host(p), (u64)S);
    marks.mark(1, st);
    // the points: U = the correlation of v_i L_i, combined per node with the key table and the string
    hipLaunchKernelGGL(k_kzg_all_load<KF>, dim3(nblocks((size_t)S * LN)), dim3(256), 0, st, lag, (const Fr*)vm, (u32)n, S, A);
    marks.mark(2, st);
    ec_correlate<F>(tb, st, A, S, p, kh, marks.on ? marks.ev + 3 : nullptr);
    marks.mark(5, st);
    hipLaunchKernelGGL(k_kzg_all_combine<KF>, dim3(nblocks(n * LN)), dim3(256), 0, st, A, kp, lag, (const Fr*)vm, (const Fr*)g, (u32)n);
    marks.mark(6, st);
    batch_to_affine<F>(st, (char*)A, n, (char*)(*proofs)->st->p, (u32)sizeof(Affine<F>));
    marks.mark(7, st);
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, who + ": kernels: " + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(PS_ERR_HIP, who + ": run: " + hipGetErrorString(e));
    for (int i = 0; stage_ms && i < KZG_ALL_STAGES; i++)
        if ((e = hipEventElapsedTime(&stage_ms[i], marks.ev[i], marks.ev[i + 1])) != hipSuccess) return fail(PS_ERR_HIP, who + ": events: " + hipGetErrorString(e));
    return scope.finish(PS_OK);
}

extern "C" int ps_kzg_all_key_lagrange(ps_ctx* c, const ps_qap* q, const ps_points* lag_g1, ps_points** out) {
    const std::string who = "ps_kzg_all_key_lagrange";
    if (!c || !q || !lag_g1 || !out) return fail(PS_ERR_ARG, who + ": NULL argument");
    *out = nullptr;
    int rc = kzg_all_args(who, q, lag_g1, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    return scope.finish(kzg_all_key_run(c, who, q, lag_g1, scope.result(out)));
}

static int kzg_all_open(ps_ctx* c, const std::string& who, const ps_qap* q, const ps_points* lag_g1, const ps_points* all_key, const ps_scalars* values,
                        ps_points** proofs, float* stage_ms) {
    if (!c || !q || !lag_g1 || !values || !proofs) return fail(PS_ERR_ARG, who + ": NULL argument");
    *proofs = nullptr;
    int rc = kzg_all_args(who, q, lag_g1, all_key, values);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    if (q->n == 1) {
        for (int i = 0; stage_ms && i < KZG_ALL_STAGES; i++) stage_ms[i] = 0.f;
        return scope.finish(kzg_all_identity(c, who, scope.result(proofs)));
    }
    if (!all_key) {  // computed inside the call and dropped
        ps_points** slot = scope.points();
        if ((rc = kzg_all_key_run(c, who, q, lag_g1, slot))) return rc;
        all_key = *slot;
    }
    return scope.finish(kzg_all_open_run(c, who, q, lag_g1, all_key, values, scope.result(proofs), stage_ms));
}

extern "C" int ps_kzg_open_all_lagrange(ps_ctx* c, const ps_qap* q, const ps_points* lag_g1, const ps_points* all_key, const ps_scalars* values,
                                        ps_points** proofs) {
    return kzg_all_open(c, "ps_kzg_open_all_lagrange", q, lag_g1, all_key, values, proofs, nullptr);
}

// Measurement hook (not in the header, like ps_debug_points_scale): ps_kzg_open_all_lagrange with the times of its stages in
// ms[0 .. 6] -- the scalar side, load, forward, pointwise, inverse, combine, normalise (tools/kzg_all_sweep.py).
extern "C" int ps_debug_kzg_all_stage_ms(ps_ctx* c, const ps_qap* q, const ps_points* lag_g1, const ps_points* all_key, const ps_scalars* values,
                                         ps_points** proofs, float* ms) {
    if (!ms) return fail(PS_ERR_ARG, "ps_debug_kzg_all_stage_ms: NULL argument");
    return kzg_all_open(c, "ps_debug_kzg_all_stage_ms", q, lag_g1, all_key, values, proofs, ms);
}
