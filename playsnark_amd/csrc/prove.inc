// QAP quotient and whole-prover entry points of the C ABI (included by capi.hip).
//
//   ps_qap_create / ps_qap_quotient  <- ToQAP + QAP.Quotient + computeAggregatePoly (qap.go:35-175)
//   ps_groth16_prove                 <- Groth16Prove (groth16.go:122-211)
//   (ps_phgr13_prove, PHGR13Prove, is in prove_shares.inc: the whole key is rank 0 of 1 of the share prover)
//   ps_poly_mul                      <- Poly.Mul     (algebra.go:92-105)

struct DevCsr {
    u32* row_ptr = nullptr;
    u32* col = nullptr;
    Fr* val = nullptr;  // Montgomery
    size_t nnz = 0;
    u32* long_rows = nullptr;  // rows with more than SPMV_LONG_ROW non-zeros
    u32 n_long = 0;
    // The long rows of a TRANSPOSED matrix once more, split for the column sums over points (srs_setup.inc): those without a
    // wide entry (coef_width.hpp), on the device, and on the host (row, first entry, entries) those that hold one
    u32* long_narrow = nullptr;
    u32 n_long_narrow = 0;
    std::vector<u32> long_wide_h;
};

static void spmv_launch(hipStream_t st, const DevCsr& m, const Fr* x, Fr* y, u32 rows) {
    hipLaunchKernelGGL(k_spmv, dim3(nblk(rows)), dim3(256), 0, st, m.row_ptr, m.col, m.val, x, y, rows);
    if (m.n_long)
        hipLaunchKernelGGL(k_spmv_long_rows, dim3(m.n_long), dim3(256), 0, st, m.row_ptr, m.col, m.val, x, y, m.long_rows);
}

struct ps_qap {
    int device;
    size_t n, m, nio;
    DevCsr mat[3];
    DevCsr matT[3];        // transposes (rows = variables): u_i(x) = sum_j M[j][i] l_j(x) for the setup
    QapTables qt;
    Fr* sol_m = nullptr;   // m   : witness in Montgomery form
    Fr* y[3] = {nullptr, nullptr, nullptr};  // n each: L.s, R.s, O.s
    Fr* coefA = nullptr;   // n
    Fr* coefB = nullptr;   // n
    Fr* coefC = nullptr;   // n
    Fr* hbuf = nullptr;    // n-1
    // rows that are long in ANY of the three matrices, ascending (k_own_rows_long): on the device, and on the host so that a
    // prover can cut the list to its range of rows
    u32* long_any = nullptr;
    std::vector<u32> long_any_h;
    size_t wide[3] = {0, 0, 0};  // per matrix: entries whose signed magnitude needs more than 64 bits (coef_width.hpp)
    std::vector<void*> owned;
};

static NttTables* ctx_tabs(ps_ctx* c) {
    if (!c->qcache) c->qcache = new QuotientCache();
    return &c->qcache->tabs;
}

template <class T>
static int dev_alloc(ps_qap* q, T** p, size_t count) {
    hipError_t e = hipMalloc((void**)p, sizeof(T) * std::max<size_t>(count, 1));
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("hipMalloc qap: ") + hipGetErrorString(e));
    q->owned.push_back(*p);
    return PS_OK;
}

extern "C" void ps_qap_free(ps_qap* q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    (void)hipDeviceSynchronize();
    for (void* p : q->owned) (void)hipFree(p);
    q->qt.free_all();
    delete q;
}

static Fr fr_mont_from_be32(const uint8_t* be);

// One matrix as either entry point gives it: int64 coefficients (ps_csr) or canonical big-endian field elements (ps_csr_fr)
struct CsrSource {
    const uint32_t* row_ptr;
    const uint32_t* col;
    const int64_t* val;       // ps_qap_create
    const uint8_t* val_be32;  // ps_qap_create_fr
    bool fr;
};

// ps_qap_create and ps_qap_create_fr: the argument checks (same order, codes and texts for both), the host preparation
// and the upload.  Only the coefficient source differs.
static int qap_create_from(ps_ctx* c, size_t n, size_t m, size_t nio, const CsrSource* src, ps_qap** out) {
    if (n == 0 || m == 0 || nio > m) return fail(PS_ERR_ARG, "ps_qap_create: bad dimensions");
    if (n >= (1ull << 27)) return fail(PS_ERR_ARG, "ps_qap_create: more than 2^27 gates is not supported");
    HIP_TRY(hipSetDevice(c->device));
    ps_qap* q = new ps_qap();
    q->device = c->device;
    q->n = n; q->m = m; q->nio = nio;
    int rc = PS_OK;
    for (int k = 0; k < 3; k++)
        if (!src[k].row_ptr) { delete q; return fail(PS_ERR_ARG, "ps_qap_create: NULL row_ptr"); }
    // Host preparation of the three matrices and of the factorial tables on four threads: coefficient
    // conversion (Value.ToFieldElement, curve.go:17-19, or the canonical bytes) to Montgomery form, the transpose
    // (counting sort by column; rows = variables, for the setups' per-variable sums) and the long-row lists.
    struct HostCsr {
        bool bad_col = false, bad_val = false, no_val = false;
        size_t wide = 0;
        std::vector<Fr> vals, tv;
        std::vector<u32> tp, tc, lr, lrT, lrT_narrow, lrT_wide;
    };
    auto prepare = [n, m](const CsrSource* s) {
        HostCsr h;
        const size_t nnz = s->row_ptr[n];
        for (size_t e = 0; e < nnz; e++)
            if (s->col[e] >= m) { h.bad_col = true; return h; }
        h.vals.resize(nnz);
        std::vector<u32> wide_in_col(m, 0);
        if (s->fr) {
            if (nnz && !s->val_be32) { h.no_val = true; return h; }
            for (size_t e = 0; e < nnz; e++) {
                const uint8_t* be = s->val_be32 + 32 * e;
                if (!coef_be32_is_canonical(be)) { h.bad_val = true; return h; }
                u32 v[8], mag[8];
                limbs_from_be<8>(v, be);
                (void)coef_signed_magnitude(mag, v);
                if (coef_is_wide(mag)) { h.wide++; wide_in_col[s->col[e]]++; }
                h.vals[e] = fr_mont_from_be32(be);
            }
        } else {
            for (size_t e = 0; e < nnz; e++) {
                int64_t v = s->val[e];
                u64 mag = v < 0 ? (u64)0 - (u64)v : (u64)v;
                Fr a = fr_from_u64(mag);
                h.vals[e] = v < 0 ? fr_neg(a) : a;
            }
        }
        h.tp.assign(m + 1, 0); h.tc.resize(nnz); h.tv.resize(nnz);
        for (size_t e = 0; e < nnz; e++) h.tp[s->col[e] + 1]++;
        for (size_t i = 0; i < m; i++) h.tp[i + 1] += h.tp[i];
        std::vector<u32> fill(h.tp.begin(), h.tp.end() - 1);
        for (size_t g = 0; g < n; g++)
            for (u32 e = s->row_ptr[g]; e < s->row_ptr[g + 1]; e++) {
                u32 pos = fill[s->col[e]]++;
                h.tc[pos] = (u32)g;
                h.tv[pos] = h.vals[e];
            }
        for (size_t r = 0; r < m; r++)
            if (h.tp[r + 1] - h.tp[r] > SPMV_LONG_ROW) {
                h.lrT.push_back((u32)r);
                if (wide_in_col[r]) h.lrT_wide.insert(h.lrT_wide.end(), {(u32)r, h.tp[r], h.tp[r + 1] - h.tp[r]});
                else h.lrT_narrow.push_back((u32)r);
            }
        for (size_t r = 0; r < n; r++)
            if (s->row_ptr[r + 1] - s->row_ptr[r] > SPMV_LONG_ROW) h.lr.push_back((u32)r);
        return h;
    };
    std::future<HostCsr> prep[3];
    for (int k = 0; k < 3; k++) prep[k] = std::async(std::launch::async, prepare, &src[k]);
    std::future<FactTables> facts = std::async(std::launch::async, fact_tables, qap_np(n));
    auto upload = [&](auto** dst, const auto& v) -> int {
        typedef typename std::remove_reference<decltype(v[0])>::type T;
        int r2 = dev_alloc(q, (typename std::remove_const<T>::type**)dst, v.size());
        if (r2) return r2;
        if (!v.empty() && hipMemcpy(*dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(PS_ERR_HIP, "hipMemcpy of a CSR array failed");
        return PS_OK;
    };
    for (int k = 0; k < 3; k++) {
        HostCsr h = prep[k].get();  // always collected, also after an error
        if (rc) continue;
        if (h.bad_col) { rc = fail(PS_ERR_ARG, "ps_qap_create: column index out of range"); continue; }
        if (h.no_val) { rc = fail(PS_ERR_ARG, "ps_qap_create_fr: NULL val_be32"); continue; }
        if (h.bad_val) { rc = fail(PS_ERR_ENCODING, "ps_qap_create_fr: coefficient not below r"); continue; }
        const CsrSource* s = &src[k];
        const size_t nnz = s->row_ptr[n];
        q->wide[k] = h.wide;
        DevCsr& d = q->mat[k];
        DevCsr& t = q->matT[k];
        d.nnz = t.nnz = nnz;
        d.n_long = (u32)h.lr.size();
        t.n_long = (u32)h.lrT.size();
        if ((rc = dev_alloc(q, &d.row_ptr, n + 1))) continue;
        if ((rc = dev_alloc(q, &d.col, nnz))) continue;
        hipError_t e1 = hipMemcpy(d.row_ptr, s->row_ptr, 4 * (n + 1), hipMemcpyHostToDevice);
        hipError_t e2 = nnz ? hipMemcpy(d.col, s->col, 4 * nnz, hipMemcpyHostToDevice) : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess) { rc = fail(PS_ERR_HIP, "hipMemcpy of the CSR matrices failed"); continue; }
        if ((rc = upload(&d.val, h.vals))) continue;
        if ((rc = upload(&t.row_ptr, h.tp))) continue;
        if ((rc = upload(&t.col, h.tc))) continue;
        if ((rc = upload(&t.val, h.tv))) continue;
        if (d.n_long && (rc = upload(&d.long_rows, h.lr))) continue;
        if (t.n_long && (rc = upload(&t.long_rows, h.lrT))) continue;
        t.n_long_narrow = (u32)h.lrT_narrow.size();
        if (t.n_long_narrow && (rc = upload(&t.long_narrow, h.lrT_narrow))) continue;
        t.long_wide_h = h.lrT_wide;
        q->long_any_h.insert(q->long_any_h.end(), h.lr.begin(), h.lr.end());
    }
    if (rc == PS_OK && !q->long_any_h.empty()) {
        std::sort(q->long_any_h.begin(), q->long_any_h.end());
        q->long_any_h.erase(std::unique(q->long_any_h.begin(), q->long_any_h.end()), q->long_any_h.end());
        rc = upload(&q->long_any, q->long_any_h);
    }
    FactTables ft = facts.get();
    if (rc == PS_OK) rc = dev_alloc(q, &q->sol_m, m);
    for (int k = 0; k < 3 && rc == PS_OK; k++) rc = dev_alloc(q, &q->y[k], n);
    if (rc == PS_OK) rc = dev_alloc(q, &q->coefA, n);
    if (rc == PS_OK) rc = dev_alloc(q, &q->coefB, n);
    if (rc == PS_OK) rc = dev_alloc(q, &q->coefC, n);
    if (rc == PS_OK) rc = dev_alloc(q, &q->hbuf, n);
    if (rc == PS_OK) {
        hipError_t e = qap_tables_build(*ctx_tabs(c), c->stream, q->qt, n, &ft);
        if (e != hipSuccess) rc = fail(PS_ERR_HIP, std::string("building the per-n QAP tables: ") + hipGetErrorString(e));
    }
    if (rc != PS_OK) {
        KeepError keep;
        ps_qap_free(q);
        return rc;
    }
    *out = q;
    return PS_OK;
}

extern "C" int ps_qap_create(ps_ctx* c, size_t n, size_t m, size_t nio, const ps_csr* L, const ps_csr* R, const ps_csr* O,
                             ps_qap** out) {
    if (!c || !L || !R || !O || !out) return fail(PS_ERR_ARG, "ps_qap_create: NULL argument");
    const CsrSource src[3] = {{L->row_ptr, L->col, L->val, nullptr, false},
                                {R->row_ptr, R->col, R->val, nullptr, false},
                                {O->row_ptr, O->col, O->val, nullptr, false}};
    return qap_create_from(c, n, m, nio, src, out);
}

// The same circuit with coefficients given as field elements: 32-byte canonical big-endian values (ps_scalars_upload's format)
extern "C" int ps_qap_create_fr(ps_ctx* c, size_t n, size_t m, size_t nio, const ps_csr_fr* L, const ps_csr_fr* R, const ps_csr_fr* O,
                                ps_qap** out) {
    if (!c || !L || !R || !O || !out) return fail(PS_ERR_ARG, "ps_qap_create: NULL argument");
    const ps_csr_fr* in[3] = {L, R, O};
    CsrSource src[3];
    for (int k = 0; k < 3; k++) src[k] = {in[k]->row_ptr, in[k]->col, nullptr, in[k]->val_be32, true};
    return qap_create_from(c, n, m, nio, src, out);
}

extern "C" int ps_qap_wide_entries(const ps_qap* q, size_t out[3]) {
    if (!q || !out) return fail(PS_ERR_ARG, "ps_qap_wide_entries: NULL argument");
    for (int k = 0; k < 3; k++) out[k] = q->wide[k];
    return PS_OK;
}

// Fresh library-owned ps_scalars holding the plain-limb form of n Montgomery values
static int scalars_from_mont(ps_ctx* c, const Fr* src, size_t n, ps_scalars** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(32 * n, 32));
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    if (n) hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n)), dim3(256), 0, c->stream, (u32*)p, src, (u64)n);
    *out = scalars_adopt(c, p, n);
    return PS_OK;
}

// core: runs the pipeline, leaves A/B(/C)/h in q's buffers (Montgomery).
//   Q_AB     A, B coefficients and h = floor(A*B / z)        (Groth16Prove needs A and B)
//   Q_ABC    ... and the coefficients of C                    (computeAggregatePoly, qap.go:164-175)
//   Q_H_ONLY h alone, from its values on the nodes n+1..2n-1  (PHGR13Prove, QAP.Quotient)
enum QuotientMode { Q_AB, Q_ABC, Q_H_ONLY, Q_H_VALUES };  // Q_H_VALUES: h(n+1..2n-1) left in qt.scratch
static int quotient_run(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, QuotientMode mode) {
    if (sol->n != q->m)  // sanityCheck, qap.go:177-189
        return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const NttTables& tabs = *ctx_tabs(c);
    const u32 n = (u32)q->n;
    if (storage_wait_ready(sol->st, st)) return fail(PS_ERR_HIP, "quotient: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, st, q->sol_m, scalars_ptr(sol), (u64)q->m);
    for (int k = 0; k < 3; k++) spmv_launch(st, q->mat[k], (const Fr*)q->sol_m, q->y[k], n);
    HIP_TRY(hipMemsetAsync(c->d_flag, 0, 4, st));
    hipLaunchKernelGGL(k_check_gates, dim3(nblk(n)), dim3(256), 0, st, (const Fr*)q->y[0], (const Fr*)q->y[1],
                       (const Fr*)q->y[2], n, c->d_flag);
    HIP_TRY(hipGetLastError());
    hipError_t e;
    if (mode == Q_H_ONLY) {
        e = quotient_h_only(tabs, st, q->qt, q->y[0], q->y[1], q->y[2], q->hbuf);
    } else if (mode == Q_H_VALUES) {
        e = quotient_h_values(tabs, st, q->qt, q->y[0], q->y[1], q->y[2]);
    } else {
        Fr* dst[3] = {q->coefA, q->coefB, q->coefC};
        int k0 = 0;
        if (q->qt.s4) {  // small circuits: A and B as one batch of transforms
            e = interpolate2_on_1_to_n(tabs, st, q->qt, q->y[0], q->y[1], q->coefA, q->coefB);
            if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("interpolation: ") + hipGetErrorString(e));
            k0 = 2;
        }
        for (int k = k0; k < (mode == Q_ABC ? 3 : 2); k++) {
            e = interpolate_on_1_to_n(tabs, st, q->qt, q->y[k]);
            if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("interpolation: ") + hipGetErrorString(e));
            HIP_TRY(hipMemcpyAsync(dst[k], q->qt.data, sizeof(Fr) * n, hipMemcpyDeviceToDevice, st));
        }
        e = quotient_from_AB(tabs, st, q->qt, q->coefA, q->coefB, q->hbuf);
    }
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("quotient: ") + hipGetErrorString(e));
    u32 flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flag) return fail(PS_ERR_NOT_DIVISIBLE, "apocalypse");  // qap.go:158-160
    return PS_OK;
}

extern "C" int ps_qap_quotient(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, ps_scalars** A, ps_scalars** B,
                               ps_scalars** C, ps_scalars** h) {
    if (!c || !q || !sol) return fail(PS_ERR_ARG, "ps_qap_quotient: NULL argument");
    int rc = quotient_run(c, q, sol, C ? Q_ABC : (A || B) ? Q_AB : Q_H_ONLY);
    if (rc) return rc;
    if (A && (rc = scalars_from_mont(c, q->coefA, q->n, A))) return rc;
    if (B && (rc = scalars_from_mont(c, q->coefB, q->n, B))) return rc;
    if (C && (rc = scalars_from_mont(c, q->coefC, q->n, C))) return rc;
    if (h && (rc = scalars_from_mont(c, q->hbuf, q->n - 1, h))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PS_OK;
}

// (*QAP).IsValid (qap.go:107-148): "t = left*right - out divided by z leaves no remainder".  z has the simple roots
// 1..n, so that is y_A[j] y_B[j] == y_C[j] at every gate j -- the SpMVs and the gate check of the quotient, nothing else.
// sanityCheck's panic (qap.go:177-189) is PS_ERR_ARG.
extern "C" int ps_qap_is_valid(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, int* valid) {
    if (!c || !q || !sol || !valid) return fail(PS_ERR_ARG, "ps_qap_is_valid: NULL argument");
    *valid = 0;
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u32 n = (u32)q->n;
    if (storage_wait_ready(sol->st, st)) return fail(PS_ERR_HIP, "ps_qap_is_valid: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, st, q->sol_m, scalars_ptr(sol), (u64)q->m);
    for (int k = 0; k < 3; k++) spmv_launch(st, q->mat[k], (const Fr*)q->sol_m, q->y[k], n);
    HIP_TRY(hipMemsetAsync(c->d_flag, 0, 4, st));
    hipLaunchKernelGGL(k_check_gates, dim3(nblk(n)), dim3(256), 0, st, (const Fr*)q->y[0], (const Fr*)q->y[1],
                       (const Fr*)q->y[2], n, c->d_flag);
    HIP_TRY(hipGetLastError());
    u32 flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *valid = flag == 0;
    return PS_OK;
}

extern "C" int ps_poly_mul(ps_ctx* c, const ps_scalars* a, const ps_scalars* b, ps_scalars** out) {
    if (!c || !a || !b || !out) return fail(PS_ERR_ARG, "ps_poly_mul: NULL argument");
    if (a->n == 0 || b->n == 0) return fail(PS_ERR_LENGTH, "ps_poly_mul: empty polynomial");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    NttTables& tabs = *ctx_tabs(c);
    const u64 nout = a->n + b->n - 1;
    const int p = ilog2_ceil(nout);
    const u64 S = 1ull << p;
    HIP_TRY(ntt_tables_ensure(tabs, p, st));
    if (storage_wait_ready(a->st, st) || storage_wait_ready(b->st, st)) return fail(PS_ERR_HIP, "ps_poly_mul: event wait failed");
    Scope scope(st);
    Fr *ta = nullptr, *tb = nullptr, *am = nullptr, *bm = nullptr;
    HIP_TRY(scope.device(&ta, S));
    HIP_TRY(scope.device(&tb, S));
    HIP_TRY(scope.device(&am, a->n));
    HIP_TRY(scope.device(&bm, b->n));
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(a->n)), dim3(256), 0, st, am, scalars_ptr(a), (u64)a->n);
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(b->n)), dim3(256), 0, st, bm, scalars_ptr(b), (u64)b->n);
    hipError_t e = poly_mul_dev(tabs, st, am, a->n, bm, b->n, ta, nout, ta, tb);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("poly_mul: ") + hipGetErrorString(e));
    return scope.finish(scalars_from_mont(c, ta, nout, scope.result(out)));
}

// ---------------------------------------------------------------------------------------
// host glue shared by the two provers (the "6 single scalar-muls / ~12 adds" of groth16.go:149-200)
// ---------------------------------------------------------------------------------------
static void scalar_from_be32_host(u32 k[8], const uint8_t* be) {
    limbs_from_be<8>(k, be);
    for (int rep = 0; rep < 2; rep++) fe_reduce_once<FrParams>(k, 0);
}

template <class F>
static Xyzz<F> host_point(const uint8_t* p, bool& ok) {
    Affine<F> a;
    ok = ok && read_affine(a, p);
    if (!ok || affine_is_identity<F>(a)) return xyzz_identity<F>();
    return xyzz_from_affine<F>(a.x, a.y);
}

// run one MSM with a sub-range of a scalar vector
static int msm_range(ps_ctx* c, const ps_points* pts, const ps_scalars* sc, size_t first, size_t n, uint8_t* out) {
    Scope scope;
    ps_scalars** view = scope.scalars();
    int rc = ps_scalars_slice(sc, first, n, view);
    if (rc) return rc;
    return ps_msm(c, pts, *view, out);
}

// ---------------------------------------------------------------------------------------
// NewGroth16TrustedSetup (groth16.go:64-101) on the device, toxic waste supplied by the caller
// (the reference draws it with random.New(); a drop-in draws it the same way and passes it in).
// ---------------------------------------------------------------------------------------
static Fr fr_mont_from_be32(const uint8_t* be);
static Fr fr_host_pow2k(Fr base, int k) { for (int i = 0; i < k; i++) base = fr_mul(base, base); return base; }

template <class F>
static void host_fixed_base(uint8_t* out, const uint8_t* k_be32) {  // k * G on the host (Point.Mul(k, nil))
    u32 k[8];
    limbs_from_be<8>(k, k_be32);
    for (int rep = 0; rep < 2; rep++) fe_reduce_once<FrParams>(k, 0);
    Affine<F> g = generator((const F*)0);
    write_affine(out, xyzz_mul_scalar<F>(xyzz_from_affine<F>(g.x, g.y), k));
}

// Shared by both setups: device work buffers, z(x) and the per-variable evaluations
// u_i(x), v_i(x), w_i(x) = (M^T l(x))_i with l_j the Lagrange basis on {1..n} (qap.go:42-55).
struct SetupWork {
    hipStream_t st;
    Scope scope;  // the work buffers, and the key's arrays as results: released once the stream is idle
    explicit SetupWork(hipStream_t stream) : st(stream), scope(stream) {}
    Fr *pw = nullptr, *uvw[3] = {nullptr, nullptr, nullptr};
    Fr* lj = nullptr;  // l_j(x), j = 1..n: the Lagrange basis of the QAP domain at the secret point
    Fr zx;
    FrPow2Table tab;
    int alloc(Fr** p, size_t cnt) {
        hipError_t e = scope.device(p, cnt);
        if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("hipMalloc setup: ") + hipGetErrorString(e));
        return PS_OK;
    }
};

static int setup_var_evals(ps_ctx* c, const ps_qap* q, const Fr& x, const char* who, SetupWork& wk) {
    const size_t n = q->n, m = q->m;
    hipStream_t st = wk.st;
    // x in {1..n} would make a Lagrange denominator vanish (probability n/r for a random x)
    {
        u32 xw[8];
        fr_to_words8(xw, fr_from_mont(x));
        bool small = true;
        for (int i = 2; i < 8; i++) small = small && xw[i] == 0;
        u64 xv = (u64)xw[0] | ((u64)xw[1] << 32);
        if (small && xv >= 1 && xv <= n) return fail(PS_ERR_ARG, std::string(who) + ": the secret point lies on the interpolation domain {1..n}");
    }
    Fr *lj = nullptr, *partial = nullptr;
    const unsigned pblocks = nblk(n);
    int rc = PS_OK;
    if ((rc = wk.alloc(&wk.pw, std::max(n, m))) || (rc = wk.alloc(&lj, n)) || (rc = wk.alloc(&partial, pblocks))) return rc;
    wk.lj = lj;
    for (int k = 0; k < 3; k++) if ((rc = wk.alloc(&wk.uvw[k], m))) return rc;
    wk.tab.p[0] = x;
    for (int k = 1; k < 32; k++) wk.tab.p[k] = fr_mul(wk.tab.p[k - 1], wk.tab.p[k - 1]);
    // z(x) = prod (x - j)
    hipLaunchKernelGGL(k_prod_x_minus_j, dim3(pblocks), dim3(256), 0, st, partial, x, (u64)n);
    std::vector<Fr> hp(pblocks);
    HIP_TRY(hipMemcpyAsync(hp.data(), partial, sizeof(Fr) * pblocks, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    wk.zx = fr_one();
    for (auto& v : hp) wk.zx = fr_mul(wk.zx, v);
    // l_j(x), then u_i(x), v_i(x), w_i(x) for every variable
    hipLaunchKernelGGL(k_lagrange_at, dim3(nblk(n)), dim3(256), 0, st, lj, (const Fr*)q->qt.invfact, x, wk.zx, (u64)n);
    for (int k = 0; k < 3; k++) spmv_launch(st, q->matT[k], (const Fr*)lj, wk.uvw[k], (u32)m);
    HIP_TRY(hipGetLastError());
    return PS_OK;
}

// lambda_k(x), k = 1..n-1: the Lagrange basis of the nodes n+1..2n-1 at the secret point, into `out` (n-1 values).
// Equally spaced nodes: the basis of {off+1..off+cnt} at x is the basis of {1..cnt} at x - off.
static int setup_shifted_lagrange(ps_ctx* c, const ps_qap* q, const Fr& x, Fr* out) {
    const size_t n = q->n, cnt = n - 1;
    hipStream_t st = c->stream;
    const Fr xs = fr_norm(fr_sub(x, fr_from_u64(n)));
    {   // x on the shifted nodes would make a denominator vanish
        u32 xw[8];
        fr_to_words8(xw, fr_from_mont(fr_reduce(xs)));
        bool small = true;
        for (int i = 2; i < 8; i++) small = small && xw[i] == 0;
        u64 xv = (u64)xw[0] | ((u64)xw[1] << 32);
        if (small && xv >= 1 && xv <= cnt) return fail(PS_ERR_ARG, "setup: the secret point lies on the nodes n+1..2n-1");
    }
    const unsigned pblocks = nblk(cnt);
    std::vector<Fr> hp(pblocks);
    {
        Scope scope(st);
        Fr* partial = nullptr;
        HIP_TRY(scope.device(&partial, pblocks));
        hipLaunchKernelGGL(k_prod_x_minus_j, dim3(pblocks), dim3(256), 0, st, partial, xs, (u64)cnt);
        hipError_t e = hipMemcpyAsync(hp.data(), partial, sizeof(Fr) * pblocks, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("setup: ") + hipGetErrorString(e));
    }
    Fr zs = fr_one();
    for (auto& v : hp) zs = fr_mul(zs, v);
    hipLaunchKernelGGL(k_lagrange_at, dim3(nblk(cnt)), dim3(256), 0, st, out, (const Fr*)q->qt.invfact, xs, zs, (u64)cnt);
    HIP_TRY(hipGetLastError());
    return PS_OK;
}

// points = { src[i] * G } for a Montgomery-form device array
static int commit_mont(ps_ctx* c, int group, const Fr* src, size_t cnt, ps_points** out) {
    Scope scope;
    ps_scalars** sc = scope.scalars();
    int rc = scalars_from_mont(c, src, cnt, sc);
    if (rc) return rc;
    return ps_points_from_scalars(c, group, *sc, out);
}

extern "C" int ps_groth16_setup(ps_ctx* c, const ps_qap* q, const ps_groth16_toxic* tw, ps_groth16_crs* out) {
    if (!c || !q || !tw || !out) return fail(PS_ERR_ARG, "ps_groth16_setup: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    memset(out, 0, sizeof *out);
    const size_t n = q->n, m = q->m, diff = q->m - q->nio;
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_setup: needs at least 2 gates");
    hipStream_t st = c->stream;
    const Fr alpha = fr_mont_from_be32(tw->alpha), beta = fr_mont_from_be32(tw->beta), delta = fr_mont_from_be32(tw->delta),
             x = fr_mont_from_be32(tw->x), gamma = fr_mont_from_be32(tw->gamma);
    if (fr_is_zero(delta) || fr_is_zero(gamma)) return fail(PS_ERR_ARG, "ps_groth16_setup: delta and gamma must be non-zero");
    const Fr dinv = fr_inv(delta), ginv = fr_inv(gamma);
    SetupWork wk(st);
    for (ps_points** made : {&out->xi, &out->xi2, &out->xi_t, &out->io_lp, &out->nio_lp, &out->lxi, &out->lxi2, &out->lxi_t}) wk.scope.result(made);
    Fr* lin = nullptr;
    int rc = setup_var_evals(c, q, x, "ps_groth16_setup", wk);
    if (!rc) rc = wk.alloc(&lin, m);
    if (rc) return rc;
    Fr* pw = wk.pw;
    hipLaunchKernelGGL(k_linear_poly, dim3(nblk(m)), dim3(256), 0, st, lin, (const Fr*)wk.uvw[0], (const Fr*)wk.uvw[1],
                       (const Fr*)wk.uvw[2], alpha, beta, ginv, dinv, (u64)diff, (u64)m);
    // Xi, Xi2 = {x^i G}, i < n            (groth16.go:79-80)
    hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n)), dim3(256), 0, st, pw, wk.tab, fr_one(), (u64)n);
    if ((rc = commit_mont(c, PS_G1, pw, n, &out->xi))) return rc;
    if ((rc = commit_mont(c, PS_G2, pw, n, &out->xi2))) return rc;
    // XiT = {x^i t(x)/delta G}, i < n-1   (groth16.go:94-97)
    hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n - 1)), dim3(256), 0, st, pw, wk.tab, fr_mul(wk.zx, dinv), (u64)(n - 1));
    if ((rc = commit_mont(c, PS_G1, pw, n - 1, &out->xi_t))) return rc;
    // IoLP / NioLP                         (groth16.go:86-91)
    if ((rc = commit_mont(c, PS_G1, lin, diff, &out->io_lp))) return rc;
    if ((rc = commit_mont(c, PS_G1, lin + diff, m - diff, &out->nio_lp))) return rc;
    // the same CRS in Lagrange form (see ps_groth16_pk): l_j(x) G1, l_j(x) G2, lambda_k(x) t(x)/delta G1
    if ((rc = commit_mont(c, PS_G1, wk.lj, n, &out->lxi))) return rc;
    if ((rc = commit_mont(c, PS_G2, wk.lj, n, &out->lxi2))) return rc;
    if ((rc = setup_shifted_lagrange(c, q, x, pw))) return rc;
    hipLaunchKernelGGL(k_fr_scale, dim3(nblk(n - 1)), dim3(256), 0, st, pw, (const Fr*)pw, fr_mul(wk.zx, dinv), (u64)(n - 1));
    if ((rc = commit_mont(c, PS_G1, pw, n - 1, &out->lxi_t))) return rc;
    host_fixed_base<Fp>(out->alpha, tw->alpha);   // groth16.go:67-76
    host_fixed_base<Fp>(out->beta, tw->beta);
    host_fixed_base<Fp2>(out->beta2, tw->beta);
    host_fixed_base<Fp>(out->delta, tw->delta);
    host_fixed_base<Fp2>(out->delta2, tw->delta);
    host_fixed_base<Fp2>(out->gamma, tw->gamma);
    wk.scope.finish(PS_OK);  // (the key is the caller's from here, as it has been when this last wait fails)
    HIP_TRY(hipStreamSynchronize(st));
    return PS_OK;
}

// ---------------------------------------------------------------------------------------
// NewPHGR13TrustedSetup (pinochio.go:93-176) on the device.  Every CRS element is a known scalar
// times the generator: generateEvalCommit(base = r*G, polys, s, shift) (pinochio.go:381-388) is
// { (poly_k(s) * shift * r) * G }, so each array is one scaling kernel + one fixed-base kernel.
// ek.vs / ek.ws / ek.ys are the [diff:] slices of the verifier's full-length arrays (same storage).
// ---------------------------------------------------------------------------------------
static void fr_mont_to_be32(uint8_t* be, const Fr& a) {
    u32 w[8];
    fr_to_words8(w, fr_from_mont(a));
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) be[31 - 4 * i - b] = (uint8_t)(w[i] >> (8 * b));
}

extern "C" void ps_phgr13_crs_free(ps_phgr13_crs* k) {
    if (!k) return;
    ps_points** all[] = {&k->gsi, &k->vs, &k->ws, &k->ys, &k->vas, &k->was, &k->yas, &k->vbs, &k->wbs, &k->ybs,
                         &k->vk_vs, &k->vk_ws, &k->vk_ys, &k->lgsi};
    for (auto** p : all) { ps_points_free(*p); *p = nullptr; }
}

extern "C" int ps_phgr13_setup(ps_ctx* c, const ps_qap* q, const ps_phgr13_toxic* tw, ps_phgr13_crs* out) {
    if (!c || !q || !tw || !out) return fail(PS_ERR_ARG, "ps_phgr13_setup: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    memset(out, 0, sizeof *out);
    const size_t n = q->n, m = q->m, diff = q->m - q->nio, nn = m - diff;
    if (n < 2) return fail(PS_ERR_ARG, "ps_phgr13_setup: needs at least 2 gates");
    hipStream_t st = c->stream;
    const Fr s = fr_mont_from_be32(tw->s), av = fr_mont_from_be32(tw->av), aw = fr_mont_from_be32(tw->aw),
             ay = fr_mont_from_be32(tw->ay), rv = fr_mont_from_be32(tw->rv), rw = fr_mont_from_be32(tw->rw),
             beta = fr_mont_from_be32(tw->beta), gamma = fr_mont_from_be32(tw->gamma);
    const Fr ry = fr_mul(rv, rw);  // pinochio.go:117
    SetupWork wk(st);
    for (ps_points** made : {&out->gsi, &out->vs, &out->ws, &out->ys, &out->vas, &out->was, &out->yas, &out->vbs, &out->wbs, &out->ybs, &out->vk_vs,
                             &out->vk_ws, &out->vk_ys, &out->lgsi})
        wk.scope.result(made);
    int rc = setup_var_evals(c, q, s, "ps_phgr13_setup", wk);
    if (rc) return rc;
    auto scaled = [&](int group, const Fr* src, size_t first, size_t cnt, const Fr& scale, ps_points** dst) -> int {
        if (cnt) hipLaunchKernelGGL(k_fr_scale, dim3(nblk(cnt)), dim3(256), 0, st, wk.pw, src + first, scale, (u64)cnt);
        return commit_mont(c, group, wk.pw, cnt, dst);
    };
    // gsi = {s^i G}, i = 0..n-2                                         (pinochio.go:101)
    hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n - 1)), dim3(256), 0, st, wk.pw, wk.tab, fr_one(), (u64)(n - 1));
    if ((rc = commit_mont(c, PS_G1, wk.pw, n - 1, &out->gsi))) return rc;
    // ... and in Lagrange form on the nodes n+1..2n-1 (see ps_phgr13_ek.lgsi)
    if ((rc = setup_shifted_lagrange(c, q, s, wk.pw))) return rc;
    if ((rc = commit_mont(c, PS_G1, wk.pw, n - 1, &out->lgsi))) return rc;
    // g_v^(v_k(s)), g_w^(w_k(s)), g_y^(y_k(s)) for all k                 (:158-160)
    if ((rc = scaled(PS_G1, wk.uvw[0], 0, m, rv, &out->vk_vs))) return rc;
    if ((rc = scaled(PS_G2, wk.uvw[1], 0, m, rw, &out->vk_ws))) return rc;
    if ((rc = scaled(PS_G1, wk.uvw[2], 0, m, ry, &out->vk_ys))) return rc;
    // the prover's non-IO part                                           (:123-125)
    if ((rc = ps_points_slice(out->vk_vs, diff, nn, &out->vs))) return rc;
    if ((rc = ps_points_slice(out->vk_ws, diff, nn, &out->ws))) return rc;
    if ((rc = ps_points_slice(out->vk_ys, diff, nn, &out->ys))) return rc;
    // shifted by alpha                                                   (:127-129; was uses g1w = rw*G1)
    if ((rc = scaled(PS_G1, wk.uvw[0], diff, nn, fr_mul(rv, av), &out->vas))) return rc;
    if ((rc = scaled(PS_G1, wk.uvw[1], diff, nn, fr_mul(rw, aw), &out->was))) return rc;
    if ((rc = scaled(PS_G1, wk.uvw[2], diff, nn, fr_mul(ry, ay), &out->yas))) return rc;
    // shifted by beta                                                    (:135-137)
    if ((rc = scaled(PS_G1, wk.uvw[0], diff, nn, fr_mul(rv, beta), &out->vbs))) return rc;
    if ((rc = scaled(PS_G1, wk.uvw[1], diff, nn, fr_mul(rw, beta), &out->wbs))) return rc;
    if ((rc = scaled(PS_G1, wk.uvw[2], diff, nn, fr_mul(ry, beta), &out->ybs))) return rc;
    uint8_t k[32];
    host_fixed_base<Fp2>(out->av, tw->av);        // :144
    host_fixed_base<Fp>(out->aw, tw->aw);         // :146 (a G1 element in the reference as well)
    host_fixed_base<Fp2>(out->ay, tw->ay);        // :148
    host_fixed_base<Fp2>(out->gamma, tw->gamma);  // :150
    fr_mont_to_be32(k, fr_mul(gamma, beta));      // :139
    host_fixed_base<Fp>(out->bgamma, k);          // :152
    host_fixed_base<Fp2>(out->bgamma2, k);        // :153
    fr_mont_to_be32(k, fr_mul(wk.zx, ry));        // t(s) * r_y, :155-157
    host_fixed_base<Fp2>(out->yts, k);
    wk.scope.finish(PS_OK);  // (as in ps_groth16_setup)
    HIP_TRY(hipStreamSynchronize(st));
    return PS_OK;
}

// ---------------------------------------------------------------------------------------
// Groth16Prove (groth16.go:122-211), fused.  Everything the reference adds around its MSMs is
// itself a scalar multiple of a fixed CRS point, so the three proof elements are three MSMs:
//   A = sum A_j Xi_j + r*Delta + Alpha                       = MSM([A | r | 1],  [Xi  | Delta  | Alpha])
//   B = sum B_j Xi2_j + s*Delta2 + Beta2                     = MSM([B | s | 1],  [Xi2 | Delta2 | Beta2])
//   C = nio + htd + s*A + r*(B1 + s*Delta + Beta) - rs*Delta
//     = MSM([sol_nio | h | s*A + r*B | rs | s | r], [NioLP | XiT | Xi | Delta | Alpha | Beta])
// (expand s*A and r*B1 and collect the Delta terms: rs + rs - rs = rs).  Same group elements as
// the reference's statement-by-statement computation, one G1 MSM fewer and no host scalar
// multiplications.  The G2 MSM runs on a second stream with its own workspace, concurrently
// with the two G1 MSMs.
// ---------------------------------------------------------------------------------------
static int points_concat(ps_ctx* c, int group, const std::vector<std::pair<const void*, size_t>>& parts, ps_points** out) {
    size_t total = 0;
    for (auto& p : parts) total += p.second;
    int rc = points_alloc(c, group, total, out);
    if (rc) return rc;
    const size_t pb = point_bytes(group);
    size_t off = 0;
    for (auto& p : parts) {
        if (p.second) HIP_TRY(hipMemcpyAsync((char*)(*out)->st->p + off * pb, p.first, p.second * pb, hipMemcpyDeviceToDevice, c->stream));
        off += p.second;
    }
    return PS_OK;
}

template <class F>
static int upload_fixed_points(ps_ctx* c, int group, const std::vector<const uint8_t*>& enc, ps_points** out) {
    std::vector<uint8_t> raw;
    const size_t wb = wire_bytes(group);
    for (auto* e : enc) raw.insert(raw.end(), e, e + wb);
    return ps_points_upload(c, group, raw.data(), enc.size(), PS_FMT_AFFINE, out);
}

// Keys of PS_TABLE_MIN_POINTS points or more get window tables.  The threshold was 1024 until a kernel trace of PHGR13Prove on
// 2^10 constraints (1 021 non-IO variables: just under it) showed what the plain plan costs a small prover: 37 bucket sets per
// sum, a chain of doublings per set on the device (k_reduce_weights) and a 300-addition Horner fold per sum on the host --
// 2.8 ms per proof, a third of it after the GPU had finished.  A table is W x 128 bytes per point: nothing at these sizes.
#ifndef PS_TABLE_MIN_POINTS
#define PS_TABLE_MIN_POINTS 32
#endif
static bool tables_wanted(const ps_ctx* c, size_t n) { return c->use_tables && n >= PS_TABLE_MIN_POINTS && n < (1ull << ENTRY_W_SHIFT) - 4; }

// Cached per proving key: PA = [Xi | Delta | Alpha], PB = [Xi2 | Delta2 | Beta2],
// PC = [NioLP | XiT | Xi | Delta | Alpha | Beta], each with its window table when the key is large enough.
static bool g16_lagrange(const ps_groth16_pk* pk) { return pk->lxi && pk->lxi2 && pk->lxi_t; }
static int groth16_prepare(ps_ctx* c, const ps_groth16_pk* pk, size_t n, size_t nn, bool split) {
    // with the Lagrange form of the key present the sums run over it (scalars: values on the nodes, not coefficients)
    const bool lag = g16_lagrange(pk);
    const ps_points *xi = lag ? pk->lxi : pk->xi, *xi2 = lag ? pk->lxi2 : pk->xi2, *xi_t = lag ? pk->lxi_t : pk->xi_t;
    const unsigned long long key[4] = {xi->uid, xi2->uid, pk->nio_lp->uid, xi_t->uid};
    uint8_t fixed[sizeof(c->g16_fixed)];
    memcpy(fixed, pk->alpha, 96); memcpy(fixed + 96, pk->beta, 96); memcpy(fixed + 192, pk->delta, 96);
    memcpy(fixed + 288, pk->beta2, 192); memcpy(fixed + 480, pk->delta2, 192);
    const bool tabs = tables_wanted(c, 3 * n + nn);
    if (c->g16_pa && !memcmp(key, c->g16_key, sizeof key) && !memcmp(fixed, c->g16_fixed, sizeof fixed) && c->g16_tabs == tabs &&
        c->g16_split == split)
        return PS_OK;
    auto drop = [&]() {
        if (c->g16_pa) { ps_points_free(c->g16_pa); c->g16_pa = nullptr; }
        if (c->g16_pb) { ps_points_free(c->g16_pb); c->g16_pb = nullptr; }
        if (c->g16_pc) { ps_points_free(c->g16_pc); c->g16_pc = nullptr; }
    };
    drop();
    if (xi->group != PS_G1 || pk->nio_lp->group != PS_G1 || xi_t->group != PS_G1 || xi2->group != PS_G2)
        return fail(PS_ERR_ARG, "ps_groth16_prove: CRS array in the wrong group");
    if (xi->n != n || xi2->n != n || xi_t->n + 1 != n)  // algebra.go:350-352 would panic
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(n) + " and blinded eval points " +
                                       std::to_string(xi->n));
    Scope scope;
    ps_points **fa = scope.points(), **fb = scope.points(), **fc = scope.points();
    int rc;
    for (const ps_points* arr : {xi, xi2, pk->nio_lp, xi_t})
        if (storage_wait_ready(arr->st, c->stream)) return fail(PS_ERR_HIP, "ps_groth16_prove: event wait failed");
    if ((rc = upload_fixed_points<Fp>(c, PS_G1, {pk->delta, pk->alpha}, fa))) return rc;
    if ((rc = upload_fixed_points<Fp2>(c, PS_G2, {pk->delta2, pk->beta2}, fb))) return rc;
    if (split) rc = upload_fixed_points<Fp>(c, PS_G1, {pk->beta}, fc);
    else rc = upload_fixed_points<Fp>(c, PS_G1, {pk->delta, pk->alpha, pk->beta}, fc);
    if (rc) return rc;
    rc = points_concat(c, PS_G1, {{points_ptr(xi), n}, {points_ptr(*fa), 2}}, &c->g16_pa);
    if (!rc) rc = points_concat(c, PS_G2, {{points_ptr(xi2), n}, {points_ptr(*fb), 2}}, &c->g16_pb);
    // split form of C (groth16_prove_impl): PC = [NioLP | XiT | Beta], no third copy of Xi
    if (!rc && split) rc = points_concat(c, PS_G1, {{points_ptr(pk->nio_lp), nn}, {points_ptr(xi_t), n - 1}, {points_ptr(*fc), 1}}, &c->g16_pc);
    else if (!rc) rc = points_concat(c, PS_G1, {{points_ptr(pk->nio_lp), nn}, {points_ptr(xi_t), n - 1}, {points_ptr(xi), n}, {points_ptr(*fc), 3}},
                                     &c->g16_pc);
    (void)hipStreamSynchronize(c->stream);  // the copies out of fa, fb, fc are complete
    // window tables when there is room for them (13 rows of 128 / 256 B per point): a table that does not fit is not an
    // error -- the sums over that array take the plain plan, which needs no memory beyond the array itself
    if (!rc && tabs) {
        rc = points_ensure_table(c, c->g16_pa, 0, true);
        if (!rc) rc = points_ensure_table(c, c->g16_pb, 0, true);
        if (!rc) rc = points_ensure_table(c, c->g16_pc, 0, true);
    }
    if (rc) { drop(); return rc; }  // nothing half-made stays behind without its key
    memcpy(c->g16_key, key, sizeof key);
    memcpy(c->g16_fixed, fixed, sizeof fixed);
    c->g16_tabs = tabs;
    c->g16_split = split;
    return PS_OK;
}

static Fr fr_mont_from_be32(const uint8_t* be) {
    u32 w[8];
    limbs_from_be<8>(w, be);
    for (int rep = 0; rep < 2; rep++) fe_reduce_once<FrParams>(w, 0);
    return fr_to_mont(fr_from_words8(w));
}

// The provers' loose scalars in device memory (one synchronous 256-byte copy before anything is enqueued):
// slot 0: r, 1: s, 2: r*s, 3: 1 -- plain limbs, copied device-to-device into the tails of the sum vectors.
static int groth16_small_scalars(ps_ctx* c, const uint8_t* r_be32, const uint8_t* s_be32, Fr* rm, Fr* sm) {
    if (!c->d_small) HIP_TRY(hipMalloc(&c->d_small, 256));
    *rm = fr_mont_from_be32(r_be32);
    *sm = fr_mont_from_be32(s_be32);
    u32 host[8][8];
    memset(host, 0, sizeof host);
    fr_to_words8(host[0], fr_from_mont(*rm));
    fr_to_words8(host[1], fr_from_mont(*sm));
    fr_to_words8(host[2], fr_from_mont(fr_mul(*rm, *sm)));
    host[3][0] = 1;
    HIP_TRY(hipMemcpy(c->d_small, host, sizeof host, hipMemcpyHostToDevice));
    return PS_OK;
}
static inline const u32* small_slot(const ps_ctx* c, int i) { return (const u32*)c->d_small + 8 * i; }

// Groth16Prove as three sums (see the header of this section):
//   SA = [A | r | 1] . PA,   SB = [B | s | 1] . PB (G2),   SC = [sol_nio | h | sA + rB | rs | s | r] . PC
// The quotient runs first, alone, on the context's high-priority stream; the sums follow on the workers (the workspaces beside the context's own).
// Running them beside each other was measured and dropped (n = 2^20): sums that need no polynomial started at once made
// the quotient 2.4 x slower (11.9 -> 29 ms) for the same total -- the NTT passes are VALU-bound by instructions, the
// bucket accumulations by multiplications, so neither has idle issue slots to lend -- and even the digit sorts alone
// (LDS / memory-bound, but 140 KB of LDS per workgroup) cost the quotient 2.7 ms for 0.7 ms of sorting hidden.
struct G16Vectors { ps_scalars *SA = nullptr, *SB = nullptr, *SC = nullptr; };  // borrowed: the vectors are the context's (prover_vector, capi.hip)

// stage 0: SpMV + gate check; 1: A interpolated, SA ready; 2: B interpolated, SB ready; 3: h, SC ready.
static int g16_quotient_stage(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, hipStream_t qs, int stage, const Fr& rm, const Fr& sm,
                              size_t diff, size_t nn, bool lag, bool split, G16Vectors& v) {
    const NttTables& tabs = *ctx_tabs(c);
    const u32 n = (u32)q->n;
    hipError_t e = hipSuccess;
    auto d2d = [&](u32* dst, int slot) { return hipMemcpyAsync(dst, small_slot(c, slot), 32, hipMemcpyDeviceToDevice, qs); };
    if (stage == 0) {
        if (storage_wait_ready(sol->st, qs)) return fail(PS_ERR_HIP, "quotient: event wait failed");
        hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, qs, q->sol_m, scalars_ptr(sol), (u64)q->m);
        for (int k = 0; k < 3; k++) spmv_launch(qs, q->mat[k], (const Fr*)q->sol_m, q->y[k], n);
        HIP_TRY(hipMemsetAsync(c->d_flag, 0, 4, qs));
        hipLaunchKernelGGL(k_check_gates, dim3(nblk(n)), dim3(256), 0, qs, (const Fr*)q->y[0], (const Fr*)q->y[1], (const Fr*)q->y[2], n,
                           c->d_flag);
    } else if (stage == 1) {
        const Fr* src = q->y[0];  // Lagrange-form key: the values (L.s)_j themselves are the scalars
        if (!lag) {
            if (q->qt.s4) {  // small circuits: both interpolations as one batch (quotient.hpp)
                e = interpolate2_on_1_to_n(tabs, qs, q->qt, q->y[0], q->y[1], q->coefA, q->coefB);
            } else {
                e = interpolate_on_1_to_n(tabs, qs, q->qt, q->y[0]);
                if (e == hipSuccess) e = hipMemcpyAsync(q->coefA, q->qt.data, sizeof(Fr) * n, hipMemcpyDeviceToDevice, qs);
            }
            src = q->coefA;
        }
        u32* a = (u32*)v.SA->st->p;
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n)), dim3(256), 0, qs, a, src, (u64)n);
        if (e == hipSuccess) e = d2d(a + 8 * (size_t)n, 0);        // r * Delta
        if (e == hipSuccess) e = d2d(a + 8 * ((size_t)n + 1), 3);  // 1 * Alpha
        if (e == hipSuccess && storage_mark_ready(v.SA->st, qs)) return fail(PS_ERR_HIP, "event record failed");
    } else if (stage == 2) {
        const Fr* src = q->y[1];
        if (!lag) {
            if (!q->qt.s4) {  // (batched with A in stage 1 otherwise)
                e = interpolate_on_1_to_n(tabs, qs, q->qt, q->y[1]);
                if (e == hipSuccess) e = hipMemcpyAsync(q->coefB, q->qt.data, sizeof(Fr) * n, hipMemcpyDeviceToDevice, qs);
            }
            src = q->coefB;
        }
        u32* b = (u32*)v.SB->st->p;
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n)), dim3(256), 0, qs, b, src, (u64)n);
        if (e == hipSuccess) e = d2d(b + 8 * (size_t)n, 1);        // s * Delta2
        if (e == hipSuccess) e = d2d(b + 8 * ((size_t)n + 1), 3);  // 1 * Beta2
        if (e == hipSuccess && storage_mark_ready(v.SB->st, qs)) return fail(PS_ERR_HIP, "event record failed");
    } else {
        // h: its n-1 coefficients (division), or with a Lagrange-form key its n-1 values on the nodes n+1..2n-1
        // (three convolutions); s*A + r*B: on coefficients or on values alike
        const Fr *hsrc = q->hbuf, *asrc = q->coefA, *bsrc = q->coefB;
        if (lag) {
            e = quotient_h_values(tabs, qs, q->qt, q->y[0], q->y[1], q->y[2]);
            hsrc = q->qt.scratch; asrc = q->y[0]; bsrc = q->y[1];
        } else {
            e = quotient_from_AB(tabs, qs, q->qt, q->coefA, q->coefB, q->hbuf);
        }
        u32* cc = (u32*)v.SC->st->p;
        if (nn && e == hipSuccess) e = hipMemcpyAsync(cc, scalars_ptr(sol) + 8 * diff, 32 * nn, hipMemcpyDeviceToDevice, qs);  // sol[i+diff]
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n - 1)), dim3(256), 0, qs, cc + 8 * nn, hsrc, (u64)(n - 1));
        if (split) {  // SC = [sol_nio | h | r] over [NioLP | XiT | Beta]; s A + r B1 is added to the sum on the host
            if (e == hipSuccess) e = d2d(cc + 8 * (nn + (size_t)n - 1), 0);  // r * Beta
        } else {
        hipLaunchKernelGGL(k_fr_lincomb_plain, dim3(nblk(n)), dim3(256), 0, qs, cc + 8 * (nn + n - 1), asrc, bsrc, sm, rm, (u64)n);
        const size_t o = nn + ((size_t)n - 1) + n;
        if (e == hipSuccess) e = d2d(cc + 8 * o, 2);        // rs * Delta
        if (e == hipSuccess) e = d2d(cc + 8 * (o + 1), 1);  // s  * Alpha
        if (e == hipSuccess) e = d2d(cc + 8 * (o + 2), 0);  // r  * Beta
        }
        if (e == hipSuccess && storage_mark_ready(v.SC->st, qs)) return fail(PS_ERR_HIP, "event record failed");
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("quotient stage: ") + hipGetErrorString(e));
    return PS_OK;
}

#ifndef PS_G16_EARLY_SUMS
#define PS_G16_EARLY_SUMS 0u  // measured, dropped: see groth16_prove_impl
#endif
// Sums a prover keeps pending.  Three, measured (round 4, 2^20 constraints, one box): 17.7 ms per Groth16 proof with three,
// 19.1 with six -- a prover's sums differ in length and group, and the G2 sum's tail must not wait behind five accumulations.
#ifndef PS_PROVER_QUEUE
#define PS_PROVER_QUEUE 3
#endif
static_assert(PS_PROVER_QUEUE <= PS_MSM_QUEUE, "the provers use the context's queue");
// ---- shared by every prover (here and in prove_shares.inc) ----
static bool ctx_busy(const ps_ctx* c) { return c->q_len > 0; }
static float ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The sums a prover has in flight on its context, oldest first, each with the kind the prover gave it and the place its result
// goes.  At most PS_PROVER_QUEUE: one more finishes the oldest (the furthest along) first.  The first error of a finish is
// kept in `err`; a prover drains the queue on every path, so that the next call on the context starts clean.
// allow_self: whether a sum may run on the context's own stream (msm_launch_impl) -- not where the quotient runs on it.
// (The provers' helper types have internal linkage: the library exports the C ABI and nothing of theirs.)
namespace {
struct SumQueue {
    struct Entry { int kind; uint8_t* dst; };
    ps_ctx* c;
    bool allow_self;
    int err = PS_OK;
    std::vector<Entry> fifo;
    int launch(int kind, const ps_points* pts, const ps_scalars* sc, uint8_t* dst) {
        while (fifo.size() + 1 > PS_PROVER_QUEUE) finish_one();
        int rc = msm_launch_impl(c, pts, sc, allow_self);
        if (!rc) fifo.push_back({kind, dst});
        return rc;
    }
    int finish_one() {  // returns the kind of the sum it finished
        const Entry e = fifo.front();
        fifo.erase(fifo.begin());
        int rc = ps_msm_finish(c, e.dst);
        if (rc && !err) err = rc;
        return e.kind;
    }
    bool empty() const { return fifo.empty(); }
    void drain_until(int kind) { while (!fifo.empty() && fifo.front().kind != kind) finish_one(); }
    void drain() { while (!fifo.empty()) finish_one(); }
};
}  // namespace

// s A + r B1' (G1): the weighting of C in the split form of groth16_prove_impl and in every rank-local share
static int g16_weight_ab1(const uint8_t* A, const uint8_t* B1, const uint8_t* r_be32, const uint8_t* s_be32, uint8_t* out) {
    uint8_t two[2 * 96], sc2[64];
    memcpy(two, A, 96); memcpy(two + 96, B1, 96);
    memcpy(sc2, s_be32, 32); memcpy(sc2 + 32, r_be32, 32);
    return ps_points_lincomb(PS_G1, two, sc2, 2, out);
}

static int groth16_prove_impl(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol, const uint8_t* r_be32,
                              const uint8_t* s_be32, int rank, int world, uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    if (!c || !pk || !q || !sol || !r_be32 || !s_be32 || !A_out || !B_out || !C_out) return fail(PS_ERR_ARG, "ps_groth16_prove: NULL argument");
    if (!pk->nio_lp || (!g16_lagrange(pk) && (!pk->xi || !pk->xi2 || !pk->xi_t))) return fail(PS_ERR_ARG, "ps_groth16_prove: NULL CRS array");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    const size_t n = q->n;
    const size_t diff = q->m - q->nio;            // groth16.go:175: "we only take variables which are _not_ io"
    const size_t nn = ps_points_len(pk->nio_lp);  // for i := range tr.NioLP, groth16.go:176
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck, qap.go:177-189
    if (diff + nn > sol->n) return fail(PS_ERR_LENGTH, "NioLP longer than the non-IO part of the solution");
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_prove: needs at least 2 gates");
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "ps_groth16_prove: an MSM is pending on this context");
    // The split form of C (Lagrange-form keys, n >= g16_b1_min_n).  C = sum NioLP + h T + s A + r B1 - rs Delta (groth16.go:180-205)
    // with B1 = Beta + sum_j b_j Xi_j + s Delta, B in G1.  One sum over [.. | Xi | ..] with the scalars s a_j + r b_j does it
    // (the form below, and the only sensible one for coefficient vectors), but with a Lagrange-form key a_j and b_j are WIRE
    // VALUES -- small or boolean in most of a real circuit, and s a_j + r b_j is full-width whatever they are.  So B1' = sum_j
    // b_j Xi_j becomes a sum of its own (over PA's Xi, with SB's scalars: no new array, no new vector), C' runs over
    // [NioLP | XiT | Beta] with [sol | h | r], and C = C' + s A + r B1' on the host (A as it leaves this function: s A
    // brings s Alpha + rs Delta along; the two scalar multiplications, ~0.5 ms, run while the GPU works on C').  The same
    // number of bucket additions when the values are uniform, fewer when they are not.  A/B on one box (tools/g16_split_ab.sh,
    // single -> split): 2^20 constraints of the tiled toy circuit (half of its right-wire values are 1) 19.2 -> 18.5 ms, 2^20
    // booleanity gates 10.0 -> 9.5 (every sum over a 2^20-point table costs ~1 ms whatever its scalars: 2^19 buckets to
    // reduce); 2^18: 7.05 -> 7.0 / 4.8 -> 5.0; 2^16: 3.4 -> 3.6 / 3.0 -> 3.6 -- a fourth sum and the host's weighting cost more than
    // they save below 2^19 constraints, hence the threshold (ps_ctx: g16_b1_min_n; PS_G16_B1_MIN_N in the environment moves it
    // for tests and measurements).
    const bool split = g16_lagrange(pk) && n >= c->g16_b1_min_n;
    int rc = groth16_prepare(c, pk, n, nn, split);
    if (rc) return rc;
    Fr rm, sm;
    if ((rc = groth16_small_scalars(c, r_be32, s_be32, &rm, &sm))) return rc;
    G16Vectors v;
    if ((rc = prover_vector(c, 0, n + 2, &v.SA)) || (rc = prover_vector(c, 1, n + 2, &v.SB)) ||
        (rc = prover_vector(c, 2, split ? nn + (n - 1) + 1 : nn + (n - 1) + n + 3, &v.SC)))
        return rc;
    // the quotient's stream: the context's high-priority one, ordered after whatever the caller left on the context stream
    hipStream_t qs = c->tail;
    if (!c->ev_q) HIP_TRY(hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_q, c->stream));
    HIP_TRY(hipStreamWaitEvent(qs, c->ev_q, 0));

    // A witness uploaded as int64 (the reference's Vector = []int) keeps its short-scalar plan: its NioLP part is
    // then a sum of its own (a quarter of the windows) over the caller's array, and C = C' + N.
    const bool split_nio = nn > 0 && sol->max_bits < 255;
    Scope scope;  // the slices the sums run over, freed at the return: every way out from here on passes sums.drain() below
    // kind: 0 = A, 1 = B, 2 = a part of C, 3 = B1' (split form); the results of a kind's pieces in the order of their launch
    SumQueue sums{c, false};
    std::vector<std::vector<uint8_t>> parts[4];
    // the share of this rank of the sum (pts, sc): its index range of every segment, and on the last rank the trailing `fixed` entries
    auto launch = [&](int kind, const ps_points* pts, const ps_scalars* sc, const std::vector<SumSegment>& segs, size_t fixed) -> int {
        for (auto& pc : share_pieces(segs, pts->n, fixed, rank, world)) {
            const ps_points* pp = pts;
            const ps_scalars* ss = sc;
            if (pc.off != 0 || pc.len != pts->n) {
                ps_points** p1 = scope.points();
                ps_scalars** s1 = scope.scalars();
                int r2 = ps_points_slice(pts, pc.off, pc.len, p1);
                if (!r2) r2 = ps_scalars_slice(sc, pc.off, pc.len, s1);
                if (r2) return r2;
                pp = *p1; ss = *s1;
            }
            std::vector<uint8_t> slot(wire_bytes(pts->group));
            parts[kind].push_back(slot);
            int r2 = sums.launch(kind, pp, ss, parts[kind].back().data());
            if (r2) { parts[kind].pop_back(); return r2; }
        }
        return PS_OK;
    };
    auto fold = [&](int kind, int group, uint8_t* out) -> int {
        if (parts[kind].empty()) { write_identity(group, out); return PS_OK; }
        if (parts[kind].size() == 1) { memcpy(out, parts[kind][0].data(), wire_bytes(group)); return PS_OK; }
        std::vector<uint8_t> flat;
        for (auto& p : parts[kind]) flat.insert(flat.end(), p.begin(), p.end());
        return ps_points_sum(group, flat.data(), parts[kind].size(), out);
    };
    ps_points **pc_rest = scope.points(), **pa_xi = scope.points();
    ps_scalars **sc_rest = scope.scalars(), **sol_nio = scope.scalars(), **sb_b = scope.scalars();
    // Small circuits: launching the sums before the host waits for the gate check (they wait on the device for their
    // scalars' ready events) was measured and is off (PS_G16_EARLY_SUMS = 0): the GPU finishes earlier (0.80 instead of
    // 1.02 ms under the profiler at 2^10 constraints) but the proof takes LONGER on the wall clock (1.2 vs 0.93 ms) -- a
    // small proof is bound by the host's ~100 us per launched sum, and enqueueing behind not-yet-complete events costs more.
    const bool early_sums = n <= PS_G16_EARLY_SUMS;
    auto launch_AB = [&]() -> int {
        int r2 = launch(1, c->g16_pb, v.SB, {{0, n}}, 2);  // B first: the longest point pass
        if (!r2) r2 = launch(0, c->g16_pa, v.SA, {{0, n}}, 2);
        if (!r2 && split) {  // B1' = sum_j b_j Xi_j: views of PA and SB
            if ((r2 = ps_points_slice(c->g16_pa, 0, n, pa_xi)) || (r2 = ps_scalars_slice(v.SB, 0, n, sb_b))) return r2;
            r2 = launch(3, *pa_xi, *sb_b, {{0, n}}, 0);
        }
        return r2;
    };
    auto launch_C = [&]() -> int {
        int r2 = PS_OK;
        if (split_nio) {
            if ((r2 = ps_scalars_slice(sol, diff, nn, sol_nio))) return r2;
            if ((r2 = launch(2, pk->nio_lp, *sol_nio, {{0, nn}}, 0))) return r2;
            // [XiT | Xi | Delta, Alpha, Beta] = PC without its NioLP head ([XiT | Beta] in the split form)
            if ((r2 = ps_points_slice(c->g16_pc, nn, c->g16_pc->n - nn, pc_rest))) return r2;
            if ((r2 = ps_scalars_slice(v.SC, nn, v.SC->n - nn, sc_rest))) return r2;
            if (split) return launch(2, *pc_rest, *sc_rest, {{0, n - 1}}, 1);
            return launch(2, *pc_rest, *sc_rest, {{0, n - 1}, {n - 1, n}}, 3);
        }
        if (split) return launch(2, c->g16_pc, v.SC, {{0, nn}, {nn, n - 1}}, 1);
        return launch(2, c->g16_pc, v.SC, {{0, nn}, {nn, n - 1}, {nn + n - 1, n}}, 3);
    };
    do {
        // the whole quotient is enqueued first (the host only enqueues: ~1 ms for ~150 launches while the GPU has started)
        for (int stage = 0; stage < 4 && !rc; stage++) rc = g16_quotient_stage(c, q, sol, qs, stage, rm, sm, diff, nn, g16_lagrange(pk), split, v);
        if (rc) break;
        // (after ALL of the quotient's launches: the host is the bottleneck here, and ~60 launches of sums ahead of the
        // quotient's last stage delay that stage by 0.4 ms)
        if (early_sums && ((rc = launch_AB()) || (rc = launch_C()))) break;
        u32 flag = 0;  // the gate check's answer
        if (hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, qs) != hipSuccess || hipStreamSynchronize(qs) != hipSuccess) {
            rc = fail(PS_ERR_HIP, "ps_groth16_prove: reading the gate check failed");
            break;
        }
        c->phase_ms[0] = ms_since(t_start);  // quotient done
        if (flag) { rc = fail(PS_ERR_NOT_DIVISIBLE, "apocalypse"); break; }  // qap.go:158-160
        if (!early_sums && ((rc = launch_AB()) || (rc = launch_C()))) break;
    } while (0);
    // split form: the sums of A, B and B1' were launched before the parts of C' and leave the queue first; their weighting
    // s A + r B1' (two scalar multiplications on the host, ~0.5 ms) runs while the GPU is still busy with C'
    uint8_t sa_rb1[96];
    bool weighted = false;
    sums.drain_until(2);
    if (split && !rc && !sums.err) {
        uint8_t a[96], b1[96];
        int r2 = fold(0, PS_G1, a);
        if (!r2) r2 = fold(3, PS_G1, b1);
        if (!r2) r2 = g16_weight_ab1(a, b1, r_be32, s_be32, sa_rb1);
        if (r2) sums.err = r2; else weighted = true;
    }
    sums.drain();
    (void)hipStreamSynchronize(qs);
    // the caller's stream continues after the quotient's
    (void)hipEventRecord(c->ev_q, qs);
    (void)hipStreamWaitEvent(c->stream, c->ev_q, 0);
    if (rc || sums.err) return rc ? rc : sums.err;
    if ((rc = fold(0, PS_G1, A_out)) || (rc = fold(1, PS_G2, B_out)) || (rc = fold(2, PS_G1, C_out))) return rc;
    if (split) {  // C = C' + (s A + r B1')
        if (!weighted) return fail(PS_ERR_ARG, "ps_groth16_prove: internal: the weighted sums are missing");
        uint8_t both[2 * 96];
        memcpy(both, C_out, 96); memcpy(both + 96, sa_rb1, 96);
        if ((rc = ps_points_sum(PS_G1, both, 2, C_out))) return rc;
    }
    c->phase_ms[1] = 0.f;
    c->phase_ms[3] = ms_since(t_start);
    c->phase_ms[2] = c->phase_ms[3] - c->phase_ms[0];
    return PS_OK;
}

extern "C" int ps_groth16_prove(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol,
                                const uint8_t* r_be32, const uint8_t* s_be32, uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    return groth16_prove_impl(c, pk, q, sol, r_be32, s_be32, 0, 1, A_out, B_out, C_out);
}

// ---------------------------------------------------------------------------------------
// Groth16Prove sharded over `world` ranks (one process per GPU): rank g takes its index range of every
// sum -- Xi of A, Xi2 of B, NioLP, Xi and XiT of C -- and the last rank also the few fixed points (they continue its ranges); each rank returns
// partial A, B, C, and the element-wise sum of all ranks' partials is the proof (playsnark_amd/dist.py gathers
// and folds them).  The quotient is computed by every rank (its NTTs do not shard without an all-to-all).
// ---------------------------------------------------------------------------------------
extern "C" int ps_groth16_prove_shard(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol,
                                      const uint8_t* r_be32, const uint8_t* s_be32, int rank, int world, uint8_t* A_part,
                                      uint8_t* B_part, uint8_t* C_part) {
    if (world < 1 || rank < 0 || rank >= world) return fail(PS_ERR_ARG, "ps_groth16_prove_shard: bad rank / world");
    return groth16_prove_impl(c, pk, q, sol, r_be32, s_be32, rank, world, A_part, B_part, C_part);
}


// ---------------------------------------------------------------------------------------
// Pieces for several GPUs (SURVEY 8e): one aggregate polynomial alone, a host-side linear combination of a few
// points, a sum over several devices from ONE process, and Groth16Prove over rank-local CRS arrays.
// ---------------------------------------------------------------------------------------
// computeAggregatePoly (qap.go:164-175) for ONE of left / right / out: the monomial coefficients of the interpolant of
// (L|R|O).s on {1..n}.  No divisibility test here (it needs all three value vectors: ps_qap_quotient does it).
extern "C" int ps_qap_interpolate(ps_ctx* c, const ps_qap* q, const ps_scalars* sol, int which, ps_scalars** out) {
    if (!c || !q || !sol || !out) return fail(PS_ERR_ARG, "ps_qap_interpolate: NULL argument");
    if (which < 0 || which > 2) return fail(PS_ERR_ARG, "ps_qap_interpolate: which must be 0 (left), 1 (right) or 2 (out)");
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const u32 n = (u32)q->n;
    if (storage_wait_ready(sol->st, st)) return fail(PS_ERR_HIP, "ps_qap_interpolate: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, st, q->sol_m, scalars_ptr(sol), (u64)q->m);
    spmv_launch(st, q->mat[which], (const Fr*)q->sol_m, q->y[which], n);
    hipError_t e = interpolate_on_1_to_n(*ctx_tabs(c), st, q->qt, q->y[which]);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("interpolation: ") + hipGetErrorString(e));
    int rc = scalars_from_mont(c, q->qt.data, n, out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return PS_OK;
}

// sum_i scalars[i] * points[i] for a HANDFUL of points, on the host (double-and-add): the fixed-point terms of a proof
// (r Delta + Alpha, ...) and the weighting of partial sums (s P_A + r P_B) when the sums themselves ran elsewhere.
template <class F>
static int points_lincomb_t(const uint8_t* pts, const uint8_t* sc_be32, size_t k, uint8_t* out, size_t wb) {
    typedef typename HostField<F>::type H;
    Xyzz<H> acc = xyzz_identity<H>();
    for (size_t i = 0; i < k; i++) {
        Affine<F> a;
        if (!read_affine(a, pts + wb * i)) return fail(PS_ERR_ENCODING, "ps_points_lincomb: bad point encoding");
        if (affine_is_identity<F>(a)) continue;
        u32 kw[8];
        scalar_from_be32_host(kw, sc_be32 + 32 * i);
        const Affine<H> h = affine_to_host<F>(a);
        xyzz_add<H>(acc, xyzz_mul_scalar<H>(xyzz_from_affine<H>(h.x, h.y), kw));
    }
    write_affine(out, acc);
    return PS_OK;
}
extern "C" int ps_points_lincomb(int group, const uint8_t* pts, const uint8_t* scalars_be32, size_t k, uint8_t* out) {
    if ((k && (!pts || !scalars_be32)) || !out) return fail(PS_ERR_ARG, "ps_points_lincomb: NULL argument");
    if (k > 64) return fail(PS_ERR_ARG, "ps_points_lincomb: at most 64 points (use ps_msm)");
    if (group == PS_G1) return points_lincomb_t<Fp>(pts, scalars_be32, k, out, 96);
    if (group == PS_G2) return points_lincomb_t<Fp2>(pts, scalars_be32, k, out, 192);
    return fail(PS_ERR_ARG, "bad group");
}

