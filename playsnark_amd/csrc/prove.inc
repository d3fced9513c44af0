// QAP quotient and whole-prover entry points of the C ABI (included by capi.hip).
//
//   ps_qap_create / ps_qap_quotient  <- ToQAP + QAP.Quotient + computeAggregatePoly (qap.go:35-175)
//   ps_groth16_prove                 <- Groth16Prove (groth16.go:122-211)
//   ps_phgr13_prove                  <- PHGR13Prove  (pinochio.go:207-254)
//   ps_poly_mul                      <- Poly.Mul     (algebra.go:92-105)

struct DevCsr {
    u32* row_ptr = nullptr;
    u32* col = nullptr;
    Fr* val = nullptr;  // Montgomery
    size_t nnz = 0;
    u32* long_rows = nullptr;  // rows with more than SPMV_LONG_ROW non-zeros
    u32 n_long = 0;
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

extern "C" int ps_qap_create(ps_ctx* c, size_t n, size_t m, size_t nio, const ps_csr* L, const ps_csr* R, const ps_csr* O,
                             ps_qap** out) {
    if (!c || !L || !R || !O || !out) return fail(PS_ERR_ARG, "ps_qap_create: NULL argument");
    if (n == 0 || m == 0 || nio > m) return fail(PS_ERR_ARG, "ps_qap_create: bad dimensions");
    if (n >= (1ull << 27)) return fail(PS_ERR_ARG, "ps_qap_create: more than 2^27 gates is not supported");
    HIP_TRY(hipSetDevice(c->device));
    ps_qap* q = new ps_qap();
    q->device = c->device;
    q->n = n; q->m = m; q->nio = nio;
    const ps_csr* src[3] = {L, R, O};
    int rc = PS_OK;
    for (int k = 0; k < 3; k++)
        if (!src[k]->row_ptr) { delete q; return fail(PS_ERR_ARG, "ps_qap_create: NULL row_ptr"); }
    // Host preparation of the three matrices and of the factorial tables on four threads: coefficient
    // conversion Value.ToFieldElement (curve.go:17-19) to Montgomery form, the transpose (counting sort
    // by column; rows = variables, for the setups' per-variable sums) and the long-row lists.
    struct HostCsr {
        bool bad_col = false;
        std::vector<Fr> vals, tv;
        std::vector<u32> tp, tc, lr, lrT;
    };
    auto prepare = [n, m](const ps_csr* s) {
        HostCsr h;
        const size_t nnz = s->row_ptr[n];
        for (size_t e = 0; e < nnz; e++)
            if (s->col[e] >= m) { h.bad_col = true; return h; }
        h.vals.resize(nnz);
        for (size_t e = 0; e < nnz; e++) {
            int64_t v = s->val[e];
            u64 mag = v < 0 ? (u64)0 - (u64)v : (u64)v;
            Fr a = fr_from_u64(mag);
            h.vals[e] = v < 0 ? fr_neg(a) : a;
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
            if (h.tp[r + 1] - h.tp[r] > SPMV_LONG_ROW) h.lrT.push_back((u32)r);
        for (size_t r = 0; r < n; r++)
            if (s->row_ptr[r + 1] - s->row_ptr[r] > SPMV_LONG_ROW) h.lr.push_back((u32)r);
        return h;
    };
    std::future<HostCsr> prep[3];
    for (int k = 0; k < 3; k++) prep[k] = std::async(std::launch::async, prepare, src[k]);
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
        const ps_csr* s = src[k];
        const size_t nnz = s->row_ptr[n];
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
        std::string keep = g_last_error;
        ps_qap_free(q);
        g_last_error = keep;
        return rc;
    }
    *out = q;
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
    Fr *ta = nullptr, *tb = nullptr, *am = nullptr, *bm = nullptr;
    HIP_TRY(hipMalloc((void**)&ta, sizeof(Fr) * S));
    HIP_TRY(hipMalloc((void**)&tb, sizeof(Fr) * S));
    HIP_TRY(hipMalloc((void**)&am, sizeof(Fr) * a->n));
    HIP_TRY(hipMalloc((void**)&bm, sizeof(Fr) * b->n));
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(a->n)), dim3(256), 0, st, am, scalars_ptr(a), (u64)a->n);
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(b->n)), dim3(256), 0, st, bm, scalars_ptr(b), (u64)b->n);
    hipError_t e = poly_mul_dev(tabs, st, am, a->n, bm, b->n, ta, nout, ta, tb);
    int rc = PS_OK;
    if (e != hipSuccess) rc = fail(PS_ERR_HIP, std::string("poly_mul: ") + hipGetErrorString(e));
    if (rc == PS_OK) rc = scalars_from_mont(c, ta, nout, out);
    (void)hipStreamSynchronize(st);
    (void)hipFree(ta); (void)hipFree(tb); (void)hipFree(am); (void)hipFree(bm);
    return rc;
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
    ps_scalars* view = nullptr;
    int rc = ps_scalars_slice(sc, first, n, &view);
    if (rc) return rc;
    rc = ps_msm(c, pts, view, out);
    ps_scalars_free(view);
    return rc;
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

static int scalars_plain_from_mont(ps_ctx* c, const Fr* src, size_t n, ps_scalars** out) { return scalars_from_mont(c, src, n, out); }

// Shared by both setups: device work buffers, z(x) and the per-variable evaluations
// u_i(x), v_i(x), w_i(x) = (M^T l(x))_i with l_j the Lagrange basis on {1..n} (qap.go:42-55).
struct SetupWork {
    hipStream_t st;
    std::vector<void*> tmp;
    Fr *pw = nullptr, *uvw[3] = {nullptr, nullptr, nullptr};
    Fr* lj = nullptr;  // l_j(x), j = 1..n: the Lagrange basis of the QAP domain at the secret point
    Fr zx;
    FrPow2Table tab;
    int alloc(Fr** p, size_t cnt) {
        hipError_t e = hipMalloc((void**)p, sizeof(Fr) * std::max<size_t>(cnt, 1));
        if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("hipMalloc setup: ") + hipGetErrorString(e));
        tmp.push_back(*p);
        return PS_OK;
    }
    void cleanup() {
        (void)hipStreamSynchronize(st);
        for (void* p : tmp) (void)hipFree(p);
        tmp.clear();
    }
};

static int setup_var_evals(ps_ctx* c, const ps_qap* q, const Fr& x, const char* who, SetupWork& wk) {
    const size_t n = q->n, m = q->m;
    hipStream_t st = wk.st = c->stream;
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
    Fr* partial = nullptr;
    HIP_TRY(hipMalloc((void**)&partial, sizeof(Fr) * std::max<unsigned>(pblocks, 1)));
    hipLaunchKernelGGL(k_prod_x_minus_j, dim3(pblocks), dim3(256), 0, st, partial, xs, (u64)cnt);
    std::vector<Fr> hp(pblocks);
    hipError_t e = hipMemcpyAsync(hp.data(), partial, sizeof(Fr) * pblocks, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(partial);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("setup: ") + hipGetErrorString(e));
    Fr zs = fr_one();
    for (auto& v : hp) zs = fr_mul(zs, v);
    hipLaunchKernelGGL(k_lagrange_at, dim3(nblk(cnt)), dim3(256), 0, st, out, (const Fr*)q->qt.invfact, xs, zs, (u64)cnt);
    HIP_TRY(hipGetLastError());
    return PS_OK;
}

// points = { src[i] * G } for a Montgomery-form device array
static int commit_mont(ps_ctx* c, int group, const Fr* src, size_t cnt, ps_points** out) {
    ps_scalars* sc = nullptr;
    int rc = scalars_plain_from_mont(c, src, cnt, &sc);
    if (rc) return rc;
    rc = ps_points_from_scalars(c, group, sc, out);
    ps_scalars_free(sc);
    return rc;
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
    SetupWork wk;
    Fr* lin = nullptr;
    int rc = setup_var_evals(c, q, x, "ps_groth16_setup", wk);
    if (!rc) rc = wk.alloc(&lin, m);
    if (rc) { wk.cleanup(); return rc; }
    Fr* pw = wk.pw;
    hipLaunchKernelGGL(k_linear_poly, dim3(nblk(m)), dim3(256), 0, st, lin, (const Fr*)wk.uvw[0], (const Fr*)wk.uvw[1],
                       (const Fr*)wk.uvw[2], alpha, beta, ginv, dinv, (u64)diff, (u64)m);
    do {
        // Xi, Xi2 = {x^i G}, i < n            (groth16.go:79-80)
        hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n)), dim3(256), 0, st, pw, wk.tab, fr_one(), (u64)n);
        if ((rc = commit_mont(c, PS_G1, pw, n, &out->xi))) break;
        if ((rc = commit_mont(c, PS_G2, pw, n, &out->xi2))) break;
        // XiT = {x^i t(x)/delta G}, i < n-1   (groth16.go:94-97)
        hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n - 1)), dim3(256), 0, st, pw, wk.tab, fr_mul(wk.zx, dinv), (u64)(n - 1));
        if ((rc = commit_mont(c, PS_G1, pw, n - 1, &out->xi_t))) break;
        // IoLP / NioLP                         (groth16.go:86-91)
        if ((rc = commit_mont(c, PS_G1, lin, diff, &out->io_lp))) break;
        if ((rc = commit_mont(c, PS_G1, lin + diff, m - diff, &out->nio_lp))) break;
        // the same CRS in Lagrange form (see ps_groth16_pk): l_j(x) G1, l_j(x) G2, lambda_k(x) t(x)/delta G1
        if ((rc = commit_mont(c, PS_G1, wk.lj, n, &out->lxi))) break;
        if ((rc = commit_mont(c, PS_G2, wk.lj, n, &out->lxi2))) break;
        if ((rc = setup_shifted_lagrange(c, q, x, pw))) break;
        hipLaunchKernelGGL(k_fr_scale, dim3(nblk(n - 1)), dim3(256), 0, st, pw, (const Fr*)pw, fr_mul(wk.zx, dinv), (u64)(n - 1));
        if ((rc = commit_mont(c, PS_G1, pw, n - 1, &out->lxi_t))) break;
    } while (0);
    wk.cleanup();
    if (rc) {
        ps_points_free(out->lxi); ps_points_free(out->lxi2); ps_points_free(out->lxi_t);
        ps_points_free(out->xi); ps_points_free(out->xi2); ps_points_free(out->xi_t); ps_points_free(out->io_lp); ps_points_free(out->nio_lp);
        memset(out, 0, sizeof *out);
        return rc;
    }
    host_fixed_base<Fp>(out->alpha, tw->alpha);   // groth16.go:67-76
    host_fixed_base<Fp>(out->beta, tw->beta);
    host_fixed_base<Fp2>(out->beta2, tw->beta);
    host_fixed_base<Fp>(out->delta, tw->delta);
    host_fixed_base<Fp2>(out->delta2, tw->delta);
    host_fixed_base<Fp2>(out->gamma, tw->gamma);
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
    SetupWork wk;
    int rc = setup_var_evals(c, q, s, "ps_phgr13_setup", wk);
    if (rc) { wk.cleanup(); return rc; }
    auto scaled = [&](int group, const Fr* src, size_t first, size_t cnt, const Fr& scale, ps_points** dst) -> int {
        if (cnt) hipLaunchKernelGGL(k_fr_scale, dim3(nblk(cnt)), dim3(256), 0, st, wk.pw, src + first, scale, (u64)cnt);
        return commit_mont(c, group, wk.pw, cnt, dst);
    };
    do {
        // gsi = {s^i G}, i = 0..n-2                                         (pinochio.go:101)
        hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n - 1)), dim3(256), 0, st, wk.pw, wk.tab, fr_one(), (u64)(n - 1));
        if ((rc = commit_mont(c, PS_G1, wk.pw, n - 1, &out->gsi))) break;
        // ... and in Lagrange form on the nodes n+1..2n-1 (see ps_phgr13_ek.lgsi)
        if ((rc = setup_shifted_lagrange(c, q, s, wk.pw))) break;
        if ((rc = commit_mont(c, PS_G1, wk.pw, n - 1, &out->lgsi))) break;
        // g_v^(v_k(s)), g_w^(w_k(s)), g_y^(y_k(s)) for all k                 (:158-160)
        if ((rc = scaled(PS_G1, wk.uvw[0], 0, m, rv, &out->vk_vs))) break;
        if ((rc = scaled(PS_G2, wk.uvw[1], 0, m, rw, &out->vk_ws))) break;
        if ((rc = scaled(PS_G1, wk.uvw[2], 0, m, ry, &out->vk_ys))) break;
        // the prover's non-IO part                                           (:123-125)
        if ((rc = ps_points_slice(out->vk_vs, diff, nn, &out->vs))) break;
        if ((rc = ps_points_slice(out->vk_ws, diff, nn, &out->ws))) break;
        if ((rc = ps_points_slice(out->vk_ys, diff, nn, &out->ys))) break;
        // shifted by alpha                                                   (:127-129; was uses g1w = rw*G1)
        if ((rc = scaled(PS_G1, wk.uvw[0], diff, nn, fr_mul(rv, av), &out->vas))) break;
        if ((rc = scaled(PS_G1, wk.uvw[1], diff, nn, fr_mul(rw, aw), &out->was))) break;
        if ((rc = scaled(PS_G1, wk.uvw[2], diff, nn, fr_mul(ry, ay), &out->yas))) break;
        // shifted by beta                                                    (:135-137)
        if ((rc = scaled(PS_G1, wk.uvw[0], diff, nn, fr_mul(rv, beta), &out->vbs))) break;
        if ((rc = scaled(PS_G1, wk.uvw[1], diff, nn, fr_mul(rw, beta), &out->wbs))) break;
        if ((rc = scaled(PS_G1, wk.uvw[2], diff, nn, fr_mul(ry, beta), &out->ybs))) break;
    } while (0);
    wk.cleanup();
    if (rc) {
        ps_phgr13_crs_free(out);
        memset(out, 0, sizeof *out);
        return rc;
    }
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
    ps_points *fa = nullptr, *fb = nullptr, *fc = nullptr;
    int rc;
    for (const ps_points* arr : {xi, xi2, pk->nio_lp, xi_t})
        if (storage_wait_ready(arr->st, c->stream)) return fail(PS_ERR_HIP, "ps_groth16_prove: event wait failed");
    if ((rc = upload_fixed_points<Fp>(c, PS_G1, {pk->delta, pk->alpha}, &fa))) return rc;
    if ((rc = upload_fixed_points<Fp2>(c, PS_G2, {pk->delta2, pk->beta2}, &fb))) { ps_points_free(fa); return rc; }
    if (split) rc = upload_fixed_points<Fp>(c, PS_G1, {pk->beta}, &fc);
    else rc = upload_fixed_points<Fp>(c, PS_G1, {pk->delta, pk->alpha, pk->beta}, &fc);
    if (rc) { ps_points_free(fa); ps_points_free(fb); return rc; }
    rc = points_concat(c, PS_G1, {{points_ptr(xi), n}, {points_ptr(fa), 2}}, &c->g16_pa);
    if (!rc) rc = points_concat(c, PS_G2, {{points_ptr(xi2), n}, {points_ptr(fb), 2}}, &c->g16_pb);
    // split form of C (groth16_prove_impl): PC = [NioLP | XiT | Beta], no third copy of Xi
    if (!rc && split) rc = points_concat(c, PS_G1, {{points_ptr(pk->nio_lp), nn}, {points_ptr(xi_t), n - 1}, {points_ptr(fc), 1}}, &c->g16_pc);
    else if (!rc) rc = points_concat(c, PS_G1, {{points_ptr(pk->nio_lp), nn}, {points_ptr(xi_t), n - 1}, {points_ptr(xi), n}, {points_ptr(fc), 3}},
                                     &c->g16_pc);
    (void)hipStreamSynchronize(c->stream);
    ps_points_free(fa); ps_points_free(fb); ps_points_free(fc);
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
// The quotient runs first, alone, on the context's high-priority stream; the sums follow on the worker contexts.
// Running them beside each other was measured and dropped (n = 2^20): sums that need no polynomial started at once made
// the quotient 2.4 x slower (11.9 -> 29 ms) for the same total -- the NTT passes are VALU-bound by instructions, the
// bucket accumulations by multiplications, so neither has idle issue slots to lend -- and even the digit sorts alone
// (LDS / memory-bound, but 140 KB of LDS per workgroup) cost the quotient 2.7 ms for 0.7 ms of sorting hidden.
struct G16Vectors { ps_scalars *SA = nullptr, *SB = nullptr, *SC = nullptr; };
static void g16_free(G16Vectors& v) { v = G16Vectors(); }  // (the vectors are the context's: prover_vector, capi.hip)

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
struct G16Plan {  // which index ranges a caller sums: the whole arrays (rank 0 of 1), or one rank's shares
    int rank = 0, world = 1;
};
struct SumSegment { size_t off, len; };

static void shard_range_c(size_t len, int rank, int world, size_t* first, size_t* cnt) {
    const size_t base = len / (size_t)world, extra = len % (size_t)world;
    *first = (size_t)rank * base + std::min<size_t>((size_t)rank, extra);
    *cnt = base + ((size_t)rank < extra ? 1 : 0);
}

static int groth16_prove_impl(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol, const uint8_t* r_be32,
                              const uint8_t* s_be32, const G16Plan& gp, uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    if (!c || !pk || !q || !sol || !r_be32 || !s_be32 || !A_out || !B_out || !C_out) return fail(PS_ERR_ARG, "ps_groth16_prove: NULL argument");
    if (!pk->nio_lp || (!g16_lagrange(pk) && (!pk->xi || !pk->xi2 || !pk->xi_t))) return fail(PS_ERR_ARG, "ps_groth16_prove: NULL CRS array");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const size_t n = q->n;
    const size_t diff = q->m - q->nio;            // groth16.go:175: "we only take variables which are _not_ io"
    const size_t nn = ps_points_len(pk->nio_lp);  // for i := range tr.NioLP, groth16.go:176
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck, qap.go:177-189
    if (diff + nn > sol->n) return fail(PS_ERR_LENGTH, "NioLP longer than the non-IO part of the solution");
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_prove: needs at least 2 gates");
    if (c->pending || (c->aux && c->aux->pending)) return fail(PS_ERR_ARG, "ps_groth16_prove: an MSM is pending on this context");
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
        (rc = prover_vector(c, 2, split ? nn + (n - 1) + 1 : nn + (n - 1) + n + 3, &v.SC))) {
        g16_free(v);
        return rc;
    }
    // the quotient's stream: the context's high-priority one, ordered after whatever the caller left on the context stream
    hipStream_t qs = c->tail;
    if (!c->ev_q) HIP_TRY(hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_q, c->stream));
    HIP_TRY(hipStreamWaitEvent(qs, c->ev_q, 0));

    // A witness uploaded as int64 (the reference's Vector = []int) keeps its short-scalar plan: its NioLP part is
    // then a sum of its own (a quarter of the windows) over the caller's array, and C = C' + N.
    const bool split_nio = nn > 0 && sol->max_bits < 255;
    std::vector<ps_points*> pv;  // slices, freed at the end
    std::vector<ps_scalars*> sv;
    struct Pending { int kind; int group; };  // kind: 0 = A, 1 = B, 2 = a part of C, 3 = B1' (split form)
    std::vector<Pending> fifo;
    std::vector<std::vector<uint8_t>> parts[4];
    int rcb = PS_OK;
    auto finish_one = [&]() {
        const Pending pe = fifo.front();
        fifo.erase(fifo.begin());
        std::vector<uint8_t> out(wire_bytes(pe.group));
        int r2 = ps_msm_finish(c, out.data());
        if (r2 && !rcb) rcb = r2;
        parts[pe.kind].push_back(out);
    };
    // the share of this rank of the sum (pts, sc): its index range of every segment, and on the last rank the trailing `fixed` entries
    auto launch = [&](int kind, const ps_points* pts, const ps_scalars* sc, const std::vector<SumSegment>& segs, size_t fixed) -> int {
        std::vector<SumSegment> pieces;
        if (gp.world == 1) {
            pieces.push_back({0, pts->n});
        } else {
            for (auto& sg : segs) {
                size_t f, cnt;
                shard_range_c(sg.len, gp.rank, gp.world, &f, &cnt);
                if (cnt) pieces.push_back({sg.off + f, cnt});
            }
            // The few fixed points behind the last segment go to the LAST rank: there they continue its range of that segment,
            // so they ride in that sum instead of being two or three sums of their own (a 3-point sum is all latency:
            // rank 0's share of a 2^20-constraint proof took 7.8 ms where the others took 6.5, tools/g16_shares.py).
            if (gp.rank == gp.world - 1 && fixed) {
                if (!pieces.empty() && pieces.back().off + pieces.back().len == pts->n - fixed) pieces.back().len += fixed;
                else pieces.push_back({pts->n - fixed, fixed});
            }
        }
        for (auto& pc : pieces) {
            while (fifo.size() + 1 > PS_PROVER_QUEUE) finish_one();  // the oldest sum is the furthest along
            const ps_points* pp = pts;
            const ps_scalars* ss = sc;
            if (pc.off != 0 || pc.len != pts->n) {
                ps_points* p1 = nullptr;
                ps_scalars* s1 = nullptr;
                int r2 = ps_points_slice(pts, pc.off, pc.len, &p1);
                if (!r2) r2 = ps_scalars_slice(sc, pc.off, pc.len, &s1);
                if (r2) { ps_points_free(p1); ps_scalars_free(s1); return r2; }
                pv.push_back(p1); sv.push_back(s1);
                pp = p1; ss = s1;
            }
            int r2 = msm_launch_impl(c, pp, ss, false);
            if (r2) return r2;
            fifo.push_back({kind, pts->group});
        }
        return PS_OK;
    };
    ps_points *pc_rest = nullptr, *pa_xi = nullptr;
    ps_scalars *sc_rest = nullptr, *sol_nio = nullptr, *sb_b = nullptr;
    // Small circuits: launching the sums before the host waits for the gate check (they wait on the device for their
    // scalars' ready events) was measured and is off (PS_G16_EARLY_SUMS = 0): the GPU finishes earlier (0.80 instead of
    // 1.02 ms under the profiler at 2^10 constraints) but the proof takes LONGER on the wall clock (1.2 vs 0.93 ms) -- a
    // small proof is bound by the host's ~100 us per launched sum, and enqueueing behind not-yet-complete events costs more.
    const bool early_sums = n <= PS_G16_EARLY_SUMS;
    auto launch_AB = [&]() -> int {
        int r2 = launch(1, c->g16_pb, v.SB, {{0, n}}, 2);  // B first: the longest point pass
        if (!r2) r2 = launch(0, c->g16_pa, v.SA, {{0, n}}, 2);
        if (!r2 && split) {  // B1' = sum_j b_j Xi_j: views of PA and SB
            if ((r2 = ps_points_slice(c->g16_pa, 0, n, &pa_xi)) || (r2 = ps_scalars_slice(v.SB, 0, n, &sb_b))) return r2;
            r2 = launch(3, pa_xi, sb_b, {{0, n}}, 0);
        }
        return r2;
    };
    auto launch_C = [&]() -> int {
        int r2 = PS_OK;
        if (split_nio) {
            if ((r2 = ps_scalars_slice(sol, diff, nn, &sol_nio))) return r2;
            if ((r2 = launch(2, pk->nio_lp, sol_nio, {{0, nn}}, 0))) return r2;
            // [XiT | Xi | Delta, Alpha, Beta] = PC without its NioLP head ([XiT | Beta] in the split form)
            if ((r2 = ps_points_slice(c->g16_pc, nn, c->g16_pc->n - nn, &pc_rest))) return r2;
            if ((r2 = ps_scalars_slice(v.SC, nn, v.SC->n - nn, &sc_rest))) return r2;
            if (split) return launch(2, pc_rest, sc_rest, {{0, n - 1}}, 1);
            return launch(2, pc_rest, sc_rest, {{0, n - 1}, {n - 1, n}}, 3);
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
    while (!fifo.empty() && fifo.front().kind != 2) finish_one();
    if (split && !rc && !rcb) {
        uint8_t two[2 * 96], sc2[64];
        auto fold_g1 = [&](int kind, uint8_t* out) -> int {
            if (parts[kind].empty()) { write_identity(PS_G1, out); return PS_OK; }
            std::vector<uint8_t> flat;
            for (auto& p : parts[kind]) flat.insert(flat.end(), p.begin(), p.end());
            return ps_points_sum(PS_G1, flat.data(), parts[kind].size(), out);
        };
        memcpy(sc2, s_be32, 32); memcpy(sc2 + 32, r_be32, 32);
        int r2 = fold_g1(0, two);
        if (!r2) r2 = fold_g1(3, two + 96);
        if (!r2) r2 = ps_points_lincomb(PS_G1, two, sc2, 2, sa_rb1);
        if (r2) rcb = r2; else weighted = true;
    }
    while (!fifo.empty()) finish_one();
    (void)hipStreamSynchronize(qs);
    // the caller's stream continues after the quotient's
    (void)hipEventRecord(c->ev_q, qs);
    (void)hipStreamWaitEvent(c->stream, c->ev_q, 0);
    for (auto* p : pv) ps_points_free(p);
    for (auto* p2 : sv) ps_scalars_free(p2);
    ps_points_free(pc_rest); ps_scalars_free(sc_rest); ps_scalars_free(sol_nio);
    ps_points_free(pa_xi); ps_scalars_free(sb_b);
    g16_free(v);
    if (rc || rcb) return rc ? rc : rcb;
    auto fold = [&](int kind, int group, uint8_t* out) -> int {
        if (parts[kind].empty()) { write_identity(group, out); return PS_OK; }
        if (parts[kind].size() == 1) { memcpy(out, parts[kind][0].data(), wire_bytes(group)); return PS_OK; }
        std::vector<uint8_t> flat;
        for (auto& p : parts[kind]) flat.insert(flat.end(), p.begin(), p.end());
        return ps_points_sum(group, flat.data(), parts[kind].size(), out);
    };
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
    return groth16_prove_impl(c, pk, q, sol, r_be32, s_be32, G16Plan{}, A_out, B_out, C_out);
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
    G16Plan gp;
    gp.rank = rank;
    gp.world = world;
    return groth16_prove_impl(c, pk, q, sol, r_be32, s_be32, gp, A_part, B_part, C_part);
}

// PHGR13Prove (pinochio.go:207-254).  The nine computeSolCommit sums (:231-241) share one scalar
// vector, solution[diff:], so they share one digit sort (ps_msm_multi); and since
// gz = sum_k s_k vbs_k + sum_k s_k wbs_k + sum_k s_k ybs_k = sum_k s_k (vbs_k + wbs_k + ybs_k), the three
// beta arrays are summed pointwise once per evaluation key and gz is ONE sum.  Same group elements,
// hence the same canonical bytes, as the reference's statement-by-statement computation.
static int phgr13_beta_sum(ps_ctx* c, const ps_phgr13_ek* ek) {
    const unsigned long long key[3] = {ek->vbs->uid, ek->wbs->uid, ek->ybs->uid};
    if (c->phgr_bsum && !memcmp(key, c->phgr_key, sizeof key)) return PS_OK;
    if (c->phgr_bsum) { ps_points_free(c->phgr_bsum); c->phgr_bsum = nullptr; }
    const size_t n = ek->vbs->n;
    int rc = points_alloc(c, PS_G1, n, &c->phgr_bsum);
    if (rc) return rc;
    for (const ps_points* arr : {ek->vbs, ek->wbs, ek->ybs})
        if (storage_wait_ready(arr->st, c->stream)) return fail(PS_ERR_HIP, "ps_phgr13_prove: event wait failed");
    if (n)
        hipLaunchKernelGGL(k_points_add3<Fp>, dim3(nblocks(n)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(ek->vbs),
                           (const Affine<Fp>*)points_ptr(ek->wbs), (const Affine<Fp>*)points_ptr(ek->ybs), (u32)n,
                           (Affine<Fp>*)c->phgr_bsum->st->p);
    HIP_TRY(hipGetLastError());
    memcpy(c->phgr_key, key, sizeof key);
    return PS_OK;
}

extern "C" int ps_phgr13_prove(ps_ctx* c, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sol, ps_phgr13_proof* out) {
    if (!c || !ek || !q || !sol || !out) return fail(PS_ERR_ARG, "ps_phgr13_prove: NULL argument");
    const ps_points* arrs[10] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, ek->gsi, ek->vbs, ek->wbs, ek->ybs};
    for (auto* p : arrs)
        if (!p) return fail(PS_ERR_ARG, "ps_phgr13_prove: NULL evaluation-key array");
    for (auto* p : arrs)
        if (p->group != (p == ek->ws ? PS_G2 : PS_G1)) return fail(PS_ERR_ARG, "ps_phgr13_prove: evaluation-key array in the wrong group");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    const size_t diff = q->m - q->nio;  // pinochio.go:219
    // computeSolCommit: acc += solution[diff+i] * evalCommit[i]  (pinochio.go:222-229)
    const size_t nn = ek->vs->n;
    bool same_len = true;
    for (auto* p : arrs)
        if (p != ek->gsi) {
            if (diff + p->n > sol->n) return fail(PS_ERR_LENGTH, "evaluation-key array longer than the non-IO part of the solution");
            same_len = same_len && p->n == nn;
        }
    int rc;
    // Order of work (measured at n = 2^20, see the Groth16 driver above): the quotient first and alone -- its NTT passes
    // and the bucket accumulations are both VALU-bound, sharing the chip only stretches the quotient --, then the h(s)
    // sum on the context itself and the seven solution sums (one digit sort) on two worker contexts, every point pass
    // chained behind the previous one.
    //                          :231     :232 (G2) :233     :234      :235      :236      :239-242
    const ps_points* pts[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, nullptr};
    uint8_t* dst[7] = {out->vss, out->wss, out->yss, out->vass, out->wass, out->yass, out->gz};
    ps_scalars* view = nullptr;
    MsmPlan mpl{};
    ps_ctx* ring[PS_MULTI_RING] = {nullptr, nullptr, nullptr, nullptr};
    const bool multi = same_len && nn > 0;
    if (multi) {
        if ((rc = phgr13_beta_sum(c, ek))) return rc;
        pts[6] = c->phgr_bsum;
        if (tables_wanted(c, nn)) {  // evaluation-key arrays are fixed across proofs: their window tables are built once
            for (int i = 0; i < 7 && !rc; i++)
                rc = points_ensure_table(c, pts[i], 0, true);  // shared keys: built once, under the array's lock; no room: plain plan
            if (!rc && !ek->lgsi && ek->gsi->n >= PS_TABLE_MIN_POINTS) rc = points_ensure_table(c, ek->gsi, 0, true);
            if (rc) return rc;
        }
        if ((rc = msm_multi_ring(c, false, 7, ring))) return rc;
        if (c->pending || c->aux->pending) return fail(PS_ERR_ARG, "ps_phgr13_prove: an MSM is pending on this context");
    }
    // h as coefficients over gsi (pinochio.go:209-218), or -- with the Lagrange form of gsi in the key -- as its values on
    // the nodes n+1..2n-1 over lgsi: the same group element without the interpolation
    const ps_points* gsi = ek->gsi;
    if (q->n >= 1 && (ek->gsi->n != q->n - 1 || (ek->lgsi && ek->lgsi->n != q->n - 1)))  // hx.BlindEval(zeroG1, ek.gsi) panics, algebra.go:350-352
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(q->n - 1) + " and blinded eval points " +
                                       std::to_string(ek->gsi->n != q->n - 1 ? ek->gsi->n : ek->lgsi->n));
    if (ek->lgsi) {
        if (ek->lgsi->group != PS_G1) return fail(PS_ERR_ARG, "ps_phgr13_prove: evaluation-key array in the wrong group");
        gsi = ek->lgsi;
        if (multi && tables_wanted(c, nn) && gsi->n >= PS_TABLE_MIN_POINTS && (rc = points_ensure_table(c, gsi, 0, true))) return rc;
    }
    rc = quotient_run(c, q, sol, ek->lgsi ? Q_H_VALUES : Q_H_ONLY);
    if (rc) return rc;
    ps_scalars* h = nullptr;  // (the context's own vector, slot 3: not freed here)
    if ((rc = prover_vector(c, 3, q->n - 1, &h))) return rc;
    if (q->n > 1)
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(q->n - 1)), dim3(256), 0, c->stream, (u32*)h->st->p, (const Fr*)(ek->lgsi ? q->qt.scratch : q->hbuf),
                           (u64)(q->n - 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->phase_ms[0] = ms_since(t_start);
    const auto t_h = std::chrono::steady_clock::now();
    if (multi) {
        // The digit sort of the seven solution sums first (on a worker stream; no fork event: nothing it reads is still
        // being produced), then the h(s) sum -- ghs := hx.BlindEval(zeroG1, ek.gsi), pinochio.go:218 -- on the context's
        // own stream, then the seven point passes chained behind its accumulation: a sort that has to share the chip with
        // an accumulation waits for CUs (140 KB of LDS per workgroup) and was measured at 1.9 ms instead of 0.1.
        bool h_launched = false;
        rc = ps_scalars_slice(sol, diff, nn, &view);
        if (!rc) rc = msm_plan_checked(c, pts, 7, nn, view->max_bits, &mpl);
        if (!rc) rc = msm_multi_sort(c, ring, view, mpl, false);
        if (!rc && !(rc = msm_launch_impl(c, gsi, h, true))) h_launched = true;
        if (!rc) {
            hipEvent_t after_h = (h->n && c->last_chain) ? c->last_chain->ev_acc_local : nullptr;
            rc = msm_multi_points(c, ring, pts, 7, view, mpl, after_h);
        }
        if (rc && h_launched) { uint8_t dump[96]; (void)ps_msm_finish(c, dump); }
        if (!rc) {
            rc = ps_msm_finish(c, out->hs);
            c->phase_ms[1] = ms_since(t_h);
            const auto t_sums = std::chrono::steady_clock::now();
            int r2 = msm_multi_finish(c, ring[0], pts, 7, mpl, rc ? nullptr : dst);
            if (!rc) rc = r2;
            c->phase_ms[2] = ms_since(t_sums);
        }
        ps_scalars_free(view);
        c->phase_ms[3] = ms_since(t_start);
        return rc;
    }
    rc = ps_msm(c, gsi, h, out->hs);  // ghs := hx.BlindEval(zeroG1, ek.gsi), pinochio.go:218
    c->phase_ms[1] = ms_since(t_h);
    if (rc) return rc;
    if (same_len) {  // nn == 0: every sum is empty
        for (int i = 0; i < 7; i++) write_identity(i == 1 ? PS_G2 : PS_G1, dst[i]);
        return PS_OK;
    }
    // arrays of different lengths (not what NewPHGR13TrustedSetup produces): one sum at a time
    auto sol_commit = [&](const ps_points* ec, uint8_t* dst) -> int { return msm_range(c, ec, sol, diff, ec->n, dst); };
    uint8_t vb[96], wb[96], yb[96];
    if ((rc = sol_commit(ek->vs, out->vss))) return rc;    // :231
    if ((rc = sol_commit(ek->ws, out->wss))) return rc;    // :232 (G2)
    if ((rc = sol_commit(ek->ys, out->yss))) return rc;    // :233
    if ((rc = sol_commit(ek->vas, out->vass))) return rc;  // :234
    if ((rc = sol_commit(ek->was, out->wass))) return rc;  // :235
    if ((rc = sol_commit(ek->yas, out->yass))) return rc;  // :236
    if ((rc = sol_commit(ek->vbs, vb))) return rc;         // :239
    if ((rc = sol_commit(ek->wbs, wb))) return rc;         // :240
    if ((rc = sol_commit(ek->ybs, yb))) return rc;         // :241
    // gz := gvb + (gwb + gyb)                                pinochio.go:242
    uint8_t three[3 * 96];
    memcpy(three, vb, 96); memcpy(three + 96, wb, 96); memcpy(three + 192, yb, 96);
    return ps_points_sum(PS_G1, three, 3, out->gz);
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

// One sum over index-range shards that live on several devices of this process: shard d is summed on ctxs[d]
// (asynchronously: the devices work side by side), the partial sums are folded on the host.
extern "C" int ps_msm_multi_device(ps_ctx* const* ctxs, const ps_points* const* pts, const ps_scalars* const* sc, size_t ndev,
                                   uint8_t* out) {
    if (!ctxs || !pts || !sc || !out || ndev == 0) return fail(PS_ERR_ARG, "ps_msm_multi_device: NULL argument");
    if (ndev > 64) return fail(PS_ERR_ARG, "ps_msm_multi_device: at most 64 devices");
    const int group = pts[0] ? pts[0]->group : 0;
    for (size_t d = 0; d < ndev; d++)
        if (!ctxs[d] || !pts[d] || !sc[d] || pts[d]->group != group) return fail(PS_ERR_ARG, "ps_msm_multi_device: NULL or mixed-group shard");
    const size_t wb = wire_bytes(group);
    std::vector<uint8_t> partial(wb * ndev);
    size_t launched = 0;
    int rc = PS_OK;
    for (; launched < ndev && !rc; launched++) rc = ps_msm_launch(ctxs[launched], pts[launched], sc[launched]);
    if (rc) launched--;
    for (size_t d = 0; d < launched; d++) {
        int r2 = ps_msm_finish(ctxs[d], partial.data() + wb * d);
        if (r2 && !rc) rc = r2;
    }
    if (rc) return rc;
    return ps_points_sum(group, partial.data(), ndev, out);
}

// Groth16Prove (groth16.go:122-211) over `ndev` devices of this process, every device holding only ITS index range of
// the CRS arrays (shard_range: contiguous, sizes differ by at most one; the fixed points are read from device 0's key).
// The three parts of the quotient are independent until the exchange: with three or more devices A, B and h (h-only
// route, which also carries the divisibility test) are computed side by side on devices 0, 1, 2; the coefficient vectors
// cross through host memory, each device takes its ranges, and the partial proofs are folded on the host.  A Go caller
// cannot start one process per GPU around a function call; this is its multi-GPU entry.
// That is the route of MONOMIAL local keys.  When every device's pk carries lxi / lxi2 / lxi_t the call goes to
// groth16_prove_multi_lagrange (end of this file): no coefficient vectors, nothing through host memory.
// The fixed points of a proof, added on the host to ONE share (the sums themselves ran elsewhere):
//   A += r Delta + Alpha ;  B += s Delta2 + Beta2 ;  C += rs Delta + s Alpha + r Beta   (expanded from groth16.go:149-200)
static int g16_add_fixed_points(const ps_groth16_pk& pk, const uint8_t* r_be32, const uint8_t* s_be32, uint8_t* A, uint8_t* B, uint8_t* C) {
    Fr rm = fr_mont_from_be32(r_be32), sm = fr_mont_from_be32(s_be32);
    uint8_t one[32] = {0}, rs[32];
    one[31] = 1;
    fr_mont_to_be32(rs, fr_mul(rm, sm));
    uint8_t pts3[3 * 96], sc3[96], fx[96], fx2[192], pts2[2 * 192], acc2[2 * 192];
    memcpy(pts3, pk.delta, 96); memcpy(pts3 + 96, pk.alpha, 96);
    memcpy(sc3, r_be32, 32); memcpy(sc3 + 32, one, 32);
    int rc = ps_points_lincomb(PS_G1, pts3, sc3, 2, fx);
    memcpy(pts3, A, 96); memcpy(pts3 + 96, fx, 96);
    if (!rc) rc = ps_points_sum(PS_G1, pts3, 2, A);
    memcpy(pts2, pk.delta2, 192); memcpy(pts2 + 192, pk.beta2, 192);
    memcpy(sc3, s_be32, 32); memcpy(sc3 + 32, one, 32);
    if (!rc) rc = ps_points_lincomb(PS_G2, pts2, sc3, 2, fx2);
    memcpy(acc2, B, 192); memcpy(acc2 + 192, fx2, 192);
    if (!rc) rc = ps_points_sum(PS_G2, acc2, 2, B);
    memcpy(pts3, pk.delta, 96); memcpy(pts3 + 96, pk.alpha, 96); memcpy(pts3 + 192, pk.beta, 96);
    memcpy(sc3, rs, 32); memcpy(sc3 + 32, s_be32, 32); memcpy(sc3 + 64, r_be32, 32);
    if (!rc) rc = ps_points_lincomb(PS_G1, pts3, sc3, 3, fx);
    memcpy(pts3, C, 96); memcpy(pts3 + 96, fx, 96);
    if (!rc) rc = ps_points_sum(PS_G1, pts3, 2, C);
    return rc;
}
// every device's pk carries lxi / lxi2 / lxi_t: the route without coefficient vectors (at the end of this file)
static int groth16_prove_multi_lagrange(const ps_groth16_device* dev, size_t ndev, size_t nn, const uint8_t* r_be32, const uint8_t* s_be32,
                                        uint8_t* A_out, uint8_t* B_out, uint8_t* C_out);
static int g16_download_all(ps_ctx* c, const ps_scalars* s, std::vector<uint8_t>& host) {
    host.resize(32 * s->n);
    return ps_scalars_download(c, s, 0, s->n, host.data());
}
extern "C" int ps_groth16_prove_multi(const ps_groth16_device* dev, size_t ndev, const uint8_t* r_be32, const uint8_t* s_be32,
                                      uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    if (!dev || ndev == 0 || !r_be32 || !s_be32 || !A_out || !B_out || !C_out) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: NULL argument");
    if (ndev > 64) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: at most 64 devices");
    for (size_t d = 0; d < ndev; d++)
        if (!dev[d].ctx || !dev[d].qap || !dev[d].sol || !dev[d].pk.nio_lp) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: NULL handle");
    // Lagrange-form local keys (lxi, lxi2, lxi_t on EVERY device; the monomial arrays may then be NULL, as in ps_groth16_prove)
    // take the route without coefficient vectors; monomial keys take the route below, as before
    const bool lag = g16_lagrange(&dev[0].pk);
    for (size_t d = 0; d < ndev; d++) {
        if (g16_lagrange(&dev[d].pk) != lag)
            return fail(PS_ERR_ARG, "ps_groth16_prove_multi: lxi / lxi2 / lxi_t must be on every device or on none");
        if (!lag && (!dev[d].pk.xi || !dev[d].pk.xi2 || !dev[d].pk.xi_t)) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: NULL handle");
    }
    const size_t n = dev[0].qap->n, m = dev[0].qap->m, diff = m - dev[0].qap->nio;
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: needs at least 2 gates");
    size_t nn = 0;
    for (size_t d = 0; d < ndev; d++) nn += dev[d].pk.nio_lp->n;
    if (diff + nn > m) return fail(PS_ERR_LENGTH, "NioLP longer than the non-IO part of the solution");
    for (size_t d = 0; d < ndev; d++) {  // every local array must be exactly this device's range (algebra.go:350-352 otherwise)
        size_t f, cnt;
        const ps_groth16_pk& pk = dev[d].pk;
        shard_range_c(n, (int)d, (int)ndev, &f, &cnt);
        const ps_points *xi = lag ? pk.lxi : pk.xi, *xi2 = lag ? pk.lxi2 : pk.xi2, *xi_t = lag ? pk.lxi_t : pk.xi_t;
        bool ok = xi->n == cnt && xi2->n == cnt;
        shard_range_c(n - 1, (int)d, (int)ndev, &f, &cnt);
        ok = ok && xi_t->n == cnt;
        shard_range_c(nn, (int)d, (int)ndev, &f, &cnt);
        ok = ok && pk.nio_lp->n == cnt;
        if (!ok || dev[d].qap->n != n || dev[d].qap->m != m || dev[d].sol->n != m)
            return fail(PS_ERR_LENGTH, "ps_groth16_prove_multi: device " + std::to_string(d) + " does not hold its index range of the CRS arrays");
    }
    if (lag) return groth16_prove_multi_lagrange(dev, ndev, nn, r_be32, s_be32, A_out, B_out, C_out);
    // ---- quotient: A, B, h as big-endian scalars in host memory ----
    std::vector<uint8_t> hA, hB, hH;
    {
        auto piece = [&](size_t d, int what, std::vector<uint8_t>* dst) -> int {  // 0: A, 1: B, 2: h, 3: all three
            ps_scalars *a = nullptr, *b = nullptr, *h = nullptr;
            int rc = PS_OK;
            if (what == 0) rc = ps_qap_interpolate(dev[d].ctx, dev[d].qap, dev[d].sol, 0, &a);
            else if (what == 1) rc = ps_qap_interpolate(dev[d].ctx, dev[d].qap, dev[d].sol, 1, &b);
            else if (what == 2) rc = ps_qap_quotient(dev[d].ctx, dev[d].qap, dev[d].sol, nullptr, nullptr, nullptr, &h);
            else rc = ps_qap_quotient(dev[d].ctx, dev[d].qap, dev[d].sol, &a, &b, nullptr, &h);
            if (!rc && a) rc = g16_download_all(dev[d].ctx, a, what == 3 ? hA : *dst);
            if (!rc && b) rc = g16_download_all(dev[d].ctx, b, what == 3 ? hB : *dst);
            if (!rc && h) rc = g16_download_all(dev[d].ctx, h, what == 3 ? hH : *dst);
            ps_scalars_free(a); ps_scalars_free(b); ps_scalars_free(h);
            return rc;
        };
        int rc;
        if (ndev >= 3) {
            std::string errs[3];
            auto run = [&](size_t d, int what, std::vector<uint8_t>* dst) { int r2 = piece(d, what, dst); errs[what] = g_last_error; return r2; };
            std::future<int> fa = std::async(std::launch::async, run, (size_t)0, 0, &hA);
            std::future<int> fb = std::async(std::launch::async, run, (size_t)1, 1, &hB);
            int rh = run(2, 2, &hH);
            int ra = fa.get(), rb = fb.get();
            rc = rh ? rh : ra ? ra : rb;  // the h-only route carries the divisibility test ("apocalypse")
            if (rc) return fail(rc, errs[rh ? 2 : ra ? 0 : 1]);
        } else if ((rc = piece(0, 3, nullptr))) {
            return rc;
        }
    }
    // ---- per-device sums over the local arrays, one host thread per device ----
    struct Part { uint8_t A[96], B[192], C[96]; int rc = PS_OK; std::string err; };
    std::vector<Part> parts(ndev);
    auto work = [&](size_t d) {
        Part& pt = parts[d];
        ps_ctx* c = dev[d].ctx;
        const ps_groth16_pk& pk = dev[d].pk;
        size_t fn, cn, fh, ch, fq, cq;
        shard_range_c(n, (int)d, (int)ndev, &fn, &cn);
        shard_range_c(n - 1, (int)d, (int)ndev, &fh, &ch);
        shard_range_c(nn, (int)d, (int)ndev, &fq, &cq);
        ps_scalars *a = nullptr, *b = nullptr, *h = nullptr, *sn = nullptr;
        uint8_t pa[96], pb2[192], pb1[96], pn[96], ph[96];
        int rc = ps_scalars_upload(c, hA.data() + 32 * fn, cn, &a);
        if (!rc) rc = ps_scalars_upload(c, hB.data() + 32 * fn, cn, &b);
        if (!rc) rc = ps_scalars_upload(c, hH.data() + 32 * fh, ch, &h);
        if (!rc) rc = ps_scalars_slice(dev[d].sol, diff + fq, cq, &sn);
        // five sums through the context's queue of three: B over Xi2 first (the longest point pass)
        int pending = 0;
        if (!rc && !(rc = ps_msm_launch(c, pk.xi2, b))) pending++;
        if (!rc && !(rc = ps_msm_launch(c, pk.xi, a))) pending++;
        if (!rc && !(rc = ps_msm_launch(c, pk.xi, b))) pending++;
        uint8_t* outs[5] = {pb2, pa, pb1, pn, ph};
        int done = 0;
        auto finish = [&]() { int r2 = ps_msm_finish(c, outs[done++]); pending--; if (r2 && !rc) rc = r2; };
        if (pending) finish();
        if (!rc && !(rc = ps_msm_launch(c, pk.nio_lp, sn))) pending++;
        if (pending == 3 || (rc && pending)) finish();
        if (!rc && !(rc = ps_msm_launch(c, pk.xi_t, h))) pending++;
        while (pending) finish();
        ps_scalars_free(a); ps_scalars_free(b); ps_scalars_free(h); ps_scalars_free(sn);
        if (!rc) {  // C_d = N + H + s P_A + r P_B1 ; on device 0 also the fixed points of all three elements
            uint8_t two[2 * 96], sc2[64], w[96], three[3 * 96];
            memcpy(two, pa, 96); memcpy(two + 96, pb1, 96);
            memcpy(sc2, s_be32, 32); memcpy(sc2 + 32, r_be32, 32);
            rc = ps_points_lincomb(PS_G1, two, sc2, 2, w);
            memcpy(three, pn, 96); memcpy(three + 96, ph, 96); memcpy(three + 192, w, 96);
            if (!rc) rc = ps_points_sum(PS_G1, three, 3, pt.C);
            memcpy(pt.A, pa, 96);
            memcpy(pt.B, pb2, 192);
        }
        if (!rc && d == 0) rc = g16_add_fixed_points(pk, r_be32, s_be32, pt.A, pt.B, pt.C);
        pt.rc = rc;
        if (rc) pt.err = g_last_error;
    };
    {
        std::vector<std::future<void>> jobs;
        for (size_t d = 1; d < ndev; d++) jobs.push_back(std::async(std::launch::async, work, d));
        work(0);
        for (auto& j : jobs) j.get();
    }
    for (size_t d = 0; d < ndev; d++)
        if (parts[d].rc) return fail(parts[d].rc, parts[d].err);
    std::vector<uint8_t> fa(96 * ndev), fb(192 * ndev), fc(96 * ndev);
    for (size_t d = 0; d < ndev; d++) {
        memcpy(fa.data() + 96 * d, parts[d].A, 96);
        memcpy(fb.data() + 192 * d, parts[d].B, 192);
        memcpy(fc.data() + 96 * d, parts[d].C, 96);
    }
    int rc = ps_points_sum(PS_G1, fa.data(), ndev, A_out);
    if (!rc) rc = ps_points_sum(PS_G2, fb.data(), ndev, B_out);
    if (!rc) rc = ps_points_sum(PS_G1, fc.data(), ndev, C_out);
    return rc;
}

// ---------------------------------------------------------------------------------------
// PHGR13Prove over index ranges: one rank's share over the whole key (ps_phgr13_prove_shard, one process per GPU), and the
// devices of one process each holding only its ranges (ps_phgr13_prove_multi).  PHGR13 has no fixed points, so every proof
// element is the sum of the ranks' partial sums.  A share's sums are those of ps_phgr13_prove over the share's ranges: the
// seven solution sums (vs, ws, ys, vas, was, yas and the pointwise beta sum, one digit sort) and the h(s) sum.
// ---------------------------------------------------------------------------------------
static float phgr13_ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
}

static int phgr13_check_arrays(const ps_phgr13_ek* ek, const char* who) {
    const ps_points* arrs[10] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, ek->gsi, ek->vbs, ek->wbs, ek->ybs};
    for (auto* p : arrs)
        if (!p) return fail(PS_ERR_ARG, std::string(who) + ": NULL evaluation-key array");
    for (int k = 0; k < 10; k++)  // by position: the same array passed as vs and ws is still a G2 array where G1 belongs
        if (arrs[k]->group != (k == 1 ? PS_G2 : PS_G1)) return fail(PS_ERR_ARG, std::string(who) + ": evaluation-key array in the wrong group");
    if (ek->lgsi && ek->lgsi->group != PS_G1) return fail(PS_ERR_ARG, std::string(who) + ": evaluation-key array in the wrong group");
    return PS_OK;
}

struct Phgr13Share {
    const ps_points* pts[7];  // vs, ws, ys, vas, was, yas and the beta sum, over this share's range
    const ps_scalars* sv;     // solution[diff + first, cnt]
    const ps_points* hp;      // gsi -- or lgsi -- over this share's range of h
};
// hands over this share's range of h as a vector on the context (a view: phgr13_share_sums frees it)
typedef std::function<int(ps_scalars**)> Phgr13GetH;

// The sums of one share on context c.  h_first: h is at hand (the quotient ran on this context, alone): ps_phgr13_prove's
// order -- digit sort, h(s) sum, point passes.  Otherwise the sort and the seven point passes are launched first and h is
// awaited behind them; phase [0] is then that wait.  Whatever was launched is drained on every path, so that no sum stays
// pending on c or on its workers and the next call on the same context starts clean.
static int phgr13_share_sums(ps_ctx* c, const Phgr13Share& sh, bool h_first, const Phgr13GetH& get_h, ps_phgr13_proof* out) {
    if (c->pending || (c->aux && c->aux->pending)) return fail(PS_ERR_ARG, "PHGR13 share: an MSM is pending on this context");
    uint8_t* dst[7] = {out->vss, out->wss, out->yss, out->vass, out->wass, out->yass, out->gz};
    const size_t cnt = sh.sv->n;
    ps_ctx* ring[PS_MULTI_RING] = {nullptr, nullptr, nullptr, nullptr};
    MsmPlan mpl{};
    ps_scalars* h = nullptr;
    bool sums = false, h_launched = false;
    auto t_h = std::chrono::steady_clock::now();
    auto launch_h = [&]() -> int {
        const auto t_wait = std::chrono::steady_clock::now();
        int r2 = get_h(&h);
        if (!h_first) {
            c->phase_ms[0] = phgr13_ms_since(t_wait);
            t_h = std::chrono::steady_clock::now();
            // not chained behind an accumulation of an earlier call's workspace (the point passes above re-recorded them)
            c->last_chain = nullptr;
        }
        if (!r2 && !(r2 = msm_launch_impl(c, sh.hp, h, true))) h_launched = true;
        return r2;
    };
    int rc = PS_OK;
    if (cnt) {
        rc = msm_multi_ring(c, false, 7, ring);
        if (!rc) rc = msm_plan_checked(c, sh.pts, 7, cnt, sh.sv->max_bits, &mpl);
        // without h first the beta sum (and a fresh window table) may still be in flight on the context stream: fork
        if (!rc) rc = msm_multi_sort(c, ring, sh.sv, mpl, !h_first);
    }
    if (!rc && h_first) rc = launch_h();
    if (!rc && cnt) {
        hipEvent_t after_h = (h_first && h->n && c->last_chain) ? c->last_chain->ev_acc_local : nullptr;
        if (!(rc = msm_multi_points(c, ring, sh.pts, 7, sh.sv, mpl, after_h))) sums = true;
    }
    if (!rc && !h_first) rc = launch_h();
    if (rc) {  // what is in flight finishes before its buffers can be reused
        for (ps_ctx* w : ring)
            if (w) (void)ps_ctx_sync(w);
        (void)ps_ctx_sync(c);
    }
    uint8_t dump[96];
    if (h_launched) {
        int r2 = ps_msm_finish(c, rc ? dump : out->hs);
        if (!rc) rc = r2;
    }
    c->phase_ms[1] = phgr13_ms_since(t_h);
    const auto t_sums = std::chrono::steady_clock::now();
    if (sums) {
        int r2 = msm_multi_finish(c, ring[0], sh.pts, 7, mpl, rc ? nullptr : dst);
        if (!rc) rc = r2;
    }
    c->phase_ms[2] = phgr13_ms_since(t_sums);
    if (!rc && !cnt)  // an empty range: every solution sum is the identity
        for (int i = 0; i < 7; i++) write_identity(i == 1 ? PS_G2 : PS_G1, dst[i]);
    ps_scalars_free(h);
    return rc;
}

extern "C" int ps_phgr13_prove_shard(ps_ctx* c, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sol, int rank, int world,
                                     ps_phgr13_proof* part) {
    if (!c || !ek || !q || !sol || !part) return fail(PS_ERR_ARG, "ps_phgr13_prove_shard: NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(PS_ERR_ARG, "ps_phgr13_prove_shard: bad rank / world");
    int rc = phgr13_check_arrays(ek, "ps_phgr13_prove_shard");
    if (rc) return rc;
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck
    if (q->n < 2) return fail(PS_ERR_ARG, "ps_phgr13_prove_shard: needs at least 2 gates");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    const size_t n = q->n, diff = q->m - q->nio, nn = ek->vs->n;
    for (const ps_points* p : {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, ek->vbs, ek->wbs, ek->ybs})
        if (p->n != nn) return fail(PS_ERR_LENGTH, "ps_phgr13_prove_shard: the nine solution arrays of the key differ in length");
    if (diff + nn > sol->n) return fail(PS_ERR_LENGTH, "evaluation-key array longer than the non-IO part of the solution");
    if (ek->gsi->n != n - 1 || (ek->lgsi && ek->lgsi->n != n - 1))  // algebra.go:350-352
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(n - 1) + " and blinded eval points " +
                                       std::to_string(ek->gsi->n != n - 1 ? ek->gsi->n : ek->lgsi->n));
    if (c->pending || (c->aux && c->aux->pending)) return fail(PS_ERR_ARG, "ps_phgr13_prove_shard: an MSM is pending on this context");
    const ps_points* gsi = ek->lgsi ? ek->lgsi : ek->gsi;
    if (nn) {  // as ps_phgr13_prove: the beta sum and the window tables of the whole arrays, once per key (views of them get their own)
        if ((rc = phgr13_beta_sum(c, ek))) return rc;
        if (tables_wanted(c, nn)) {
            const ps_points* whole[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, c->phgr_bsum};
            for (int i = 0; i < 7 && !rc; i++) rc = points_ensure_table(c, whole[i], 0, true);
            if (!rc && gsi->n >= PS_TABLE_MIN_POINTS) rc = points_ensure_table(c, gsi, 0, true);
            if (rc) return rc;
        }
    }
    if ((rc = quotient_run(c, q, sol, ek->lgsi ? Q_H_VALUES : Q_H_ONLY))) return rc;
    size_t fs, cs, fh, ch;
    shard_range_c(nn, rank, world, &fs, &cs);
    shard_range_c(n - 1, rank, world, &fh, &ch);
    ps_scalars* h = nullptr;  // the context's own vector (slot 3, as ps_phgr13_prove): this rank's range of h only
    if ((rc = prover_vector(c, 3, ch, &h))) return rc;
    if (ch)
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(ch)), dim3(256), 0, c->stream, (u32*)h->st->p,
                           (const Fr*)(ek->lgsi ? q->qt.scratch : q->hbuf) + fh, (u64)ch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->phase_ms[0] = phgr13_ms_since(t_start);
    const ps_points* whole[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, nn ? c->phgr_bsum : ek->vbs};
    ps_points* views[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ps_scalars* sv = nullptr;
    for (int i = 0; i < 7 && !rc; i++) rc = ps_points_slice(whole[i], fs, cs, &views[i]);
    if (!rc) rc = ps_points_slice(gsi, fh, ch, &views[7]);
    if (!rc) rc = ps_scalars_slice(sol, diff + fs, cs, &sv);
    if (!rc) {
        const Phgr13Share sh{{views[0], views[1], views[2], views[3], views[4], views[5], views[6]}, sv, views[7]};
        rc = phgr13_share_sums(c, sh, true, [&](ps_scalars** o) { return ps_scalars_slice(h, 0, ch, o); }, part);
    }
    for (ps_points* v : views) ps_points_free(v);
    ps_scalars_free(sv);
    c->phase_ms[3] = phgr13_ms_since(t_start);
    return rc;
}

// Peer access from `dev` to `peer`, asked for once per pair where the hardware allows it.  The copies of h do not depend on
// it (hipMemcpyPeerAsync works either way); "already enabled", or a refusal, is cleared so that it does not surface as the
// next launch's error.
static void peer_access_once(int dev, int peer) {
    static std::mutex mu;
    static std::vector<std::pair<int, int>> asked;
    std::lock_guard<std::mutex> lk(mu);
    for (auto& p : asked)
        if (p.first == dev && p.second == peer) return;
    asked.push_back({dev, peer});
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dev, peer) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(peer, 0);
    (void)hipGetLastError();
}

// PHGR13Prove (pinochio.go:207-254) over `ndev` devices of this process, every device holding only its index ranges of the
// evaluation key.  The quotient runs ONCE, on dev[0], alone (as in ps_phgr13_prove: it and the accumulations are both
// VALU-bound) and leaves h, plain limbs, in dev[0]'s context vector; an event recorded behind that conversion is the only
// thing the other devices wait for.  Devices 1.. launch their digit sort and seven point passes at once, then wait for h on
// the host (a condition variable: released with h, or with the first error of any device), make their stream wait for the
// event and copy their range of h device to device into their own context vector -- no byte of h crosses host memory, no
// upload, no allocation once the contexts are warm -- and launch the h(s) sum.  One host thread per device; the partial
// proofs are folded on the host.
extern "C" int ps_phgr13_prove_multi(const ps_phgr13_device* dev, size_t ndev, ps_phgr13_proof* out) {
    if (!dev || ndev == 0 || !out) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: NULL argument");
    if (ndev > 64) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: at most 64 devices");
    for (size_t d = 0; d < ndev; d++) {
        if (!dev[d].ctx || !dev[d].qap || !dev[d].sol) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: NULL handle");
        int rc = phgr13_check_arrays(&dev[d].ek, "ps_phgr13_prove_multi");
        if (rc) return rc;
        for (size_t e = 0; e < d; e++)
            if (dev[e].ctx == dev[d].ctx) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: one context per device (a context appears twice)");
    }
    const bool lag = dev[0].ek.lgsi != nullptr;
    for (size_t d = 0; d < ndev; d++)
        if ((dev[d].ek.lgsi != nullptr) != lag) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: lgsi must be on every device or on none");
    const size_t n = dev[0].qap->n, m = dev[0].qap->m, diff = m - dev[0].qap->nio;
    if (n < 2) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: needs at least 2 gates");
    size_t nn = 0;
    for (size_t d = 0; d < ndev; d++) nn += dev[d].ek.vs->n;
    if (diff + nn > m)
        return fail(PS_ERR_LENGTH, "ps_phgr13_prove_multi: the devices' ranges of vs add up to " + std::to_string(nn) +
                                       " points, more than the non-IO part of the solution (" + std::to_string(m - diff) + ")");
    for (size_t d = 0; d < ndev; d++) {  // every local array must be exactly this device's range (algebra.go:350-352 otherwise)
        const ps_phgr13_ek& ek = dev[d].ek;
        size_t f, cnt;
        shard_range_c(nn, (int)d, (int)ndev, &f, &cnt);
        bool ok = true;
        for (const ps_points* p : {ek.vs, ek.ws, ek.ys, ek.vas, ek.was, ek.yas, ek.vbs, ek.wbs, ek.ybs}) ok = ok && p->n == cnt;
        shard_range_c(n - 1, (int)d, (int)ndev, &f, &cnt);
        ok = ok && ek.gsi->n == cnt && (!ek.lgsi || ek.lgsi->n == cnt);
        if (!ok || dev[d].qap->n != n || dev[d].qap->m != m || dev[d].sol->n != m)
            return fail(PS_ERR_LENGTH, "ps_phgr13_prove_multi: device " + std::to_string(d) + " does not hold its index range of the evaluation-key arrays");
    }
    ps_ctx* const c0 = dev[0].ctx;
    struct {
        std::mutex mu;
        std::condition_variable cv;
        int state = 0;    // 0: no h yet; 1: h on dev[0] (c0->ev_q recorded behind it); -1: released with an error
        int err = PS_OK;  // the first error of any device, and its text
        std::string msg;
        ps_scalars* h0 = nullptr;
    } ho;
    auto fail_all = [&](int rc) {
        std::lock_guard<std::mutex> lk(ho.mu);
        if (!ho.err) { ho.err = rc; ho.msg = g_last_error; }
        if (ho.state == 0) ho.state = -1;
        ho.cv.notify_all();
    };
    std::vector<ps_phgr13_proof> parts(ndev);
    auto work = [&](size_t d) {
        ps_ctx* c = dev[d].ctx;
        const ps_phgr13_ek& ek = dev[d].ek;
        const auto t_start = std::chrono::steady_clock::now();
        int rc = hipSetDevice(c->device) == hipSuccess ? PS_OK : fail(PS_ERR_HIP, "ps_phgr13_prove_multi: hipSetDevice failed");
        size_t fs, cs, fh, ch;
        shard_range_c(nn, (int)d, (int)ndev, &fs, &cs);
        shard_range_c(n - 1, (int)d, (int)ndev, &fh, &ch);
        const ps_points* hp = lag ? ek.lgsi : ek.gsi;
        if (!rc && (c->pending || (c->aux && c->aux->pending))) rc = fail(PS_ERR_ARG, "ps_phgr13_prove_multi: an MSM is pending on a context");
        if (!rc && cs) {  // as ps_phgr13_prove, over the local arrays
            rc = phgr13_beta_sum(c, &ek);
            if (!rc && tables_wanted(c, cs)) {
                const ps_points* loc[7] = {ek.vs, ek.ws, ek.ys, ek.vas, ek.was, ek.yas, c->phgr_bsum};
                for (int i = 0; i < 7 && !rc; i++) rc = points_ensure_table(c, loc[i], 0, true);
                if (!rc && hp->n >= PS_TABLE_MIN_POINTS) rc = points_ensure_table(c, hp, 0, true);
            }
        }
        ps_scalars* sv = nullptr;
        if (!rc) rc = ps_scalars_slice(dev[d].sol, diff + fs, cs, &sv);
        const Phgr13Share sh{{ek.vs, ek.ws, ek.ys, ek.vas, ek.was, ek.yas, cs ? c->phgr_bsum : ek.vbs}, sv, hp};
        if (d == 0) {
            const ps_qap* q = dev[0].qap;
            ps_scalars* h = nullptr;  // the context's own vector (slot 3, as ps_phgr13_prove): all of h, the others copy from it
            if (!rc) rc = quotient_run(c, q, dev[0].sol, lag ? Q_H_VALUES : Q_H_ONLY);
            if (!rc) rc = prover_vector(c, 3, n - 1, &h);
            if (!rc) {
                hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(n - 1)), dim3(256), 0, c->stream, (u32*)h->st->p,
                                   (const Fr*)(lag ? q->qt.scratch : q->hbuf), (u64)(n - 1));
                hipError_t e = hipGetLastError();
                if (e == hipSuccess && !c->ev_q) e = hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventRecord(c->ev_q, c->stream);
                if (e != hipSuccess) rc = fail(PS_ERR_HIP, std::string("ps_phgr13_prove_multi: h: ") + hipGetErrorString(e));
            }
            if (rc) {
                fail_all(rc);
            } else {
                std::lock_guard<std::mutex> lk(ho.mu);
                ho.h0 = h;
                if (ho.state == 0) ho.state = 1;
                ho.cv.notify_all();
            }
            if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(PS_ERR_HIP, "ps_phgr13_prove_multi: quotient: stream synchronisation failed");
            c->phase_ms[0] = phgr13_ms_since(t_start);
            if (!rc) rc = phgr13_share_sums(c, sh, true, [&](ps_scalars** o) { return ps_scalars_slice(h, fh, ch, o); }, &parts[0]);
        } else if (!rc) {
            auto get_h = [&](ps_scalars** o) -> int {
                {
                    std::unique_lock<std::mutex> lk(ho.mu);
                    ho.cv.wait(lk, [&] { return ho.state != 0; });
                    if (ho.state < 0) return fail(ho.err, ho.msg);
                }
                ps_scalars* hl = nullptr;  // this device's context vector (slot 3): its range of h
                int r2 = prover_vector(c, 3, ch, &hl);
                if (r2) return r2;
                HIP_TRY(hipStreamWaitEvent(c->stream, c0->ev_q, 0));
                if (ch) {
                    const u32* src = scalars_ptr(ho.h0) + 8 * fh;
                    if (c->device == c0->device) {
                        HIP_TRY(hipMemcpyAsync(hl->st->p, src, 32 * ch, hipMemcpyDeviceToDevice, c->stream));
                    } else {
                        peer_access_once(c->device, c0->device);
                        HIP_TRY(hipMemcpyPeerAsync(hl->st->p, c->device, src, c0->device, 32 * ch, c->stream));
                    }
                }
                HIP_TRY(hipStreamSynchronize(c->stream));
                return ps_scalars_slice(hl, 0, ch, o);
            };
            rc = phgr13_share_sums(c, sh, false, get_h, &parts[d]);
        }
        if (rc) fail_all(rc);
        ps_scalars_free(sv);
        c->phase_ms[3] = phgr13_ms_since(t_start);
    };
    {
        std::vector<std::future<void>> jobs;
        for (size_t d = 1; d < ndev; d++) jobs.push_back(std::async(std::launch::async, work, d));
        work(0);
        for (auto& j : jobs) j.get();
    }
    if (ho.err) return fail(ho.err, ho.msg);
    const size_t off[8] = {offsetof(ps_phgr13_proof, vss), offsetof(ps_phgr13_proof, vass), offsetof(ps_phgr13_proof, wss),
                           offsetof(ps_phgr13_proof, wass), offsetof(ps_phgr13_proof, yss), offsetof(ps_phgr13_proof, yass),
                           offsetof(ps_phgr13_proof, hs), offsetof(ps_phgr13_proof, gz)};
    for (int k = 0; k < 8; k++) {
        const int group = off[k] == offsetof(ps_phgr13_proof, wss) ? PS_G2 : PS_G1;
        const size_t wb = wire_bytes(group);
        std::vector<uint8_t> flat(wb * ndev);
        for (size_t d = 0; d < ndev; d++) memcpy(flat.data() + wb * d, (const uint8_t*)&parts[d] + off[k], wb);
        int rc = ps_points_sum(group, flat.data(), ndev, (uint8_t*)out + off[k]);
        if (rc) return rc;
    }
    return PS_OK;
}

// ---------------------------------------------------------------------------------------
// Groth16Prove over rank-local LAGRANGE-form keys: ps_groth16_prove_multi (the devices of one process) and
// ps_groth16_prove_local (one process per GPU).  With lxi / lxi2 in the key the scalars of A, B and B1' are the wire values
// a_j = (L.s)_j, b_j = (R.s)_j, so a device that holds lxi[range] and lxi2[range] gets exactly the scalars it needs from its
// OWN rows of the three sparse products (k_own_rows): those three sums need no exchange at all.  Only the n-1 values h(n+k)
// depend on the whole circuit.  C's share is N + H + s A + r B1' as in the split form of groth16_prove_impl.
// ---------------------------------------------------------------------------------------
struct G16LocalShare {
    const ps_points *lxi, *lxi2, *lxi_t, *nio_lp;  // this share's ranges of the key
    const ps_qap* q;
    const ps_scalars* sol;
    int rank, world;
    size_t nn;                    // len(NioLP) of the whole key
    const ps_groth16_pk* fixed;   // the key whose fixed points this share adds, or nullptr
};
// Called once the own-row kernels are enqueued on the share's stream (the witness is in q->sol_m): whatever this device
// contributes to the values route.
typedef std::function<int(hipStream_t)> G16Produce;
// Hands over S[0..2]: this share's range (ch values from node index fh on) of the three convolutions, in memory of this
// device, valid for work enqueued on the stream afterwards.  May block the host until the convolutions exist.
typedef std::function<int(hipStream_t, const Fr* S[3])> G16GetS;

static int g16_lagrange_share(ps_ctx* c, const G16LocalShare& sh, const uint8_t* r_be32, const uint8_t* s_be32, const G16Produce& produce,
                              const G16GetS& get_s, uint8_t* A_part, uint8_t* B_part, uint8_t* C_part) {
    const ps_qap* q = sh.q;
    const ps_scalars* sol = sh.sol;
    const size_t n = q->n, diff = q->m - q->nio;
    size_t fn, cn, fh, ch, fq, cq;
    shard_range_c(n, sh.rank, sh.world, &fn, &cn);
    shard_range_c(n - 1, sh.rank, sh.world, &fh, &ch);
    shard_range_c(sh.nn, sh.rank, sh.world, &fq, &cq);
    if (c->pending || (c->aux && c->aux->pending)) return fail(PS_ERR_ARG, "Groth16 share: an MSM is pending on this context");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    int rc = PS_OK;
    // window tables over the local arrays, once per array (lxi serves A and B1'); an int64 witness keeps its short-scalar
    // plan over NioLP, which no table of full-width windows helps
    for (const ps_points* arr : {sh.lxi2, sh.lxi, sh.lxi_t, sh.nio_lp})
        if (!rc && tables_wanted(c, arr->n) && (arr != sh.nio_lp || sol->max_bits >= 255)) rc = points_ensure_table(c, arr, 0, true);
    ps_scalars *va = nullptr, *vb = nullptr, *vh = nullptr, *sn = nullptr;  // the context's own vectors, and a view of the solution
    if (!rc) rc = prover_vector(c, 0, cn, &va);
    if (!rc) rc = prover_vector(c, 1, cn, &vb);
    if (!rc) rc = prover_vector(c, 2, ch, &vh);
    if (!rc && !c->ev_q && hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming) != hipSuccess) rc = fail(PS_ERR_HIP, "Groth16 share: event creation failed");
    if (!rc) rc = ps_scalars_slice(sol, diff + fq, cq, &sn);
    if (rc) { ps_scalars_free(sn); return rc; }
    // the share's own kernels run on the context's high-priority stream, as the quotient of groth16_prove_impl does: the sums
    // launched right behind them (worker contexts) must not hold back what every other device may be waiting for
    hipStream_t qs = c->tail;
    std::vector<int> fifo;  // sums pending on the context, oldest first: 0 B.lxi2, 1 A.lxi, 2 B1' = b.lxi, 3 sol.NioLP, 4 h.lxi_t
    uint8_t part[5][192];
    for (int k = 0; k < 5; k++) write_identity(k == 0 ? PS_G2 : PS_G1, part[k]);
    int rcb = PS_OK;
    auto t_h = t_start;
    float h_ms = 0.f;
    auto finish_one = [&]() {
        const int kind = fifo.front();
        fifo.erase(fifo.begin());
        int r2 = ps_msm_finish(c, part[kind]);
        if (r2 && !rcb) rcb = r2;
        if (kind == 4) h_ms = phgr13_ms_since(t_h);
    };
    auto launch = [&](int kind, const ps_points* pts, const ps_scalars* sc) -> int {
        while (fifo.size() + 1 > PS_PROVER_QUEUE) finish_one();  // the oldest sum is the furthest along
        int r2 = msm_launch_impl(c, pts, sc, false);
        if (!r2) fifo.push_back(kind);
        return r2;
    };
    float own_ms = 0.f, wait_ms = 0.f;
    do {
        hipError_t e = hipEventRecord(c->ev_q, c->stream);  // ordered after whatever the caller left on the context stream
        if (e == hipSuccess) e = hipStreamWaitEvent(qs, c->ev_q, 0);
        if (e != hipSuccess || storage_wait_ready(sol->st, qs)) { rc = fail(PS_ERR_HIP, "Groth16 share: event wait failed"); break; }
        // 1. the witness in Montgomery form, then a_j, b_j of the own rows, their gate check and their scalars in one pass
        hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(q->m)), dim3(256), 0, qs, q->sol_m, scalars_ptr(sol), (u64)q->m);
        e = hipMemsetAsync(c->d_flag, 0, 4, qs);
        if (cn) {
            Csr3 m3;
            for (int k = 0; k < 3; k++) m3.m[k] = CsrView{q->mat[k].row_ptr, q->mat[k].col, q->mat[k].val};
            u32 *a = (u32*)va->st->p, *b = (u32*)vb->st->p;
            hipLaunchKernelGGL(k_own_rows, dim3(nblk(cn)), dim3(256), 0, qs, m3, (const Fr*)q->sol_m, (u32)fn, (u32)cn, a, b, c->d_flag);
            // the part of the QAP's (global, ascending) list of long rows that lies in [fn, fn + cn)
            const auto lo = std::lower_bound(q->long_any_h.begin(), q->long_any_h.end(), (u32)fn);
            const auto hi = std::lower_bound(lo, q->long_any_h.end(), (u32)(fn + cn));
            if (hi != lo)
                hipLaunchKernelGGL(k_own_rows_long, dim3((unsigned)(hi - lo)), dim3(256), 0, qs, m3, (const Fr*)q->sol_m,
                                   (const u32*)q->long_any + (lo - q->long_any_h.begin()), (u32)fn, a, b, c->d_flag);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) { rc = fail(PS_ERR_HIP, std::string("Groth16 share: own rows: ") + hipGetErrorString(e)); break; }
        if (storage_mark_ready(va->st, qs) || storage_mark_ready(vb->st, qs)) { rc = fail(PS_ERR_HIP, "event record failed"); break; }
        if (produce && (rc = produce(qs))) break;
        // 2. at once, without waiting for any h: B.lxi2 (G2, the longest point pass) first, A.lxi, B1' = b.lxi, then sol.NioLP
        if ((rc = launch(0, sh.lxi2, vb)) || (rc = launch(1, sh.lxi, va)) || (rc = launch(2, sh.lxi, vb))) break;
        u32 flag = 0;  // the gate check's answer for the own rows
        if (hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, qs) != hipSuccess || hipStreamSynchronize(qs) != hipSuccess) {
            rc = fail(PS_ERR_HIP, "Groth16 share: reading the gate check failed");
            break;
        }
        own_ms = phgr13_ms_since(t_start);
        if (flag) { rc = fail(PS_ERR_NOT_DIVISIBLE, "apocalypse"); break; }  // qap.go:158-160
        if ((rc = launch(3, sh.nio_lp, sn))) break;
        // 3. h on the own range of nodes, from the three convolutions wherever they were computed, then h.lxi_t behind it
        const auto t_wait = std::chrono::steady_clock::now();
        if (ch) {
            const Fr* S[3] = {nullptr, nullptr, nullptr};
            if ((rc = get_s(qs, S))) break;
            hipLaunchKernelGGL(k_h_values_range, dim3(nblk(ch)), dim3(256), 0, qs, (u32*)vh->st->p, S[0], S[1], S[2], (const Fr*)q->qt.fact2,
                               (const Fr*)q->qt.invfact, (u64)n, (u64)fh, (u64)ch);
            if (hipGetLastError() != hipSuccess) { rc = fail(PS_ERR_HIP, "Groth16 share: h on the own range failed"); break; }
        }
        if (storage_mark_ready(vh->st, qs)) { rc = fail(PS_ERR_HIP, "event record failed"); break; }
        wait_ms = phgr13_ms_since(t_wait);
        t_h = std::chrono::steady_clock::now();
        if ((rc = launch(4, sh.lxi_t, vh))) break;
    } while (0);
    // everything that was launched is drained on every path: the next call on this context starts clean
    while (!fifo.empty()) finish_one();
    (void)hipStreamSynchronize(qs);
    ps_scalars_free(sn);
    if (rc || rcb) {
        std::string keep = g_last_error;
        (void)ps_ctx_sync(c);
        g_last_error = keep;
        return rc ? rc : rcb;
    }
    // C_part = N + H + s A_part + r B1'_part (groth16.go:180-205, the fixed points apart)
    uint8_t two[2 * 96], sc2[64], w[96], three[3 * 96];
    memcpy(two, part[1], 96); memcpy(two + 96, part[2], 96);
    memcpy(sc2, s_be32, 32); memcpy(sc2 + 32, r_be32, 32);
    rc = ps_points_lincomb(PS_G1, two, sc2, 2, w);
    memcpy(three, part[3], 96); memcpy(three + 96, part[4], 96); memcpy(three + 192, w, 96);
    if (!rc) rc = ps_points_sum(PS_G1, three, 3, C_part);
    memcpy(A_part, part[1], 96);
    memcpy(B_part, part[0], 192);
    if (!rc && sh.fixed) rc = g16_add_fixed_points(*sh.fixed, r_be32, s_be32, A_part, B_part, C_part);
    c->phase_ms[0] = own_ms + wait_ms;
    c->phase_ms[1] = h_ms;
    c->phase_ms[3] = phgr13_ms_since(t_start);
    c->phase_ms[2] = std::max(0.f, c->phase_ms[3] - c->phase_ms[0] - c->phase_ms[1]);
    return rc;
}

static int g16_local_key_check(const ps_groth16_pk& pk, const char* who) {
    if (pk.lxi->group != PS_G1 || pk.lxi_t->group != PS_G1 || pk.nio_lp->group != PS_G1 || pk.lxi2->group != PS_G2)
        return fail(PS_ERR_ARG, std::string(who) + ": CRS array in the wrong group");
    return PS_OK;
}

// ps_groth16_prove_multi, every device with lxi / lxi2 / lxi_t (the caller has checked handles and ranges).  One host thread
// per device runs g16_lagrange_share.  The values route -- three convolutions of length 2 np -- is split over devices 0, 1, 2
// BY POLYNOMIAL (device k: the full sparse product of matrix k, its Lagrange weights, one convolution), not by node range: a
// range of n / D outputs of a length-n convolution still needs a transform of >= n + n / D points, which rounds up to the same
// 2 np, so a split by range saves nothing.  With fewer than three devices (or PS_G16_MULTI_HSPLIT=0) dev[0] runs all three as
// the batch of quotient_h_values.  Either way an event is recorded behind each convolution; every device makes its stream
// wait for the three events, copies its ranges of S_0, S_1, S_2 (3 x 40 bytes per node of its range) device to device into
// buffers of its own QAP (coefA / coefB / coefC: idle on this route) and runs k_h_values_range.  No byte of A, B or h crosses
// host memory, nothing is allocated once the contexts are warm.  The gate check is the union of the devices' own-row flags:
// the first error of any device releases every device that waits, and every device drains what it launched.
static int groth16_prove_multi_lagrange(const ps_groth16_device* dev, size_t ndev, size_t nn, const uint8_t* r_be32, const uint8_t* s_be32,
                                        uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    for (size_t d = 0; d < ndev; d++) {
        int rc = g16_local_key_check(dev[d].pk, "ps_groth16_prove_multi");
        if (rc) return rc;
        for (size_t e = 0; e < d; e++)
            if (dev[e].ctx == dev[d].ctx) return fail(PS_ERR_ARG, "ps_groth16_prove_multi: one context per device (a context appears twice)");
    }
    const size_t n = dev[0].qap->n;
    const bool hsplit = ndev >= 3 && dev[0].ctx->g16_multi_hsplit;
    struct {
        std::mutex mu;
        std::condition_variable cv;
        int err = PS_OK;  // the first error of any device, and its text
        std::string msg;
        int have = 0;     // convolutions at hand (3: all)
        const Fr* S[3] = {nullptr, nullptr, nullptr};
        int sdev[3] = {0, 0, 0};
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    } ho;
    auto fail_all = [&](int rc) {
        std::lock_guard<std::mutex> lk(ho.mu);
        if (!ho.err) { ho.err = rc; ho.msg = g_last_error; }
        ho.cv.notify_all();
    };
    struct Part { uint8_t A[96], B[192], C[96]; };
    std::vector<Part> parts(ndev);
    auto work = [&](size_t d) {
        ps_ctx* c = dev[d].ctx;
        const ps_qap* q = dev[d].qap;
        const ps_groth16_pk& pk = dev[d].pk;
        size_t fh, ch;
        shard_range_c(n - 1, (int)d, (int)ndev, &fh, &ch);
        const G16LocalShare sh{pk.lxi, pk.lxi2, pk.lxi_t, pk.nio_lp, q, dev[d].sol, (int)d, (int)ndev, nn, d == 0 ? &dev[0].pk : nullptr};
        // The values route ahead of the device's own sums (as the quotient of groth16_prove_impl runs first): every other
        // device waits for it.  (Behind the sums instead: not measured yet.)
        auto produce = [&](hipStream_t qs) -> int {
            if (hsplit ? d >= 3 : d != 0) return PS_OK;
            const NttTables& tabs = *ctx_tabs(c);
            Fr* S[3] = {nullptr, nullptr, nullptr};
            hipError_t e;
            if (hsplit) {
                spmv_launch(qs, q->mat[d], (const Fr*)q->sol_m, q->y[d], (u32)n);
                e = quotient_h_conv_one(tabs, qs, q->qt, q->y[d], &S[d]);
            } else {
                for (int k = 0; k < 3; k++) spmv_launch(qs, q->mat[k], (const Fr*)q->sol_m, q->y[k], (u32)n);
                e = quotient_h_convs(tabs, qs, q->qt, q->y[0], q->y[1], q->y[2], S);
            }
            if (e == hipSuccess) e = hipEventRecord(c->ev_q, qs);
            if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_prove_multi: values route: ") + hipGetErrorString(e));
            std::lock_guard<std::mutex> lk(ho.mu);
            for (int k = 0; k < 3; k++)
                if (S[k]) { ho.S[k] = S[k]; ho.sdev[k] = c->device; ho.ev[k] = c->ev_q; ho.have++; }
            ho.cv.notify_all();
            return PS_OK;
        };
        auto get_s = [&](hipStream_t qs, const Fr* out[3]) -> int {
            const Fr* S[3];
            int sdev[3];
            hipEvent_t ev[3];
            {
                std::unique_lock<std::mutex> lk(ho.mu);
                ho.cv.wait(lk, [&] { return ho.err != PS_OK || ho.have == 3; });
                if (ho.err) return fail(ho.err, ho.msg);
                for (int k = 0; k < 3; k++) { S[k] = ho.S[k]; sdev[k] = ho.sdev[k]; ev[k] = ho.ev[k]; }
            }
            Fr* dst[3] = {q->coefA, q->coefB, q->coefC};
            for (int k = 0; k < 3; k++) {
                HIP_TRY(hipStreamWaitEvent(qs, ev[k], 0));
                const Fr* src = S[k] + (n - 1 + fh);  // S_P for hv[i] sits at n - 1 + i
                if (sdev[k] == c->device) {
                    HIP_TRY(hipMemcpyAsync(dst[k], src, sizeof(Fr) * ch, hipMemcpyDeviceToDevice, qs));
                } else {
                    peer_access_once(c->device, sdev[k]);
                    HIP_TRY(hipMemcpyPeerAsync(dst[k], c->device, src, sdev[k], sizeof(Fr) * ch, qs));
                }
                out[k] = dst[k];
            }
            return PS_OK;
        };
        int rc = g16_lagrange_share(c, sh, r_be32, s_be32, produce, get_s, parts[d].A, parts[d].B, parts[d].C);
        if (rc) fail_all(rc);
    };
    {
        std::vector<std::future<void>> jobs;
        for (size_t d = 1; d < ndev; d++) jobs.push_back(std::async(std::launch::async, work, d));
        work(0);
        for (auto& j : jobs) j.get();
    }
    if (ho.err) return fail(ho.err, ho.msg);
    std::vector<uint8_t> fa(96 * ndev), fb(192 * ndev), fc(96 * ndev);
    for (size_t d = 0; d < ndev; d++) {
        memcpy(fa.data() + 96 * d, parts[d].A, 96);
        memcpy(fb.data() + 192 * d, parts[d].B, 192);
        memcpy(fc.data() + 96 * d, parts[d].C, 96);
    }
    int rc = ps_points_sum(PS_G1, fa.data(), ndev, A_out);
    if (!rc) rc = ps_points_sum(PS_G2, fb.data(), ndev, B_out);
    if (!rc) rc = ps_points_sum(PS_G1, fc.data(), ndev, C_out);
    return rc;
}

// One rank's share when the rank holds ONLY its index ranges of a Lagrange-form key (one process per GPU).  Processes cannot
// copy peer to peer, and the values route is 2 ms at 2^20 constraints: every rank computes it itself (with the gate check
// over ALL rows, so every rank of an unsatisfied witness reports it) rather than wait for three broadcasts.
extern "C" int ps_groth16_prove_local(ps_ctx* c, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol, const uint8_t* r_be32,
                                      const uint8_t* s_be32, int rank, int world, uint8_t* A_part, uint8_t* B_part, uint8_t* C_part) {
    if (!c || !pk || !q || !sol || !r_be32 || !s_be32 || !A_part || !B_part || !C_part) return fail(PS_ERR_ARG, "ps_groth16_prove_local: NULL argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(PS_ERR_ARG, "ps_groth16_prove_local: bad rank / world");
    if (!pk->nio_lp || !g16_lagrange(pk)) return fail(PS_ERR_ARG, "ps_groth16_prove_local: the key must carry lxi, lxi2 and lxi_t (and NioLP)");
    int rc = g16_local_key_check(*pk, "ps_groth16_prove_local");
    if (rc) return rc;
    const size_t n = q->n, nn = q->nio;  // len(NioLP) = nbVars - diff = nbIO (groth16.go:86-91)
    if (n < 2) return fail(PS_ERR_ARG, "ps_groth16_prove_local: needs at least 2 gates");
    if (sol->n != q->m) return fail(PS_ERR_ARG, "different number of solution variables than left polynomials");  // sanityCheck
    size_t f, cn, fh, ch, cq;
    shard_range_c(n, rank, world, &f, &cn);
    shard_range_c(n - 1, rank, world, &fh, &ch);
    shard_range_c(nn, rank, world, &f, &cq);
    if (pk->lxi->n != cn || pk->lxi2->n != cn || pk->lxi_t->n != ch || pk->nio_lp->n != cq)
        return fail(PS_ERR_LENGTH, "ps_groth16_prove_local: rank " + std::to_string(rank) + " of " + std::to_string(world) +
                                       " does not hold its index range of the CRS arrays");
    Fr* S[3] = {nullptr, nullptr, nullptr};
    auto produce = [&](hipStream_t qs) -> int {
        for (int k = 0; k < 3; k++) spmv_launch(qs, q->mat[k], (const Fr*)q->sol_m, q->y[k], (u32)n);
        hipLaunchKernelGGL(k_check_gates, dim3(nblk(n)), dim3(256), 0, qs, (const Fr*)q->y[0], (const Fr*)q->y[1], (const Fr*)q->y[2], (u32)n,
                           c->d_flag);
        hipError_t e = quotient_h_convs(*ctx_tabs(c), qs, q->qt, q->y[0], q->y[1], q->y[2], S);
        if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_prove_local: values route: ") + hipGetErrorString(e));
        return PS_OK;
    };
    auto get_s = [&](hipStream_t, const Fr* out[3]) -> int {
        for (int k = 0; k < 3; k++) out[k] = S[k] + (n - 1 + fh);
        return PS_OK;
    };
    const G16LocalShare sh{pk->lxi, pk->lxi2, pk->lxi_t, pk->nio_lp, q, sol, rank, world, nn, rank == world - 1 ? pk : nullptr};
    return g16_lagrange_share(c, sh, r_be32, s_be32, produce, get_s, A_part, B_part, C_part);
}
