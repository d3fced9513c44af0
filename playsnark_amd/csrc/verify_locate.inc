// ps_groth16_verify_batch_locate: WHICH proofs of a rejected batch are invalid, by bisection over partial results kept on the
// device (included by capi.hip after verify_batch.inc and locate_dev.hpp).  With F_S = prod_{i in S} miller(rho_i A_i, B_i),
// R_S = sum rho_i, C_S = sum rho_i C_i, t_S,j = sum rho_i io_ij and X_S = sum_j t_S,j IoLP_j,
//     check(S):  final_exp(F_S miller(-R_S alpha, beta2) miller(-X_S, gamma) miller(-C_S, delta2)) == 1
// is the batch equation restricted to S, multiplicative over disjoint unions: a set that passes needs no further look, one
// that fails has a failing half, and check({i}) is proof i's own equation raised to rho_i != 0 (GT has prime order).
//   1. the batch check of ps_groth16_verify_batch (verify_batch_impl), the levels of its product tree kept: accepted ->
//      done, one check, nothing else launched;
//   2. otherwise the C tree and the scalar tree (locate_dev.hpp), built once;
//   3. the descent: locate_bisect (locate_descent.hpp, shared with verify_phgr13_locate.inc, run as it ships by
//      tests/host_locate_index.cpp) with a one-bit mask.  A round (locate_check_sets): the sets' values gathered on the device
//      (one launch per array), X_S by k_ec_scale and segmented k_g1_pair_sums, one batch normalisation, one download; the
//      three Miller loops with the key's G2 points and the final exponentiation of every set on at most 16 host threads.
// No step after the batch check passes over the proofs of a set again: b bad proofs among N cost <= 2 b ceil(log2 N) checks.

constexpr size_t PS_VERIFY_LOCATE_MAX = (size_t)1 << 20;  // the F tree is 1 344 B per proof: 1.4 GB here
constexpr size_t PS_LOCATE_ROUND_POINTS = (size_t)1 << 20;  // sets x public inputs one pass of a round scales and sums (two XYZZ buffers: 448 MB)
constexpr unsigned PS_LOCATE_THREADS = 16;
static size_t locate_per_pass(size_t diff) { return std::max<size_t>(1, PS_LOCATE_ROUND_POINTS / std::max<size_t>(diff, 1)); }  // sets of one pass

// The round helpers of both locators, down to locate_parallel.  k_gather_words on c->stream; an empty gather (PHGR13 rounds
// have them) launches nothing.  No Groth16 gather is empty: count = K >= 1 sets or segments, width W12, WX, 8 or, where
// diff >= 1, a multiple of diff -- the guard holds back no launch there.
static void locate_gather(ps_ctx* c, const void* in, const u32* ix, size_t count, u64 stride, u64 off, size_t width, void* out) {
    if (count * width)
        hipLaunchKernelGGL(k_gather_words, dim3(nblocks(count * width)), dim3(256), 0, c->stream, (const u32*)in, ix, (u32)count, stride, off, (u32)width, (u32*)out);
}

// Regions of c->lc_work one behind the other, each rounded up to 256 bytes: take() is where the next one starts
struct LocateCarve {
    size_t at = 0;
    size_t take(size_t bytes) { return std::exchange(at, at + ((bytes + 255) & ~(size_t)255)); }
    size_t total() const { return at; }
};

// A lap of the wall clock into lc_ms / plc_ms: *ms += the time since *t, which becomes now
static void locate_lap(float* ms, std::chrono::steady_clock::time_point* t) {
    const auto was = std::exchange(*t, std::chrono::steady_clock::now());
    *ms += std::chrono::duration<float, std::milli>(*t - was).count();
}

// The levels of a product tree above level 0, each to its own place: level l at f + f_level_base(off, l, diff)
static void locate_product_levels(ps_ctx* c, pairing_dev::Fp12* f, const u64* size, const u64* off, int nl, size_t diff, u32 simds) {
    for (int l = 0; l + 1 < nl; l++) {
        const u32 lpw = pairing_dev::spread_lanes(size[l + 1], simds);
        hipLaunchKernelGGL(k_f12_product, dim3((unsigned)((size[l + 1] + lpw - 1) / lpw)), dim3(64), 0, c->stream,
                           (const pairing_dev::Fp12*)(f + locate::f_level_base(off, l, diff)), (u32)size[l], lpw, f + locate::f_level_base(off, l + 1, diff));
    }
}

static int locate_miller_levels(ps_ctx* c, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, const pairing_dev::Fp12** res, VbClock* clk) {
    typedef pairing_dev::Fp12 D12;
    u32 simds = 0;
    int rc = ctx_simds(c, &simds);
    if (rc) return rc;
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    const int nl = locate::tree_levels(n, size, off);
    if (c->lc_f12.ensure(sizeof(D12) * off[nl]))
        return fail(PS_ERR_HIP, "ps_groth16_verify_batch_locate: no device memory for the levels of the product tree (" +
                                    std::to_string(sizeof(D12) * off[nl]) + " bytes for " + std::to_string(n) + " proofs)");
    D12* f = (D12*)c->lc_f12.p;
    const u32 lpw = pairing_dev::spread_lanes(n, simds);
    hipLaunchKernelGGL(k_miller_batch, dim3((unsigned)((n + lpw - 1) / lpw)), dim3(64), 0, c->stream, g1, g2, (u32)n, lpw, f);
    if (clk) clk->mark(2);
    locate_product_levels(c, f, size, off, nl, 0, simds);
    HIP_TRY(hipGetLastError());
    if (clk) clk->mark(3);
    *res = f + off[nl - 1];
    return PS_OK;
}

// fn(i) for i < n on min(n, PS_LOCATE_THREADS) host threads
template <class Fn>
static void locate_parallel(size_t n, Fn fn) {
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < std::min<size_t>(n, PS_LOCATE_THREADS); t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

struct LocateTrees {
    int nl = 0;  // levels, the root is level nl - 1
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    size_t diff = 0;
    const pairing_dev::Fp12* f = nullptr;
    const Xyzz<Fp>* pts = nullptr;
    const u32* rows = nullptr;
    const Xyzz<Fp>* iolp = nullptr;
};

// The C tree, the scalar tree and IoLP in XYZZ form, enqueued on c->stream
static int locate_build_trees(ps_ctx* c, const ps_groth16_vk* vk, const ps_scalars* io, size_t N, const VbKeep& keep, LocateTrees* t) {
    const size_t diff = vk->io_lp->n, cols = diff + 1;
    t->diff = diff;
    t->nl = locate::tree_levels(N, t->size, t->off);
    const u64 nodes = t->off[t->nl];
    if (c->lc_pts.ensure(sizeof(Xyzz<Fp>) * nodes) || c->lc_rows.ensure(32 * cols * nodes) || c->lc_iolp.ensure(sizeof(Xyzz<Fp>) * std::max<size_t>(diff, 1)))
        return fail(PS_ERR_HIP, "ps_groth16_verify_batch_locate: no device memory for the trees (" +
                                    std::to_string((sizeof(Xyzz<Fp>) + 32 * cols) * nodes) + " bytes for " + std::to_string(N) + " proofs of " +
                                    std::to_string(diff) + " public inputs)");
    Xyzz<Fp>* pts = (Xyzz<Fp>*)c->lc_pts.p;
    u32* rows = (u32*)c->lc_rows.p;
    const Fr* rho_m = (const Fr*)c->vb_rho.p;
    hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(N)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(keep.c_pts), (u32)N, (u32)N, pts);
    hipLaunchKernelGGL(k_ec_scale<Fp>, dim3(nblocks(N)), dim3(256), 0, c->stream, pts, (u32)N, rho_m, ~0ull);
    hipLaunchKernelGGL(k_fr_locate_rows, dim3(nblocks(N * cols)), dim3(256), 0, c->stream, scalars_ptr(keep.rho), rho_m, diff ? scalars_ptr(io) : nullptr,
                       (u32)N, (u32)diff, rows);
    for (int l = 0; l + 1 < t->nl; l++) {
        const u64 n = t->size[l], h = t->size[l + 1];
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(h)), dim3(256), 0, c->stream, (const Xyzz<Fp>*)(pts + t->off[l]), (u32)n, 1u, 0u, pts + t->off[l + 1], 0u);
        hipLaunchKernelGGL(k_fr_row_pair_sums, dim3(nblocks(h * cols)), dim3(256), 0, c->stream, (const u32*)(rows + 8 * cols * t->off[l]), (u32)n, (u32)cols,
                           rows + 8 * cols * t->off[l + 1]);
    }
    if (diff)
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(diff)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(vk->io_lp), (u32)diff, (u32)diff,
                           (Xyzz<Fp>*)c->lc_iolp.p);
    HIP_TRY(hipGetLastError());
    t->f = (const pairing_dev::Fp12*)c->lc_f12.p;
    t->pts = pts;
    t->rows = rows;
    t->iolp = (const Xyzz<Fp>*)c->lc_iolp.p;
    return PS_OK;
}

// K sums of `diff` >= 1 scaled points side by side: segment k = scal[k * diff + j] * base[j], j < diff, summed by levels of
// k_g1_pair_sums.  *src and *dst are two buffers of K * diff points; on return the sum of segment k is (*src)[k * diff] (the
// two may have changed places) and *dst is free.  Enqueued on c->stream; K * diff < 2^32 is the caller's.  Shared by the
// descent below (X_S) and by ps_phgr13_verify_batch (the io part of rho_i gv_i, verify_phgr13_batch.inc).
static void segment_sums(ps_ctx* c, const Xyzz<Fp>* base, size_t diff, size_t K, const Fr* scal_mont, Xyzz<Fp>** src, Xyzz<Fp>** dst) {
    constexpr size_t WX = sizeof(Xyzz<Fp>) / 4;
    locate_gather(c, base, nullptr, K, 0, 0, WX * diff, *src);  // base, K times
    hipLaunchKernelGGL(k_ec_scale<Fp>, dim3(nblocks(K * diff)), dim3(256), 0, c->stream, *src, (u32)(K * diff), scal_mont, ~0ull);
    for (size_t n = diff; n > 1; n = (n + 1) / 2) {  // K segments of diff points, the sum of a segment ends in its first slot
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(K * ((n + 1) / 2))), dim3(256), 0, c->stream, (const Xyzz<Fp>*)*src, (u32)n, (u32)K, (u32)diff, *dst,
                           (u32)diff);
        std::swap(*src, *dst);
    }
}

// check(S) for the K nodes idx[] of level l: fail_mask[k] = 1 where it fails, else 0 -- the one-bit mask of locate_bisect
static int locate_check_sets(ps_ctx* c, const LocateTrees& t, const VbKeep& keep, int l, const u32* idx, size_t K, uint8_t* fail_mask) {
    typedef pairing_dev::Fp12 D12;
    constexpr size_t WX = sizeof(Xyzz<Fp>) / 4, W12 = sizeof(D12) / 4;
    const size_t diff = t.diff, cols = diff + 1, pd = std::max<size_t>(diff, 1);
    // one workspace: node indices | F_S | R_S | t_S plain, Montgomery | two buffers of K x diff points | 2K points and their
    // chain products for the normalisation | 2K affine points
    LocateCarve work;
    const size_t o_idx = work.take(4 * K), o_f = work.take(sizeof(D12) * K), o_r = work.take(32 * K), o_t = work.take(32 * K * pd),
                 o_tm = work.take(sizeof(Fr) * K * pd), o_p0 = work.take(sizeof(Xyzz<Fp>) * K * pd), o_p1 = work.take(sizeof(Xyzz<Fp>) * K * pd),
                 o_n = work.take(batch_affine_tmp_bytes(2 * K, sizeof(Xyzz<Fp>))), o_a = work.take(sizeof(Affine<Fp>) * 2 * K), total = work.total();
    if (c->lc_work.ensure(total))
        return fail(PS_ERR_HIP, "ps_groth16_verify_batch_locate: no device memory for a round of " + std::to_string(K) + " sets (" + std::to_string(total) + " bytes)");
    char* w = (char*)c->lc_work.p;
    u32* d_idx = (u32*)(w + o_idx);
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(d_idx, idx, 4 * K, hipMemcpyHostToDevice, c->stream));
    const u32* rows = t.rows + 8 * cols * t.off[l];
    locate_gather(c, t.f + t.off[l], d_idx, K, W12, 0, W12, w + o_f);
    locate_gather(c, rows, d_idx, K, 8 * cols, 0, 8, w + o_r);
    Xyzz<Fp>* norm = (Xyzz<Fp>*)(w + o_n);
    if (diff) {
        locate_gather(c, rows, d_idx, K, 8 * cols, 8, 8 * diff, w + o_t);
        hipLaunchKernelGGL(k_fr_to_mont, dim3(nblocks(K * diff)), dim3(256), 0, c->stream, (Fr*)(w + o_tm), (const u32*)(w + o_t), (u64)(K * diff));
        Xyzz<Fp>*src = (Xyzz<Fp>*)(w + o_p0), *dst = (Xyzz<Fp>*)(w + o_p1);
        segment_sums(c, t.iolp, diff, K, (const Fr*)(w + o_tm), &src, &dst);
        locate_gather(c, src, nullptr, K, WX * diff, 0, WX, norm);
    } else {
        HIP_TRY(hipMemsetAsync(norm, 0, sizeof(Xyzz<Fp>) * K, c->stream));  // X_S is the identity (ZZ = 0)
    }
    locate_gather(c, t.pts + t.off[l], d_idx, K, WX, 0, WX, norm + K);
    batch_to_affine<Fp>(c->stream, (char*)norm, 2 * K, w + o_a, (u32)sizeof(Affine<Fp>));
    HIP_TRY(hipGetLastError());
    std::vector<D12> hf(K);
    std::vector<u32> hr(8 * K);
    std::vector<Affine<Fp>> ha(2 * K);
    HIP_TRY(hipMemcpyAsync(hf.data(), w + o_f, sizeof(D12) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hr.data(), w + o_r, 32 * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), w + o_a, sizeof(Affine<Fp>) * 2 * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    locate_lap(&c->lc_ms[1], &t0);
    // the host's share: 3K Miller loops, then K products and final exponentiations
    typedef Affine<Fq> H1;
    std::vector<pairing::Fp12> loops(3 * K);
    locate_parallel(3 * K, [&](size_t j) {
        const size_t k = j / 3, which = j % 3;
        H1 p;
        if (which == 0) {  // R_S alpha
            p.x = f_zero((const Fq*)0);
            p.y = f_zero((const Fq*)0);
            if (!affine_is_identity<Fq>(keep.alpha)) {
                Xyzz<Fq> s = xyzz_mul_scalar<Fq>(xyzz_from_affine<Fq>(keep.alpha.x, keep.alpha.y), &hr[8 * k]);
                if (!xyzz_to_affine<Fq>(s, p.x, p.y)) { p.x = f_zero((const Fq*)0); p.y = f_zero((const Fq*)0); }
            }
        } else {
            p = affine_to_host<Fp>(ha[which == 1 ? k : K + k]);  // X_S, C_S
        }
        loops[j] = pairing::miller(pairing::neg_g1(p), keep.g2[which]);
    });
    locate_parallel(K, [&](size_t k) {
        pairing::Fp12 f = f12_to_host(hf[k]);
        for (int j = 0; j < 3; j++) f = pairing::f12_mul(f, loops[3 * k + j]);
        fail_mask[k] = pairing::f12_eq(pairing::final_exp(f), pairing::f12_one()) ? 0 : 1;
    });
    locate_lap(&c->lc_ms[2], &t0);
    return PS_OK;
}

static int locate_descent(ps_ctx* c, const ps_groth16_vk* vk, const ps_scalars* io, size_t N, const VbKeep& keep, uint8_t* valid, size_t* ninvalid) {
    memset(valid, 1, N);
    ps_verify_locate_info& info = c->lc_info;
    LocateTrees t;
    if (N > 1) {  // (one proof: the root is the leaf, the descent reads no tree)
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = locate_build_trees(c, vk, io, N, keep, &t)) return rc;
        if (c->timing) (void)hipStreamSynchronize(c->stream);
        locate_lap(&c->lc_ms[0], &t0);
    }
    std::vector<u32> leaves;
    std::vector<uint8_t> masks;  // one equation: every failing leaf has mask 1
    auto check = [&](int l, const u32* idx, const uint8_t*, size_t K, uint8_t* fmask) { return locate_check_sets(c, t, keep, l, idx, K, fmask); };
    if (int rc = locate_bisect(N, 1, locate_per_pass(t.diff), check, &leaves, &masks, &info.checks, &info.levels)) return rc;
    for (u32 i : leaves) valid[i] = 0;  // level 0: a failing leaf is an invalid proof
    *ninvalid = info.invalid = (u32)leaves.size();
    return PS_OK;
}

extern "C" int ps_groth16_verify_batch_locate(ps_ctx* c, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t* proofs, size_t nproofs,
                                              const uint8_t* rho_be32, uint8_t* valid, size_t* ninvalid) {
    if (!c || !vk || !io || !ninvalid || !vk->io_lp || (nproofs && (!proofs || !rho_be32 || !valid)))
        return fail(PS_ERR_ARG, "ps_groth16_verify_batch_locate: NULL argument");
    *ninvalid = 0;
    c->lc_info = ps_verify_locate_info{0, 0, 0, 0};
    for (float& v : c->lc_ms) v = 0;
    int ok = 0;
    VbKeep keep;
    int rc = verify_batch_impl(c, "ps_groth16_verify_batch_locate", PS_VERIFY_LOCATE_MAX, "2^20", vk, io, proofs, nproofs, rho_be32, &ok, &keep);
    Scope scope(c->stream);  // what a rejected batch handed over is this call's from here on, on every way out
    scope.in_flight();       // ... and a failed descent leaves a round's copies behind on the stream: wait for them
    *scope.points() = keep.c_pts;
    *scope.scalars() = keep.rho;
    if (rc || nproofs == 0) return rc;
    c->lc_info.checks = 1;
    if (ok) {
        memset(valid, 1, nproofs);
        return scope.finish(PS_OK);
    }
    rc = locate_descent(c, vk, io, nproofs, keep, valid, ninvalid);
    if (rc) *ninvalid = 0;
    return scope.finish(rc);
}

extern "C" int ps_groth16_verify_batch_locate_info(ps_ctx* c, ps_verify_locate_info* out) {
    if (!c || !out) return fail(PS_ERR_ARG, "ps_groth16_verify_batch_locate_info: NULL argument");
    *out = c->lc_info;
    return PS_OK;
}

// Wall clock of the descent of the last ps_groth16_verify_batch_locate on the context: [0] building the C and scalar trees
// (enqueued only, unless ps_ctx_set_timing is on), [1] the rounds' device part (gathers, X_S, normalisation, download, up to
// the synchronisation), [2] their host part (Miller loops, final exponentiations).  Measurement hook, not in the header.
extern "C" int ps_debug_verify_locate_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "ps_debug_verify_locate_ms: NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = c->lc_ms[i];
    return PS_OK;
}
