// ps_msm_batch: K scalar vectors over one point array (msm_batch.hpp: the kernels; msm_batch_plan.hpp: the passes).
// Included by capi.hip behind the MSM driver.

// Limits of one pass (msm_batch_plan.hpp).  Bytes: the bucket array and the partial slots of a pass, 4 GiB -- a pass that
// large holds tens of millions of digits and fills the chip many times over; more members per pass buy nothing.
#ifndef PS_BATCH_MAX_BYTES
#define PS_BATCH_MAX_BYTES (4ull << 30)
#endif
constexpr u64 PS_BATCH_MAX_SETS = 1ull << 16;
static BatchLimits msm_batch_limits(const ps_ctx* c) {
    return BatchLimits{SORT_MAX_BUCKETS, 1ull << 31, PS_BATCH_MAX_BYTES, PS_BATCH_MAX_SETS, (u64)c->batch_chunk};
}

// Plan of a pass of kc members.  The window c (hence W, NB) is the cost model's for ONE member's n (msm_plan: the per-member
// cost is the same kc times over; ps_msm_set_window is honoured there).  Everything behind the sort is planned as ONE plain
// sum of kc * n scalars over kc * W bucket sets, by the rules a single sum of that size gets:
//   slices    msm_plan's rule on the pass's digits kc * n * W and buckets G = kc * W * NB (32 entries; longer while more
//             than 2^19 threads or an average bucket spans more than five slices; shorter below 2^17 threads)
//   qtail     G <= 2^16: the reduction by rows / columns / bits of the buckets themselves
//   hybrid    otherwise the 8-bucket running sums with quads behind them (k_reduce_small when NB <= 1024)
//   shortsum  kc * n * W < PS_QTAIL_MAX_ENTRIES: slices as short as keep one wave per SIMD busy, and
//   lpb       msm_plan_lpb's quads per cut bucket for that G (0, the one-lane k_fixup, from G * 4 (G1) / 8 (G2) > 2^17)
// all through msm_plan_tail / msm_plan_lpb with n := kc * n; ps_msm_set_tail and ps_msm_set_slice apply as to a single sum.
// No window table: a table forces one bucket set and tags the window into the entry.
static MsmPlan msm_batch_plan(const ps_ctx* c, const MsmPlan& one, size_t n, size_t kc, int group) {
    MsmPlan pl = one;
    pl.table = false;
    pl.sets = (int)(kc * (size_t)one.W);
    pl.G = (u64)pl.sets * pl.NB;
    const u64 total = (u64)kc * n * (u64)pl.W;
    pl.M = 32;
    while (pl.M < 1024 && total / (2 * (u64)pl.M) >= (1u << 19)) pl.M *= 2;
    while (pl.M < 1024 && (u64)pl.M * 5 * pl.G < total) pl.M *= 2;
    while (pl.M > 8 && total / (u64)pl.M < (1u << 17) && (u64)(pl.M / 2) * 5 * pl.G >= total) pl.M /= 2;
    msm_plan_tail(pl, kc * n, group, c->forced_tail, false);
    if (c->forced_slice) pl.M = c->forced_slice;
    if (pl.shortsum) msm_plan_lpb(pl, kc * n, group);
    return pl;
}

// The two-level sort of msm_sort over the virtual array of kc * n scalars starting at `scal` (msm_batch.hpp).
static int msm_batch_sort(ps_ctx* c, const u32* scal, size_t n, size_t kc, int fold_neg, const MsmPlan& pl, bool timed, hipStream_t st) {
    const u64 N = (u64)kc * n;
    const u64 total = (u64)pl.W * N;  // upper bound on entries
    const u64 G = pl.G;
    if (G > SORT_MAX_BUCKETS || total >= (1ull << 31)) return fail(PS_ERR_ARG, "ps_msm_batch: internal: pass outside the sort's limits");
    int rc;
    if ((rc = c->counts.ensure(4 * G))) return rc;
    if ((rc = c->offs.ensure(4 * (G + 1)))) return rc;
    if ((rc = c->keys.ensure(4 * total))) return rc;
    if ((rc = c->ranks.ensure(4 * total))) return rc;
    if ((rc = c->vals.ensure(4 * total))) return rc;
    if ((rc = c->sorted.ensure(4 * total + 4))) return rc;
    if ((rc = c->coarse.ensure(4 * (4 * (size_t)SORT_MAX_COARSE + 8)))) return rc;
    if (c->tail_used) HIP_TRY(hipStreamWaitEvent(st, c->ev_tail_done, 0));  // the last tail still reads offs
    int evi = 0;
#define PS_BATCH_MARK() do { if (timed) HIP_TRY(hipEventRecord(c->ev[evi++], st)); } while (0)
    PS_BATCH_MARK();  // 0: start
    DigitConst cadd{};
    for (int w = 0; w + 1 < pl.W; w++) {
        int bit = w * pl.c + pl.c - 1;
        if (bit < 256) cadd.w[bit >> 5] |= 1u << (bit & 31);
    }
    int fb = 5;  // fine bits: as few as keep the coarse bins within SORT_MAX_COARSE
    while (((G + (1ull << fb) - 1) >> fb) > SORT_MAX_COARSE) fb++;
    const u32 ncoarse = (u32)((G + (1ull << fb) - 1) >> fb);
    u32* coarse_cnt = (u32*)c->coarse.p;
    u32* coarse_off = coarse_cnt + SORT_MAX_COARSE + 1;
    u32* coarse_cur = coarse_off + SORT_MAX_COARSE + 1;
    u32* tile_base = coarse_cur + SORT_MAX_COARSE + 1;
    HIP_TRY(hipMemsetAsync(coarse_cnt, 0, 4 * SORT_MAX_COARSE, st));
    const bool may_have_big_bins = total > SORT_BIG;
    if (may_have_big_bins) HIP_TRY(hipMemsetAsync(c->counts.p, 0, 4 * G, st));
    const dim3 cgrid((unsigned)((N + (size_t)COUNT_PER_THREAD * DIGITS_THREADS - 1) / ((size_t)COUNT_PER_THREAD * DIGITS_THREADS)));
    const dim3 dgrid((unsigned)((N + DIGITS_CHUNK - 1) / DIGITS_CHUNK), (unsigned)pl.W);
    hipLaunchKernelGGL(k_sort_count_batch, cgrid, dim3(DIGITS_THREADS), 0, st, scal, (u32)n, (u32)N, pl.c, pl.W, pl.NB, cadd, fold_neg, ncoarse, fb,
                       (u32*)c->ranks.p, coarse_cnt);
    PS_BATCH_MARK();  // 1: after digits + coarse histogram
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(SORT_MAX_COARSE), 0, st, (const u32*)coarse_cnt, ncoarse, coarse_off, coarse_cur,
                       (u32*)c->offs.p + G, tile_base);
    hipLaunchKernelGGL(k_sort_partition_batch, dgrid, dim3(DIGITS_THREADS), 2 * DIGITS_CHUNK * sizeof(u32), st, (const u32*)c->ranks.p, (u32)n,
                       (u32)N, pl.W, pl.NB, fb, coarse_cur, (unsigned short*)c->keys.p, (u32*)c->vals.p);
    PS_BATCH_MARK();  // 2: after scan + partition
    hipLaunchKernelGGL(k_sort_fine, dim3(ncoarse), dim3(SORT_FINE), 0, st, (const unsigned short*)c->keys.p, (const u32*)c->vals.p,
                       (const u32*)coarse_off, (u32)G, fb, (u32*)c->offs.p, (u32*)c->sorted.p);
    if (may_have_big_bins) {
        const unsigned big_grid = (unsigned)std::min<u64>(2048, total / SORT_TILE + 1);
        hipLaunchKernelGGL(k_sort_big_count, dim3(big_grid), dim3(SORT_FINE), 0, st, (const unsigned short*)c->keys.p, (const u32*)coarse_off,
                           (const u32*)tile_base, ncoarse, fb, (u32*)c->counts.p);
        hipLaunchKernelGGL(k_sort_big_scan, dim3(ncoarse), dim3(SORT_FINE), 0, st, (const u32*)coarse_off, (u32)G, fb, (u32*)c->counts.p,
                           (u32*)c->offs.p);
        hipLaunchKernelGGL(k_sort_big_scatter, dim3(big_grid), dim3(SORT_FINE), 0, st, (const unsigned short*)c->keys.p,
                           (const u32*)c->vals.p, (const u32*)coarse_off, (const u32*)tile_base, ncoarse, fb, (u32*)c->counts.p,
                           (u32*)c->sorted.p);
    }
    PS_BATCH_MARK();  // 3: after the fine sort
#undef PS_BATCH_MARK
    HIP_TRY(hipGetLastError());
    return PS_OK;
}

// One pass: members [first, first + kc) of `sc`, their wire bytes to out[first ..] -- everything on the context stream; the
// caller synchronises once behind the last pass.
template <class F>
static int msm_batch_pass(ps_ctx* c, const ps_points* pts, const ps_scalars* sc, size_t first, size_t kc, const MsmPlan& one, uint8_t* out) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    const size_t n = pts->n, wb = wire_bytes(pts->group);
    const MsmPlan pl = msm_batch_plan(c, one, n, kc, pts->group);
    hipStream_t st = c->stream;
    int rc;
    if ((rc = msm_batch_sort(c, scalars_ptr(sc) + 8 * first * n, n, kc, sc->neg_small ? 1 : 0, pl, c->timing, st))) return rc;
    Xyzz<F>* dsets = nullptr;
    if ((rc = msm_points_t<F>(c, c, pts, kc * n, pl, c->timing, 0, nullptr, nullptr, true, &dsets))) return rc;
    c->ev_valid = c->timing;
    c->last_timed = c;
    if ((rc = c->mb_fold.ensure(batch_affine_tmp_bytes(kc, sizeof(Xyzz<F>))))) return rc;
    if ((rc = c->mb_out.ensure(kc * (sizeof(Affine<F>) + wb)))) return rc;
    if (c->timing) {
        for (auto& e : c->mb_ev) if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(c->mb_ev[0], st));
    }
    hipLaunchKernelGGL(k_batch_fold<KF>, dim3(nblocks(kc * LN)), dim3(256), 0, st, (const Xyzz<F>*)dsets, (u32)kc, pl.W, pl.c,
                       (Xyzz<F>*)c->mb_fold.p);
    batch_to_affine<F>(c, (char*)c->mb_fold.p, kc, (char*)c->mb_out.p, (u32)sizeof(Affine<F>));
    uint8_t* d_bytes = (uint8_t*)c->mb_out.p + kc * sizeof(Affine<F>);
    if (pts->group == PS_G1)
        hipLaunchKernelGGL(k_points_to_bytes_g1, dim3(nblocks(kc)), dim3(256), 0, st, (const Affine<Fp>*)c->mb_out.p, (u32)kc, d_bytes);
    else
        hipLaunchKernelGGL(k_points_to_bytes_g2, dim3(nblocks(kc)), dim3(256), 0, st, (const Affine<Fp2>*)c->mb_out.p, (u32)kc, d_bytes);
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(c->mb_ev[1], st));
    HIP_TRY(hipMemcpyAsync(out + first * wb, d_bytes, kc * wb, hipMemcpyDeviceToHost, st));
    // the results of this pass are read and the tail's buffers free before the next pass reuses them (same stream), and the
    // context's other users order themselves behind ev_tail_done as behind any sum
    HIP_TRY(hipEventRecord(c->ev_tail_done, st));
    c->last_info = ps_msm_info{pl.c, pl.W, 0, pl.G, pl.M, 0};
    return PS_OK;
}

extern "C" int ps_msm_batch_set_chunk(ps_ctx* c, int members) {
    if (!c || members < 0) return fail(PS_ERR_ARG, "ps_msm_batch_set_chunk: members per pass must be 0 (automatic) or positive");
    c->batch_chunk = members;
    return PS_OK;
}

extern "C" int ps_msm_batch(ps_ctx* c, const ps_points* pts, const ps_scalars* sc, size_t k, uint8_t* out) {
    if (!c || !pts || !sc || (k && !out)) return fail(PS_ERR_ARG, "ps_msm_batch: NULL argument");
    if (c->q_len) return fail(PS_ERR_ARG, "ps_msm_batch: sums are pending on this context (ps_msm_finish them first)");
    const size_t n = pts->n;
    if (sc->n != k * n)  // algebra.go:350-352, k times
        return fail(PS_ERR_LENGTH, "mismatch of length between " + std::to_string(k) + " polys of " + std::to_string(n) +
                                       " blinded eval points and " + std::to_string(sc->n) + " scalars");
    const size_t wb = wire_bytes(pts->group);
    if (k == 0) return PS_OK;
    if (n == 0) {
        for (size_t j = 0; j < k; j++) write_identity(pts->group, out + j * wb);
        return PS_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const MsmPlan one = msm_plan(n, sc->max_bits, c->forced_c);
    const u64 pb = pts->group == PS_G1 ? sizeof(Xyzz<Fp>) : sizeof(Xyzz<Fp2>);
    const BatchShape shape{(u64)n, (u64)one.W, (u64)one.NB, pb, (u64)(c->forced_slice ? c->forced_slice : 2)};
    std::vector<BatchPass> passes;
    if (!batch_passes((u64)k, shape, msm_batch_limits(c), &passes)) {
        // not even one member fits a pass (n * W >= 2^31, or a forced window whose W * NB buckets exceed the sort's): one by one
        for (size_t j = 0; j < k; j++) {
            Scope scope;
            ps_scalars** sl = scope.scalars();
            int rc = ps_scalars_slice(sc, j * n, n, sl);
            if (!rc) rc = ps_msm(c, pts, *sl, out + j * wb);
            if (rc) return rc;
        }
        return PS_OK;
    }
    if (storage_wait_ready(sc->st, c->stream)) return fail(PS_ERR_HIP, "ps_msm_batch: event wait failed");  // asynchronously produced scalars
    int rc = PS_OK;
    for (const BatchPass& p : passes) {
        rc = pts->group == PS_G1 ? msm_batch_pass<Fp>(c, pts, sc, (size_t)p.first, (size_t)p.count, one, out)
                                 : msm_batch_pass<Fp2>(c, pts, sc, (size_t)p.first, (size_t)p.count, one, out);
        if (rc) break;
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PS_OK;
}

// Measurement hook (tools/prove_batch_sweep.py; not in the header).  Of the last timed call on the context (ps_ctx_set_timing):
// ms[0] the fold, normalisation and encoding of the last pass of the last ps_msm_batch; of the last ps_groth16_prove_batch
// ms[1] wire values + gate check + scalar rows, ms[2] the h values, ms[3..5] the sums B, A, C.  Stages that did not run: -1.
extern "C" int ps_debug_batch_stage_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < 6; i++) ms[i] = -1.f;
    if (c->mb_ev[0] && c->mb_ev[1] && c->ev_valid) HIP_TRY(hipEventElapsedTime(&ms[0], c->mb_ev[0], c->mb_ev[1]));
    if (c->pb_timed)
        for (int i = 0; i < 5; i++) HIP_TRY(hipEventElapsedTime(&ms[1 + i], c->pb_ev[i], c->pb_ev[i + 1]));
    return PS_OK;
}
