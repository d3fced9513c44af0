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
// Over a window table (`one` is msm_plan_table's: c and W the table's) a member is ONE bucket set: kc sets, G = kc * NB, the
// same kc * n * W digits, and the same rules on them.
static MsmPlan msm_batch_plan(const ps_ctx* c, const MsmPlan& one, size_t n, size_t kc, int group) {
    MsmPlan pl = one;
    pl.sets = (int)(one.table ? kc : kc * (size_t)one.W);
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

// ps_msm_batch_set_table: when a batch sums over the points' window tables (one bucket set per member, no fold).
//   0  automatic: every array of the call carries a usable table of one window size (table_usable: a table, no forced window,
//      n < 2^26, the scalars' windows within the table's -- msm_plan_checked's rule), a member has at least
//      PS_BATCH_TABLE_MIN_POINTS points, and the plain plan is not cheaper by PS_TABLE_COST_MARGIN per member in the cost
//      model (an int64 witness over a 20-bit table: 2^19 buckets to reduce for four windows -- msm_plan_checked's rule again)
//   1  never (the plain pass)
//   2  wherever the tables are usable
// Returns the tables' window size, 0 for the plain pass.
#ifndef PS_BATCH_TABLE_MIN_POINTS
#define PS_BATCH_TABLE_MIN_POINTS 512  // shorter members have not been measured over tables (PHGR13's lgsi at 2^10 constraints: 1 023 points)
#endif
static int msm_batch_table_window(const ps_ctx* c, const ps_points* const* pts, size_t a, size_t n, int max_bits) {
    if (c->batch_table == 1 || a == 0) return 0;
    for (size_t i = 0; i < a; i++)
        if (!table_usable(c, pts[i], n, max_bits) || pts[i]->st->table_c != pts[0]->st->table_c) return 0;
    const int tc = pts[0]->st->table_c;
    if (c->batch_table == 2) return tc;
    if (n < PS_BATCH_TABLE_MIN_POINTS) return 0;
    const MsmPlan plain = msm_plan(n, max_bits, 0);
    const double cost_plain = (double)n * plain.W * 10.0 + (double)plain.G * 42.0;
    return cost_plain < PS_TABLE_COST_MARGIN * table_plan_cost(n, max_bits, tc) ? 0 : tc;
}

// The two-level sort of msm_sort over the virtual array of kc * n scalars (msm_batch.hpp): member j's n scalars start at
// scalar index j * stride of `scal` (ps_msm_batch: stride == n, the members back to back).
static int msm_batch_sort(MsmWorkspace* ws, const u32* scal, size_t n, size_t stride, size_t kc, int fold_neg, const MsmPlan& pl, bool timed,
                          hipStream_t st) {
    const u64 N = (u64)kc * n;
    const u64 total = (u64)pl.W * N;  // upper bound on entries
    const u64 G = pl.G;
    if (G > SORT_MAX_BUCKETS || total >= (1ull << 31)) return fail(PS_ERR_ARG, "ps_msm_batch: internal: pass outside the sort's limits");
    int rc;
    if ((rc = ws->counts.ensure(4 * G))) return rc;
    if ((rc = ws->offs.ensure(4 * (G + 1)))) return rc;
    if ((rc = ws->keys.ensure(4 * total))) return rc;
    if ((rc = ws->ranks.ensure(4 * total))) return rc;
    if ((rc = ws->vals.ensure(4 * total))) return rc;
    if ((rc = ws->sorted.ensure(4 * total + 4))) return rc;
    if ((rc = ws->coarse.ensure(4 * (4 * (size_t)SORT_MAX_COARSE + 8)))) return rc;
    if (ws->tail_used) HIP_TRY(hipStreamWaitEvent(st, ws->ev_tail_done, 0));  // the last tail still reads offs
    int evi = 0;
#define PS_BATCH_MARK() do { if (timed) HIP_TRY(hipEventRecord(ws->ev[evi++], st)); } while (0)
    PS_BATCH_MARK();  // 0: start
    DigitConst cadd{};
    for (int w = 0; w + 1 < pl.W; w++) {
        int bit = w * pl.c + pl.c - 1;
        if (bit < 256) cadd.w[bit >> 5] |= 1u << (bit & 31);
    }
    int fb = 5;  // fine bits: as few as keep the coarse bins within SORT_MAX_COARSE
    while (((G + (1ull << fb) - 1) >> fb) > SORT_MAX_COARSE) fb++;
    const u32 ncoarse = (u32)((G + (1ull << fb) - 1) >> fb);
    u32* coarse_cnt = (u32*)ws->coarse.p;
    u32* coarse_off = coarse_cnt + SORT_MAX_COARSE + 1;
    u32* coarse_cur = coarse_off + SORT_MAX_COARSE + 1;
    u32* tile_base = coarse_cur + SORT_MAX_COARSE + 1;
    HIP_TRY(hipMemsetAsync(coarse_cnt, 0, 4 * SORT_MAX_COARSE, st));
    const bool may_have_big_bins = total > SORT_BIG;
    if (may_have_big_bins) HIP_TRY(hipMemsetAsync(ws->counts.p, 0, 4 * G, st));
    const dim3 cgrid((unsigned)((N + (size_t)COUNT_PER_THREAD * DIGITS_THREADS - 1) / ((size_t)COUNT_PER_THREAD * DIGITS_THREADS)));
    const dim3 dgrid((unsigned)((N + DIGITS_CHUNK - 1) / DIGITS_CHUNK), (unsigned)pl.W);
    // over a window table the key is member * NB + digit and the entry names its window (msm_batch.hpp)
    const auto k_count = pl.table ? k_sort_count_batch_tab : k_sort_count_batch;
    const auto k_partition = pl.table ? k_sort_partition_batch_tab : k_sort_partition_batch;
    hipLaunchKernelGGL(k_count, cgrid, dim3(DIGITS_THREADS), 0, st, scal, (u32)n, (u32)stride, (u32)N,
                       pl.c, pl.W, pl.NB, cadd, fold_neg, ncoarse, fb, (u32*)ws->ranks.p, coarse_cnt);
    PS_BATCH_MARK();  // 1: after digits + coarse histogram
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(SORT_MAX_COARSE), 0, st, (const u32*)coarse_cnt, ncoarse, coarse_off, coarse_cur,
                       (u32*)ws->offs.p + G, tile_base);
    hipLaunchKernelGGL(k_partition, dgrid, dim3(DIGITS_THREADS), 2 * DIGITS_CHUNK * sizeof(u32), st,
                       (const u32*)ws->ranks.p, (u32)n, (u32)N, pl.W, pl.NB, fb, coarse_cur, (unsigned short*)ws->keys.p, (u32*)ws->vals.p);
    PS_BATCH_MARK();  // 2: after scan + partition
    hipLaunchKernelGGL(k_sort_fine, dim3(ncoarse), dim3(SORT_FINE), 0, st, (const unsigned short*)ws->keys.p, (const u32*)ws->vals.p,
                       (const u32*)coarse_off, (u32)G, fb, (u32*)ws->offs.p, (u32*)ws->sorted.p);
    if (may_have_big_bins) {
        const unsigned big_grid = (unsigned)std::min<u64>(2048, total / SORT_TILE + 1);
        hipLaunchKernelGGL(k_sort_big_count, dim3(big_grid), dim3(SORT_FINE), 0, st, (const unsigned short*)ws->keys.p, (const u32*)coarse_off,
                           (const u32*)tile_base, ncoarse, fb, (u32*)ws->counts.p);
        hipLaunchKernelGGL(k_sort_big_scan, dim3(ncoarse), dim3(SORT_FINE), 0, st, (const u32*)coarse_off, (u32)G, fb, (u32*)ws->counts.p,
                           (u32*)ws->offs.p);
        hipLaunchKernelGGL(k_sort_big_scatter, dim3(big_grid), dim3(SORT_FINE), 0, st, (const unsigned short*)ws->keys.p,
                           (const u32*)ws->vals.p, (const u32*)coarse_off, (const u32*)tile_base, ncoarse, fb, (u32*)ws->counts.p,
                           (u32*)ws->sorted.p);
    }
    PS_BATCH_MARK();  // 3: after the fine sort
#undef PS_BATCH_MARK
    HIP_TRY(hipGetLastError());
    return PS_OK;
}

// Where a workspace keeps what one pass leaves in its mb_out: the affine sums of the array it is working on (read by the
// encoding only), then one slot of wire bytes per array it serves in this pass -- a workspace that serves several arrays
// (more arrays than workspaces) keeps every array's bytes until the copies at the end of the pass.
struct BatchOut { size_t affine_bytes, slot_bytes; };

// One array's share of a pass: the point pass over the sort that the context `c` owns (sorted / offs), the fold per member
// (plain pass; over a window table the set sums ARE the members' sums), the normalisation and the encoding -- all on workspace
// rw's stream and in rw's buffers (rw == c: ps_msm_batch).  The kc * wb wire bytes are left in slot `slot` of rw->mb_out.
template <class F>
static int msm_batch_points(ps_ctx* c, MsmWorkspace* rw, const ps_points* pts, size_t n, size_t kc, const MsmPlan& pl, bool timed,
                            const BatchOut& lay, size_t slot) {
    typedef typename KernelField<F>::type KF;
    constexpr unsigned LN = FieldTraits<KF>::LANES;
    hipStream_t st = rw->stream;
    int rc;
    Xyzz<F>* dsets = nullptr;
    if ((rc = msm_points_t<F>(c, rw, pts, kc * n, pl, timed, 0, nullptr, nullptr, true, &dsets, n))) return rc;
    if (timed) {
        for (auto& e : c->mb_ev) if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(c->mb_ev[0], st));
    }
    if (pl.table) {
        // batch_to_affine with the points where k_reduce_weights left them; mb_fold holds the chain products alone
        const u32 T = (u32)std::min<size_t>(65536, std::max<size_t>(1, kc / 16));
        hipLaunchKernelGGL(k_batch_to_affine<F>, dim3(nblocks(T)), dim3(256), 0, st, (const Xyzz<F>*)dsets, (u32)kc, T, (Fp*)rw->mb_fold.p,
                           (char*)rw->mb_out.p, (u32)sizeof(Affine<F>));
    } else {
        hipLaunchKernelGGL(k_batch_fold<KF>, dim3(nblocks(kc * LN)), dim3(256), 0, st, (const Xyzz<F>*)dsets, (u32)kc, pl.W, pl.c,
                           (Xyzz<F>*)rw->mb_fold.p);
        batch_to_affine<F>(st, (char*)rw->mb_fold.p, kc, (char*)rw->mb_out.p, (u32)sizeof(Affine<F>));
    }
    uint8_t* d_bytes = (uint8_t*)rw->mb_out.p + lay.affine_bytes + slot * lay.slot_bytes;
    if (pts->group == PS_G1)
        hipLaunchKernelGGL(k_points_to_bytes_g1, dim3(nblocks(kc)), dim3(256), 0, st, (const Affine<Fp>*)rw->mb_out.p, (u32)kc, d_bytes);
    else
        hipLaunchKernelGGL(k_points_to_bytes_g2, dim3(nblocks(kc)), dim3(256), 0, st, (const Affine<Fp2>*)rw->mb_out.p, (u32)kc, d_bytes);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(c->mb_ev[1], st));
    return PS_OK;
}

// The workspaces a call over `a` arrays uses: ring[i % PS_MULTI_RING] serves array i, the first min(a, PS_MULTI_RING) entries
// are distinct (msm_multi_ring).
static inline size_t msm_batch_used(size_t a) { return std::min<size_t>(a, PS_MULTI_RING); }

// One pass: members [first, first + kc) of the batch, for every array.  ONE sort on the context stream over the strided
// source (`scal`: the first scalar of member 0), then per array msm_batch_points on its workspace -- the folds of different
// arrays (serial chains of ~250 doublings) sit on different streams and run side by side; a workspace that serves a second
// array takes it up behind its own fold, in stream order.  Every array's launches are enqueued before the first copy: a
// copy to pageable memory holds the host until its stream has drained.  The caller synchronises behind the last pass.
static int msm_batch_pass(ps_ctx* c, MsmWorkspace* const* ring, const ps_points* const* pts, size_t a, const u32* scal, size_t n, size_t stride,
                          size_t first, size_t kc, int fold_neg, const MsmPlan& one, int plan_group, uint8_t* const* out) {
    const MsmPlan pl = msm_batch_plan(c, one, n, kc, plan_group);
    const size_t used = msm_batch_used(a);
    const bool timed = c->timing && a == 1;  // stage events describe one array's pass
    hipStream_t st = c->stream;
    int rc;
    // buffers of every workspace, sized for the largest group it serves, before anything is enqueued
    BatchOut lay{0, 0};
    size_t xyzz = 0;
    for (size_t i = 0; i < a; i++) {
        const bool g1 = pts[i]->group == PS_G1;
        lay.affine_bytes = std::max(lay.affine_bytes, kc * (g1 ? sizeof(Affine<Fp>) : sizeof(Affine<Fp2>)));
        lay.slot_bytes = std::max(lay.slot_bytes, kc * wire_bytes(pts[i]->group));
        xyzz = std::max(xyzz, g1 ? sizeof(Xyzz<Fp>) : sizeof(Xyzz<Fp2>));
    }
    for (size_t j = 0; j < used; j++) {
        const size_t slots = (a - j + PS_MULTI_RING - 1) / PS_MULTI_RING;  // arrays j, j + ring, ...
        if ((rc = ring[j]->mb_fold.ensure(batch_affine_tmp_bytes(kc, xyzz)))) return rc;
        if ((rc = ring[j]->mb_out.ensure(lay.affine_bytes + slots * lay.slot_bytes))) return rc;
    }
    // the point passes of the pass before, on the other workspaces, still read sorted / offs (the context's own: msm_batch_sort)
    for (size_t j = 0; j < used; j++)
        if (ring[j] != c && ring[j]->tail_used) HIP_TRY(hipStreamWaitEvent(st, ring[j]->ev_tail_done, 0));
    if ((rc = msm_batch_sort(c, scal + 8 * first * stride, n, stride, kc, fold_neg, pl, timed, st))) return rc;
    if (used > 1) {
        if (!c->ev_sorted) HIP_TRY(hipEventCreateWithFlags(&c->ev_sorted, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->ev_sorted, st));
        for (size_t j = 0; j < used; j++)
            if (ring[j] != c) HIP_TRY(hipStreamWaitEvent(ring[j]->stream, c->ev_sorted, 0));
    }
    for (size_t i = 0; i < a; i++) {
        MsmWorkspace* rw = ring[i % PS_MULTI_RING];
        rc = pts[i]->group == PS_G1 ? msm_batch_points<Fp>(c, rw, pts[i], n, kc, pl, timed, lay, i / PS_MULTI_RING)
                                    : msm_batch_points<Fp2>(c, rw, pts[i], n, kc, pl, timed, lay, i / PS_MULTI_RING);
        if (rc) return rc;
    }
    c->ev_valid = timed;
    c->last_timed = c;
    for (size_t i = 0; i < a; i++) {
        MsmWorkspace* rw = ring[i % PS_MULTI_RING];
        const size_t wb = wire_bytes(pts[i]->group);
        const uint8_t* d_bytes = (const uint8_t*)rw->mb_out.p + lay.affine_bytes + (i / PS_MULTI_RING) * lay.slot_bytes;
        HIP_TRY(hipMemcpyAsync(out[i] + first * wb, d_bytes, kc * wb, hipMemcpyDeviceToHost, rw->stream));
    }
    // the results of this pass are read and the tails' buffers free before the next pass reuses them (same streams), and the
    // workspaces' other users order themselves behind ev_tail_done as behind any sum
    for (size_t j = 0; j < used; j++) HIP_TRY(hipEventRecord(ring[j]->ev_tail_done, ring[j]->stream));
    c->last_info = ps_msm_info{pl.c, pl.W, 0, pl.G, pl.M, pl.table ? 1 : 0};
    return PS_OK;
}

// every workspace the call used is idle when it returns, whatever happened: the next call on the context starts clean
static int msm_batch_drain(MsmWorkspace* const* ring, size_t a) {
    hipError_t first = hipSuccess;
    for (size_t j = 0; j < msm_batch_used(a); j++) {
        const hipError_t e = hipStreamSynchronize(ring[j]->stream);
        if (first == hipSuccess) first = e;
    }
    if (first != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_msm_batch: hipStreamSynchronize: ") + hipGetErrorString(first));
    return PS_OK;
}

// k members of n scalars each (member j at scalar index j * stride + first of `sc`) over `a` arrays of n points; the caller has
// checked every length.  ps_msm_batch is a == 1 on the context's own workspace.
static int msm_batch_run(ps_ctx* c, const ps_points* const* pts, size_t a, const ps_scalars* sc, size_t k, size_t stride, size_t first,
                         uint8_t* const* out) {
    const size_t n = pts[0]->n;
    bool any_g1 = false, any_g2 = false;
    for (size_t i = 0; i < a; i++) (pts[i]->group == PS_G1 ? any_g1 : any_g2) = true;
    const int plan_group = any_g2 ? PS_G2 : PS_G1;  // the tail is sized for the group whose points take more lanes (msm_plan_checked)
    HIP_TRY(hipSetDevice(c->device));
    const u64 pb = batch_multi_point_bytes(any_g1, any_g2, sizeof(Xyzz<Fp>), sizeof(Xyzz<Fp2>));
    const u64 min_slice = (u64)(c->forced_slice ? c->forced_slice : 2);
    std::vector<BatchPass> passes;
    MsmPlan one{};
    bool fits = false;
    // over the tables where the route is admitted; a table whose window leaves no room for even one member in a pass (22 bits:
    // 2^21 buckets) falls through to the plain route
    if (const int tc = msm_batch_table_window(c, pts, a, n, sc->max_bits)) {
        one = msm_plan_table(n, sc->max_bits, tc);
        const BatchShape shape{(u64)n, (u64)one.W, (u64)one.NB, pb, min_slice, 1};
        fits = batch_multi_passes((u64)k, shape, msm_batch_limits(c), (u64)stride, &passes);
    }
    if (!fits) {
        one = msm_plan(n, sc->max_bits, c->forced_c);
        const BatchShape shape{(u64)n, (u64)one.W, (u64)one.NB, pb, min_slice};
        fits = batch_multi_passes((u64)k, shape, msm_batch_limits(c), (u64)stride, &passes);
    }
    if (!fits) {
        // not even one member fits a plain pass (n * W >= 2^31, or a forced window whose W * NB buckets exceed the sort's): one by one
        for (size_t i = 0; i < a; i++)
            for (size_t j = 0; j < k; j++) {
                Scope scope;
                ps_scalars** sl = scope.scalars();
                int rc = ps_scalars_slice(sc, j * stride + first, n, sl);
                if (!rc) rc = ps_msm(c, pts[i], *sl, out[i] + j * wire_bytes(pts[i]->group));
                if (rc) return rc;
            }
        return PS_OK;
    }
    MsmWorkspace* ring[PS_MULTI_RING];
    int rc = msm_multi_ring(c, true, a, ring);
    if (rc) return rc;
    if (storage_wait_ready(sc->st, c->stream)) return fail(PS_ERR_HIP, "ps_msm_batch: event wait failed");  // asynchronously produced scalars
    for (const BatchPass& p : passes)
        if ((rc = msm_batch_pass(c, ring, pts, a, scalars_ptr(sc) + 8 * first, n, stride, (size_t)p.first, (size_t)p.count, sc->neg_small ? 1 : 0,
                                 one, plan_group, out)))
            break;
    if (rc) {
        KeepError keep;
        (void)msm_batch_drain(ring, a);
        return rc;
    }
    return msm_batch_drain(ring, a);
}

extern "C" int ps_msm_batch_set_chunk(ps_ctx* c, int members) {
    if (!c || members < 0) return fail(PS_ERR_ARG, "ps_msm_batch_set_chunk: members per pass must be 0 (automatic) or positive");
    c->batch_chunk = members;
    return PS_OK;
}

extern "C" int ps_msm_batch_set_table(ps_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2)
        return fail(PS_ERR_ARG, "ps_msm_batch_set_table: mode must be 0 (automatic), 1 (never over window tables) or 2 (wherever a table is usable)");
    c->batch_table = mode;
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
    return msm_batch_run(c, &pts, 1, sc, k, n, 0, &out);
}

extern "C" int ps_msm_batch_multi(ps_ctx* c, const ps_points* const* pts, size_t a, const ps_scalars* sc, size_t k, size_t stride, size_t first,
                                  uint8_t* const* out) {
    if (!c || !sc || (a && (!pts || !out))) return fail(PS_ERR_ARG, "ps_msm_batch_multi: NULL argument");
    if (a > PS_MSM_MULTI_MAX) return fail(PS_ERR_ARG, "ps_msm_batch_multi: more than PS_MSM_MULTI_MAX point arrays");
    for (size_t i = 0; i < a; i++)
        if (!pts[i] || (k && !out[i])) return fail(PS_ERR_ARG, "ps_msm_batch_multi: NULL argument");
    if (c->q_len) return fail(PS_ERR_ARG, "ps_msm_batch_multi: sums are pending on this context (ps_msm_finish them first)");
    if (a == 0) return PS_OK;
    const size_t n = pts[0]->n;
    for (size_t i = 1; i < a; i++)
        if (pts[i]->n != n)  // algebra.go:350-352
            return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(n) + " and blinded eval points " +
                                           std::to_string(pts[i]->n));
    if (first > stride || n > stride - first)
        return fail(PS_ERR_LENGTH, "ps_msm_batch_multi: a member's range [" + std::to_string(first) + ", +" + std::to_string(n) +
                                       ") does not lie within the stride " + std::to_string(stride));
    if ((stride && k > (size_t)-1 / stride) || sc->n != k * stride)
        return fail(PS_ERR_LENGTH, "mismatch of length between " + std::to_string(k) + " polys of stride " + std::to_string(stride) + " and " +
                                       std::to_string(sc->n) + " scalars");
    if (k == 0) return PS_OK;
    if (n == 0) {
        for (size_t i = 0; i < a; i++)
            for (size_t j = 0; j < k; j++) write_identity(pts[i]->group, out[i] + j * wire_bytes(pts[i]->group));
        return PS_OK;
    }
    return msm_batch_run(c, pts, a, sc, k, stride, first, out);
}

// Measurement hook (tools/prove_batch_sweep.py; not in the header).  Of the last timed call on the context (ps_ctx_set_timing):
// ms[0] the fold (plain pass only), normalisation and encoding of the last pass of the last ps_msm_batch; of the last ps_groth16_prove_batch
// ms[1] wire values + gate check + scalar rows, ms[2] the h values, ms[3..5] the sums B, A, C.  Stages that did not run: -1.
extern "C" int ps_debug_batch_stage_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    for (int i = 0; i < 6; i++) ms[i] = -1.f;
    if (c->mb_ev[0] && c->mb_ev[1] && c->ev_valid) HIP_TRY(hipEventElapsedTime(&ms[0], c->mb_ev[0], c->mb_ev[1]));
    if (c->pb_timed) {
        HIP_TRY(hipEventSynchronize(c->pb_ev[5]));  // recorded behind the call's last synchronisation
        for (int i = 0; i < 5; i++) HIP_TRY(hipEventElapsedTime(&ms[1 + i], c->pb_ev[i], c->pb_ev[i + 1]));
    }
    return PS_OK;
}
