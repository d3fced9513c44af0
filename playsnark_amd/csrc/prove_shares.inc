// The provers that work over index ranges (included by capi.hip right after prove.inc), and the helpers they share:
//
//   ps_msm_multi_device      one sum over shards that live on several devices of this process
//   ps_phgr13_prove          <- PHGR13Prove (pinochio.go:207-254): the whole key is rank 0 of 1 of the share prover
//   ps_phgr13_prove_shard    one rank's share over the whole key (one process per GPU)
//   ps_phgr13_prove_multi    the devices of one process, each holding only its ranges of the evaluation key
//   ps_groth16_prove_multi   the same for Groth16Prove, over monomial or over Lagrange-form rank-local keys
//   ps_groth16_prove_local   one rank's share over its ranges of a Lagrange-form key (one process per GPU)
//
// Ranges are shard_range_c's (share_ranges.hpp).  ctx_busy, ms_since, SumQueue and g16_weight_ab1 are in prove.inc, which the
// unsharded Groth16 prover shares them with.

// ---------------------------------------------------------------------------------------
// helpers of the drivers that run one host thread per device
// ---------------------------------------------------------------------------------------
// The first error of any device, with its text, and the condition variable on which devices wait for what another device
// produces: data that sits beside the latch, published under its lock.  An error releases every waiter.
namespace {
struct FirstError {
    std::mutex mu;
    std::condition_variable cv;
    int err = PS_OK;
    std::string msg;
    size_t dev = 0;
    // Called on the thread that failed (g_last_error is per thread).  Keeps the first error in time; by_device: that of the
    // lowest-numbered failing device instead -- what a loop over the devices reports, for a driver whose devices never wait.
    void set(int rc, size_t d = 0, bool by_device = false) {
        std::lock_guard<std::mutex> lk(mu);
        if (!err || (by_device && d < dev)) { err = rc; msg = g_last_error; dev = d; }
        cv.notify_all();
    }
    template <class Publish>
    void publish(Publish pub) {
        std::lock_guard<std::mutex> lk(mu);
        pub();
        cv.notify_all();
    }
    // returns once `pred` holds (PS_OK) or a device has failed (that error, as this thread's own)
    template <class Pred>
    int wait(Pred pred) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return err != PS_OK || pred(); });
        return err ? fail(err, msg) : PS_OK;
    }
};
}  // namespace

// work(d) for every device: devices 1.. on threads of their own, device 0 on the caller's; returns when all are done
template <class Work>
static void run_per_device(size_t ndev, const Work& work) {
    std::vector<std::future<void>> jobs;
    for (size_t d = 1; d < ndev; d++) jobs.push_back(std::async(std::launch::async, work, d));
    work(0);
    for (auto& j : jobs) j.get();
}

// device d's context is none of the devices' before it
template <class Dev>
static int require_distinct_contexts(const Dev* dev, size_t d, const char* who) {
    for (size_t e = 0; e < d; e++)
        if (dev[e].ctx == dev[d].ctx) return fail(PS_ERR_ARG, std::string(who) + ": one context per device (a context appears twice)");
    return PS_OK;
}

// Peer access from `dev` to `peer`, asked for once per pair where the hardware allows it.  The copies do not depend on
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

// "my range, from the device that has it": enqueued on `st`, a stream of dst_dev
static int copy_range_from(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
    if (dst_dev == src_dev) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    } else {
        peer_access_once(dst_dev, src_dev);
        HIP_TRY(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
    }
    return PS_OK;
}

// out = the sum over d of the point at parts + d * stride + offset (the devices' parts of one proof element), on the host
static int fold_parts(int group, const void* parts, size_t stride, size_t offset, size_t ndev, uint8_t* out) {
    const size_t wb = wire_bytes(group);
    std::vector<uint8_t> flat(wb * ndev);
    for (size_t d = 0; d < ndev; d++) memcpy(flat.data() + wb * d, (const uint8_t*)parts + stride * d + offset, wb);
    return ps_points_sum(group, flat.data(), ndev, out);
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
    return fold_parts(group, partial.data(), wb, 0, ndev, out);
}

// ---------------------------------------------------------------------------------------
// PHGR13Prove (pinochio.go:207-254), whole and over index ranges: the whole key (ps_phgr13_prove), one rank's share over the
// whole key (ps_phgr13_prove_shard, one process per GPU), and the devices of one process each holding only its ranges
// (ps_phgr13_prove_multi).  The nine computeSolCommit sums (:231-241) share one scalar vector, solution[diff:], so they
// share one digit sort (ps_msm_multi); and since
// gz = sum_k s_k vbs_k + sum_k s_k wbs_k + sum_k s_k ybs_k = sum_k s_k (vbs_k + wbs_k + ybs_k), the three
// beta arrays are summed pointwise once per evaluation key and gz is ONE sum.  Same group elements, hence the same canonical
// bytes, as the reference's statement-by-statement computation.  PHGR13 has no fixed points, so every proof element is the
// sum of the ranks' partial sums.  A share's sums: the seven solution sums (vs, ws, ys, vas, was, yas and the pointwise beta
// sum) and the h(s) sum, each over the share's range.
// ---------------------------------------------------------------------------------------
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

// The window tables of a PHGR13 key, built once whoever asks first (evaluation-key arrays are fixed across proofs; shared
// keys: under the array's lock) and optional: no room for one is no error, the sums over that array take the plain plan.
// Views of these arrays get tables of their own.  The seven solution arrays (the beta sum made: phgr13_beta_sum) ...
static int phgr13_solution_tables(ps_ctx* c, const ps_phgr13_ek* ek) {
    const ps_points* arr[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, c->phgr_bsum};
    int rc = PS_OK;
    for (int i = 0; i < 7 && !rc; i++) rc = points_ensure_table(c, arr[i], 0, true);
    return rc;
}
// ... and hp (gsi or lgsi), from PS_TABLE_MIN_POINTS points on
static int phgr13_h_table(ps_ctx* c, const ps_points* hp) {
    return hp->n >= PS_TABLE_MIN_POINTS ? points_ensure_table(c, hp, 0, true) : PS_OK;
}

// Once per key, for a prover that sums `cnt` (> 0) solution entries over ek's arrays: the beta sum, and the window tables of
// the seven arrays and of hp.
static int phgr13_prepare(ps_ctx* c, const ps_phgr13_ek* ek, size_t cnt, const ps_points* hp) {
    if (!cnt) return PS_OK;
    int rc = phgr13_beta_sum(c, ek);
    if (rc || !tables_wanted(c, cnt)) return rc;
    if ((rc = phgr13_solution_tables(c, ek))) return rc;
    return phgr13_h_table(c, hp);
}

// After quotient_run on c: h[first, first + cnt) as plain limbs into the context's own vector (slot 3: not freed by the
// caller) -- h's coefficients, or with lgsi in the key its values on the nodes n+1..2n-1.  Enqueued on the context stream.
static int phgr13_h_to_vector(ps_ctx* c, const ps_qap* q, bool lag, size_t first, size_t cnt, ps_scalars** h) {
    int rc = prover_vector(c, 3, cnt, h);
    if (rc) return rc;
    if (cnt)
        hipLaunchKernelGGL(k_fr_from_mont, dim3(nblk(cnt)), dim3(256), 0, c->stream, (u32*)(*h)->st->p,
                           (const Fr*)(lag ? q->qt.scratch : q->hbuf) + first, (u64)cnt);
    HIP_TRY(hipGetLastError());
    return PS_OK;
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
// hands over this share's range of h as a vector on the context (a view, into a slot of phgr13_share_sums's scope)
typedef std::function<int(ps_scalars**)> Phgr13GetH;

// The sums of one share on context c.  Order of work (measured at n = 2^20, see groth16_prove_impl): the quotient has run
// first and alone -- its NTT passes and the bucket accumulations are both VALU-bound, sharing the chip only stretches the
// quotient --, then the h(s) sum on the context itself and the seven solution sums (one digit sort) on workers, every
// point pass chained behind the previous one.
// h_first: h is at hand (the quotient ran on this context).  The digit sort of the seven sums first (on a worker stream; no
// fork event: nothing it reads is still being produced), then the h(s) sum -- ghs := hx.BlindEval(zeroG1, ek.gsi),
// pinochio.go:218 -- on the context's own stream, then the seven point passes chained behind its accumulation: a sort that
// has to share the chip with an accumulation waits for CUs (140 KB of LDS per workgroup) and was measured at 1.9 ms instead
// of 0.1.  Otherwise the sort and the seven point passes are launched first and h is awaited behind them; phase [0] is then
// that wait.  Whatever was launched is drained on every path, so that no sum stays pending on c or on its workers and the
// next call on the same context starts clean.
static int phgr13_share_sums(ps_ctx* c, const Phgr13Share& sh, bool h_first, const Phgr13GetH& get_h, ps_phgr13_proof* out) {
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "PHGR13 share: an MSM is pending on this context");
    uint8_t* dst[7] = {out->vss, out->wss, out->yss, out->vass, out->wass, out->yass, out->gz};
    const size_t cnt = sh.sv->n;
    MsmWorkspace* ring[PS_MULTI_RING] = {nullptr, nullptr, nullptr, nullptr};
    MsmPlan mpl{};
    MultiGuess guess;  // the point pass the seven sums are launched with (point_pass_predict.hpp)
    Scope scope;
    ps_scalars** h = scope.scalars();
    bool sums = false, h_launched = false;
    auto t_h = std::chrono::steady_clock::now();
    auto launch_h = [&]() -> int {
        const auto t_wait = std::chrono::steady_clock::now();
        int r2 = get_h(h);
        if (!h_first) {
            c->phase_ms[0] = ms_since(t_wait);
            t_h = std::chrono::steady_clock::now();
            // not chained behind an accumulation of an earlier call's workspace (the point passes above re-recorded them)
            c->last_chain = nullptr;
        }
        if (!r2 && !(r2 = msm_launch_impl(c, sh.hp, *h, true))) h_launched = true;
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
        hipEvent_t after_h = (h_first && (*h)->n && c->last_chain) ? c->last_chain->ev_acc_local : nullptr;
        guess = msm_multi_guess(c, sh.pts, 7, sh.sv, mpl);
        if (!(rc = msm_multi_points(c, ring, sh.pts, 7, sh.sv, mpl, after_h, guess.family))) sums = true;
    }
    if (!rc && !h_first) rc = launch_h();
    if (rc) {  // what is in flight finishes before its buffers can be reused
        for (MsmWorkspace* w : ring) if (w) (void)w->sync();
        (void)c->sync();
    }
    uint8_t dump[96];
    if (h_launched) {
        int r2 = ps_msm_finish(c, rc ? dump : out->hs);
        if (!rc) rc = r2;
    }
    c->phase_ms[1] = ms_since(t_h);
    const auto t_sums = std::chrono::steady_clock::now();
    if (sums) {
        int r2 = msm_multi_finish(c, ring, sh.pts, 7, sh.sv, mpl, guess, rc ? nullptr : dst);
        if (!rc) rc = r2;
    }
    c->phase_ms[2] = ms_since(t_sums);
    if (!rc && !cnt)  // an empty range: every solution sum is the identity
        for (int i = 0; i < 7; i++) write_identity(i == 1 ? PS_G2 : PS_G1, dst[i]);
    return rc;
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
    const size_t diff = q->m - q->nio;  // pinochio.go:219
    // computeSolCommit: acc += solution[diff+i] * evalCommit[i]  (pinochio.go:222-229)
    const size_t nn = ek->vs->n;
    bool same_len = true;
    for (auto* p : arrs)
        if (p != ek->gsi) {
            if (diff + p->n > sol->n) return fail(PS_ERR_LENGTH, "evaluation-key array longer than the non-IO part of the solution");
            same_len = same_len && p->n == nn;
        }
    // h as coefficients over gsi (pinochio.go:209-218), or -- with the Lagrange form of gsi in the key -- as its values on
    // the nodes n+1..2n-1 over lgsi: the same group element without the interpolation
    const ps_points* gsi = ek->lgsi ? ek->lgsi : ek->gsi;
    const bool multi = same_len && nn > 0;  // what NewPHGR13TrustedSetup produces: the share prover, as rank 0 of 1
    int rc = phgr13_prepare(c, ek, multi ? nn : 0, gsi);
    if (rc) return rc;
    if (multi) {  // the workers exist before the quotient runs (a fresh context makes them here, not inside phase 1)
        MsmWorkspace* ring[PS_MULTI_RING];
        if ((rc = msm_multi_ring(c, false, 7, ring))) return rc;
        if (ctx_busy(c)) return fail(PS_ERR_ARG, "ps_phgr13_prove: an MSM is pending on this context");
    }
    if (q->n >= 1 && (ek->gsi->n != q->n - 1 || (ek->lgsi && ek->lgsi->n != q->n - 1)))  // hx.BlindEval(zeroG1, ek.gsi) panics, algebra.go:350-352
        return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(q->n - 1) + " and blinded eval points " +
                                       std::to_string(ek->gsi->n != q->n - 1 ? ek->gsi->n : ek->lgsi->n));
    if (ek->lgsi && ek->lgsi->group != PS_G1) return fail(PS_ERR_ARG, "ps_phgr13_prove: evaluation-key array in the wrong group");
    if ((rc = quotient_run(c, q, sol, ek->lgsi ? Q_H_VALUES : Q_H_ONLY))) return rc;
    ps_scalars* h = nullptr;
    if ((rc = phgr13_h_to_vector(c, q, ek->lgsi != nullptr, 0, q->n - 1, &h))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->phase_ms[0] = ms_since(t_start);
    if (multi) {
        Scope scope;
        ps_scalars** view = scope.scalars();
        if ((rc = ps_scalars_slice(sol, diff, nn, view))) return rc;
        const Phgr13Share sh{{ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, c->phgr_bsum}, *view, gsi};
        rc = phgr13_share_sums(c, sh, true, [&](ps_scalars** o) { return ps_scalars_slice(h, 0, h->n, o); }, out);
        c->phase_ms[3] = ms_since(t_start);
        return rc;
    }
    const auto t_h = std::chrono::steady_clock::now();
    rc = ps_msm(c, gsi, h, out->hs);  // ghs := hx.BlindEval(zeroG1, ek.gsi), pinochio.go:218
    c->phase_ms[1] = ms_since(t_h);
    if (rc) return rc;
    uint8_t* dst[7] = {out->vss, out->wss, out->yss, out->vass, out->wass, out->yass, out->gz};
    if (same_len) {  // nn == 0: every sum is empty
        for (int i = 0; i < 7; i++) write_identity(i == 1 ? PS_G2 : PS_G1, dst[i]);
        return PS_OK;
    }
    // arrays of different lengths (not what NewPHGR13TrustedSetup produces): one sum at a time
    //                          :231     :232 (G2) :233     :234      :235      :236      :239     :240     :241
    const ps_points* one[9] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, ek->vbs, ek->wbs, ek->ybs};
    uint8_t three[3 * 96];
    for (int i = 0; i < 9; i++)
        if ((rc = msm_range(c, one[i], sol, diff, one[i]->n, i < 6 ? dst[i] : three + 96 * (i - 6)))) return rc;
    return ps_points_sum(PS_G1, three, 3, out->gz);  // gz := gvb + (gwb + gyb), pinochio.go:242
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
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "ps_phgr13_prove_shard: an MSM is pending on this context");
    const ps_points* gsi = ek->lgsi ? ek->lgsi : ek->gsi;
    if ((rc = phgr13_prepare(c, ek, nn, gsi))) return rc;  // over the whole arrays, as ps_phgr13_prove
    if ((rc = quotient_run(c, q, sol, ek->lgsi ? Q_H_VALUES : Q_H_ONLY))) return rc;
    size_t fs, cs, fh, ch;
    shard_range_c(nn, rank, world, &fs, &cs);
    shard_range_c(n - 1, rank, world, &fh, &ch);
    ps_scalars* h = nullptr;  // this rank's range of h only
    if ((rc = phgr13_h_to_vector(c, q, ek->lgsi != nullptr, fh, ch, &h))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->phase_ms[0] = ms_since(t_start);
    const ps_points* whole[7] = {ek->vs, ek->ws, ek->ys, ek->vas, ek->was, ek->yas, nn ? c->phgr_bsum : ek->vbs};
    Scope scope;
    ps_points** views[8];  // the seven arrays and gsi over this rank's ranges
    ps_scalars** sv = scope.scalars();
    for (int i = 0; i < 8; i++) views[i] = scope.points();
    for (int i = 0; i < 7; i++)
        if ((rc = ps_points_slice(whole[i], fs, cs, views[i]))) return rc;
    if ((rc = ps_points_slice(gsi, fh, ch, views[7])) || (rc = ps_scalars_slice(sol, diff + fs, cs, sv))) return rc;
    const Phgr13Share sh{{*views[0], *views[1], *views[2], *views[3], *views[4], *views[5], *views[6]}, *sv, *views[7]};
    rc = phgr13_share_sums(c, sh, true, [&](ps_scalars** o) { return ps_scalars_slice(h, 0, ch, o); }, part);
    c->phase_ms[3] = ms_since(t_start);
    return rc;
}

// every array of a rank-local key must be exactly the rank's range (algebra.go:350-352 otherwise)
static bool phgr13_holds_ranges(const ps_phgr13_ek& ek, size_t n, size_t nn, int rank, int world) {
    size_t f, cs, ch;
    shard_range_c(nn, rank, world, &f, &cs);
    shard_range_c(n - 1, rank, world, &f, &ch);
    bool ok = ek.gsi->n == ch && (!ek.lgsi || ek.lgsi->n == ch);
    for (const ps_points* p : {ek.vs, ek.ws, ek.ys, ek.vas, ek.was, ek.yas, ek.vbs, ek.wbs, ek.ybs}) ok = ok && p->n == cs;
    return ok;
}

// PHGR13Prove over `ndev` devices of this process, every device holding only its index ranges of the evaluation key.  The
// quotient runs ONCE, on dev[0], alone, and leaves h, plain limbs, in dev[0]'s context vector; an event recorded behind that
// conversion is the only thing the other devices wait for.  Devices 1.. launch their digit sort and seven point passes at
// once, then wait for h on the host (released with h, or with the first error of any device), make their stream wait for the
// event and copy their range of h device to device into their own context vector -- no byte of h crosses host memory, no
// upload, no allocation once the contexts are warm -- and launch the h(s) sum.  The partial proofs are folded on the host.
extern "C" int ps_phgr13_prove_multi(const ps_phgr13_device* dev, size_t ndev, ps_phgr13_proof* out) {
    if (!dev || ndev == 0 || !out) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: NULL argument");
    if (ndev > 64) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: at most 64 devices");
    int rc;
    for (size_t d = 0; d < ndev; d++) {
        if (!dev[d].ctx || !dev[d].qap || !dev[d].sol) return fail(PS_ERR_ARG, "ps_phgr13_prove_multi: NULL handle");
        if ((rc = phgr13_check_arrays(&dev[d].ek, "ps_phgr13_prove_multi"))) return rc;
        if ((rc = require_distinct_contexts(dev, d, "ps_phgr13_prove_multi"))) return rc;
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
    for (size_t d = 0; d < ndev; d++)
        if (!phgr13_holds_ranges(dev[d].ek, n, nn, (int)d, (int)ndev) || dev[d].qap->n != n || dev[d].qap->m != m || dev[d].sol->n != m)
            return fail(PS_ERR_LENGTH, "ps_phgr13_prove_multi: device " + std::to_string(d) + " does not hold its index range of the evaluation-key arrays");
    ps_ctx* const c0 = dev[0].ctx;
    FirstError ho;
    ps_scalars* h0 = nullptr;  // beside the latch: all of h on dev[0], once c0->ev_q is recorded behind it
    std::vector<ps_phgr13_proof> parts(ndev);
    auto work = [&](size_t d) {
        ps_ctx* c = dev[d].ctx;
        const ps_phgr13_ek& ek = dev[d].ek;
        const auto t_start = std::chrono::steady_clock::now();
        int rc = hipSetDevice(c->device) == hipSuccess ? PS_OK : fail(PS_ERR_HIP, "ps_phgr13_prove_multi: hipSetDevice failed");
        Scope scope;  // this thread's, on this device
        size_t fs, cs, fh, ch;
        shard_range_c(nn, (int)d, (int)ndev, &fs, &cs);
        shard_range_c(n - 1, (int)d, (int)ndev, &fh, &ch);
        const ps_points* hp = lag ? ek.lgsi : ek.gsi;
        if (!rc && ctx_busy(c)) rc = fail(PS_ERR_ARG, "ps_phgr13_prove_multi: an MSM is pending on a context");
        if (!rc) rc = phgr13_prepare(c, &ek, cs, hp);  // over the local arrays
        ps_scalars** sv = scope.scalars();
        if (!rc) rc = ps_scalars_slice(dev[d].sol, diff + fs, cs, sv);
        const Phgr13Share sh{{ek.vs, ek.ws, ek.ys, ek.vas, ek.was, ek.yas, cs ? c->phgr_bsum : ek.vbs}, *sv, hp};
        if (d == 0) {
            ps_scalars* h = nullptr;  // all of h: the others copy from it
            if (!rc) rc = quotient_run(c, dev[0].qap, dev[0].sol, lag ? Q_H_VALUES : Q_H_ONLY);
            if (!rc) rc = phgr13_h_to_vector(c, dev[0].qap, lag, 0, n - 1, &h);
            if (!rc) {
                hipError_t e = c->ev_q ? hipSuccess : hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventRecord(c->ev_q, c->stream);
                if (e != hipSuccess) rc = fail(PS_ERR_HIP, std::string("ps_phgr13_prove_multi: h: ") + hipGetErrorString(e));
            }
            if (rc) ho.set(rc);
            else ho.publish([&] { h0 = h; });
            if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(PS_ERR_HIP, "ps_phgr13_prove_multi: quotient: stream synchronisation failed");
            c->phase_ms[0] = ms_since(t_start);
            if (!rc) rc = phgr13_share_sums(c, sh, true, [&](ps_scalars** o) { return ps_scalars_slice(h, fh, ch, o); }, &parts[0]);
        } else if (!rc) {
            auto get_h = [&](ps_scalars** o) -> int {
                int r2 = ho.wait([&] { return h0 != nullptr; });
                if (r2) return r2;
                ps_scalars* hl = nullptr;  // this device's context vector (slot 3): its range of h
                if ((r2 = prover_vector(c, 3, ch, &hl))) return r2;
                HIP_TRY(hipStreamWaitEvent(c->stream, c0->ev_q, 0));
                if (ch && (r2 = copy_range_from(hl->st->p, c->device, scalars_ptr(h0) + 8 * fh, c0->device, 32 * ch, c->stream))) return r2;
                HIP_TRY(hipStreamSynchronize(c->stream));
                return ps_scalars_slice(hl, 0, ch, o);
            };
            rc = phgr13_share_sums(c, sh, false, get_h, &parts[d]);
        }
        if (rc) ho.set(rc);
        c->phase_ms[3] = ms_since(t_start);
    };
    run_per_device(ndev, work);
    if (ho.err) return fail(ho.err, ho.msg);
    const size_t off[8] = {offsetof(ps_phgr13_proof, vss), offsetof(ps_phgr13_proof, vass), offsetof(ps_phgr13_proof, wss),
                           offsetof(ps_phgr13_proof, wass), offsetof(ps_phgr13_proof, yss), offsetof(ps_phgr13_proof, yass),
                           offsetof(ps_phgr13_proof, hs), offsetof(ps_phgr13_proof, gz)};
    rc = PS_OK;
    for (int k = 0; k < 8 && !rc; k++)
        rc = fold_parts(off[k] == offsetof(ps_phgr13_proof, wss) ? PS_G2 : PS_G1, parts.data(), sizeof(ps_phgr13_proof), off[k], ndev,
                        (uint8_t*)out + off[k]);
    return rc;
}

// ---------------------------------------------------------------------------------------
// Groth16Prove (groth16.go:122-211) over rank-local keys: every device (ps_groth16_prove_multi, the devices of one process:
// a Go caller cannot start one process per GPU around a function call) or every rank (ps_groth16_prove_local, one process per
// GPU) holds only ITS index range of the CRS arrays (shard_range: contiguous, sizes differ by at most one).  A share is
//   A_part = a . Xi,   B_part = b . Xi2,   C_part = sol . NioLP + h . XiT + s A_part + r B1'_part,   B1' = b . Xi
// as in the split form of groth16_prove_impl; ONE share also adds the fixed points, and the proof is the sum of the shares.
// ---------------------------------------------------------------------------------------
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

// C_part = N + H + s A_part + r B1'_part (groth16.go:180-205, the fixed points apart)
static int g16_share_c(const uint8_t* N, const uint8_t* H, const uint8_t* A, const uint8_t* B1, const uint8_t* r_be32, const uint8_t* s_be32,
                       uint8_t* C_out) {
    uint8_t three[3 * 96];
    memcpy(three, N, 96); memcpy(three + 96, H, 96);
    int rc = g16_weight_ab1(A, B1, r_be32, s_be32, three + 192);
    if (!rc) rc = ps_points_sum(PS_G1, three, 3, C_out);
    return rc;
}

// every local array must be exactly the rank's range (algebra.go:350-352 otherwise); lag: of the Lagrange-form arrays
static bool g16_holds_ranges(const ps_groth16_pk& pk, bool lag, size_t n, size_t nn, int rank, int world) {
    const ps_points *xi = lag ? pk.lxi : pk.xi, *xi2 = lag ? pk.lxi2 : pk.xi2, *xi_t = lag ? pk.lxi_t : pk.xi_t;
    size_t f, cn, ch, cq;
    shard_range_c(n, rank, world, &f, &cn);
    shard_range_c(n - 1, rank, world, &f, &ch);
    shard_range_c(nn, rank, world, &f, &cq);
    return xi->n == cn && xi2->n == cn && xi_t->n == ch && pk.nio_lp->n == cq;
}

// the devices' shares of a proof, folded on the host
namespace {
struct G16Part { uint8_t A[96], B[192], C[96]; };
}
static int g16_fold_parts(const std::vector<G16Part>& parts, uint8_t* A_out, uint8_t* B_out, uint8_t* C_out) {
    int rc = fold_parts(PS_G1, parts.data(), sizeof(G16Part), offsetof(G16Part, A), parts.size(), A_out);
    if (!rc) rc = fold_parts(PS_G2, parts.data(), sizeof(G16Part), offsetof(G16Part, B), parts.size(), B_out);
    if (!rc) rc = fold_parts(PS_G1, parts.data(), sizeof(G16Part), offsetof(G16Part, C), parts.size(), C_out);
    return rc;
}

// The five sums of a share, as SumQueue kinds (and in the order of their launch: the G2 sum, the longest point pass, first)
enum { G16_B = 0, G16_A = 1, G16_B1 = 2, G16_N = 3, G16_H = 4 };

// ---- Lagrange-form keys ----
// With lxi / lxi2 in the key the scalars of A, B and B1' are the wire values a_j = (L.s)_j, b_j = (R.s)_j, so a device that
// holds lxi[range] and lxi2[range] gets exactly the scalars it needs from its OWN rows of the three sparse products
// (k_own_rows): those three sums need no exchange at all.  Only the n-1 values h(n+k) depend on the whole circuit.
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
    if (ctx_busy(c)) return fail(PS_ERR_ARG, "Groth16 share: an MSM is pending on this context");
    HIP_TRY(hipSetDevice(c->device));
    const auto t_start = std::chrono::steady_clock::now();
    int rc = PS_OK;
    // window tables over the local arrays, once per array (lxi serves A and B1'); an int64 witness keeps its short-scalar
    // plan over NioLP, which no table of full-width windows helps
    for (const ps_points* arr : {sh.lxi2, sh.lxi, sh.lxi_t, sh.nio_lp})
        if (!rc && tables_wanted(c, arr->n) && (arr != sh.nio_lp || sol->max_bits >= 255)) rc = points_ensure_table(c, arr, 0, true);
    Scope scope;
    ps_scalars *va = nullptr, *vb = nullptr, *vh = nullptr, **sn = scope.scalars();  // the context's own vectors, and a view of the solution
    if (!rc) rc = prover_vector(c, 0, cn, &va);
    if (!rc) rc = prover_vector(c, 1, cn, &vb);
    if (!rc) rc = prover_vector(c, 2, ch, &vh);
    if (!rc && !c->ev_q && hipEventCreateWithFlags(&c->ev_q, hipEventDisableTiming) != hipSuccess) rc = fail(PS_ERR_HIP, "Groth16 share: event creation failed");
    if (!rc) rc = ps_scalars_slice(sol, diff + fq, cq, sn);
    if (rc) return rc;
    // the share's own kernels run on the context's high-priority stream, as the quotient of groth16_prove_impl does: the sums
    // launched right behind them (workers) must not hold back what every other device may be waiting for
    hipStream_t qs = c->tail;
    SumQueue sums{c, false};
    uint8_t part[5][192];
    for (int k = 0; k < 5; k++) write_identity(k == G16_B ? PS_G2 : PS_G1, part[k]);
    auto t_h = t_start;
    float h_ms = 0.f, own_ms = 0.f, wait_ms = 0.f;
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
        if ((rc = sums.launch(G16_B, sh.lxi2, vb, part[G16_B])) || (rc = sums.launch(G16_A, sh.lxi, va, part[G16_A])) ||
            (rc = sums.launch(G16_B1, sh.lxi, vb, part[G16_B1])))
            break;
        u32 flag = 0;  // the gate check's answer for the own rows
        if (hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, qs) != hipSuccess || hipStreamSynchronize(qs) != hipSuccess) {
            rc = fail(PS_ERR_HIP, "Groth16 share: reading the gate check failed");
            break;
        }
        own_ms = ms_since(t_start);
        if (flag) { rc = fail(PS_ERR_NOT_DIVISIBLE, "apocalypse"); break; }  // qap.go:158-160
        if ((rc = sums.launch(G16_N, sh.nio_lp, *sn, part[G16_N]))) break;
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
        wait_ms = ms_since(t_wait);
        t_h = std::chrono::steady_clock::now();
        if ((rc = sums.launch(G16_H, sh.lxi_t, vh, part[G16_H]))) break;
    } while (0);
    // everything that was launched is drained on every path: the next call on this context starts clean
    while (!sums.empty())
        if (sums.finish_one() == G16_H) h_ms = ms_since(t_h);
    (void)hipStreamSynchronize(qs);
    if (rc || sums.err) {
        KeepError keep;
        (void)ps_ctx_sync(c);
        return rc ? rc : sums.err;
    }
    rc = g16_share_c(part[G16_N], part[G16_H], part[G16_A], part[G16_B1], r_be32, s_be32, C_part);
    memcpy(A_part, part[G16_A], 96);
    memcpy(B_part, part[G16_B], 192);
    if (!rc && sh.fixed) rc = g16_add_fixed_points(*sh.fixed, r_be32, s_be32, A_part, B_part, C_part);
    c->phase_ms[0] = own_ms + wait_ms;
    c->phase_ms[1] = h_ms;
    c->phase_ms[3] = ms_since(t_start);
    c->phase_ms[2] = std::max(0.f, c->phase_ms[3] - c->phase_ms[0] - c->phase_ms[1]);
    return rc;
}

static int g16_local_key_check(const ps_groth16_pk& pk, const char* who) {
    if (pk.lxi->group != PS_G1 || pk.lxi_t->group != PS_G1 || pk.nio_lp->group != PS_G1 || pk.lxi2->group != PS_G2)
        return fail(PS_ERR_ARG, std::string(who) + ": CRS array in the wrong group");
    return PS_OK;
}

// ps_groth16_prove_multi, every device with lxi / lxi2 / lxi_t (the caller has checked handles and ranges): no coefficient
// vectors, nothing through host memory.  One host thread per device runs g16_lagrange_share.  The values route -- three
// convolutions of length 2 np -- is split over devices 0, 1, 2
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
    int rc;
    for (size_t d = 0; d < ndev; d++)
        if ((rc = g16_local_key_check(dev[d].pk, "ps_groth16_prove_multi")) || (rc = require_distinct_contexts(dev, d, "ps_groth16_prove_multi")))
            return rc;
    const size_t n = dev[0].qap->n;
    const bool hsplit = ndev >= 3 && dev[0].ctx->g16_multi_hsplit;
    FirstError ho;
    struct {  // beside the latch: the convolutions at hand (have == 3: all), where they are and the event behind each
        int have = 0;
        const Fr* S[3] = {nullptr, nullptr, nullptr};
        int sdev[3] = {0, 0, 0};
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    } conv;
    std::vector<G16Part> parts(ndev);
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
            ho.publish([&] {
                for (int k = 0; k < 3; k++)
                    if (S[k]) { conv.S[k] = S[k]; conv.sdev[k] = c->device; conv.ev[k] = c->ev_q; conv.have++; }
            });
            return PS_OK;
        };
        auto get_s = [&](hipStream_t qs, const Fr* out[3]) -> int {
            int r2 = ho.wait([&] { return conv.have == 3; });  // (complete from here on: read without the lock)
            if (r2) return r2;
            Fr* dst[3] = {q->coefA, q->coefB, q->coefC};
            for (int k = 0; k < 3; k++) {
                HIP_TRY(hipStreamWaitEvent(qs, conv.ev[k], 0));
                // S_P for hv[i] sits at n - 1 + i
                if ((r2 = copy_range_from(dst[k], c->device, conv.S[k] + (n - 1 + fh), conv.sdev[k], sizeof(Fr) * ch, qs))) return r2;
                out[k] = dst[k];
            }
            return PS_OK;
        };
        int rc = g16_lagrange_share(c, sh, r_be32, s_be32, produce, get_s, parts[d].A, parts[d].B, parts[d].C);
        if (rc) ho.set(rc);
    };
    run_per_device(ndev, work);
    if (ho.err) return fail(ho.err, ho.msg);
    return g16_fold_parts(parts, A_out, B_out, C_out);
}

// ---- monomial keys ----
// The three parts of the quotient are independent until the exchange: with three or more devices A, B and h (h-only
// route, which also carries the divisibility test) are computed side by side on devices 0, 1, 2; the coefficient vectors
// cross through host memory, each device takes its ranges, and the partial proofs are folded on the host.
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
    for (size_t d = 0; d < ndev; d++)
        if (!g16_holds_ranges(dev[d].pk, lag, n, nn, (int)d, (int)ndev) || dev[d].qap->n != n || dev[d].qap->m != m || dev[d].sol->n != m)
            return fail(PS_ERR_LENGTH, "ps_groth16_prove_multi: device " + std::to_string(d) + " does not hold its index range of the CRS arrays");
    if (lag) return groth16_prove_multi_lagrange(dev, ndev, nn, r_be32, s_be32, A_out, B_out, C_out);
    // ---- quotient: A, B, h as big-endian scalars in host memory ----
    std::vector<uint8_t> hA, hB, hH;
    {
        auto piece = [&](size_t d, int what, std::vector<uint8_t>* dst) -> int {  // 0: A, 1: B, 2: h, 3: all three
            Scope scope;
            ps_scalars **a = scope.scalars(), **b = scope.scalars(), **h = scope.scalars();
            int rc = PS_OK;
            if (what == 0) rc = ps_qap_interpolate(dev[d].ctx, dev[d].qap, dev[d].sol, 0, a);
            else if (what == 1) rc = ps_qap_interpolate(dev[d].ctx, dev[d].qap, dev[d].sol, 1, b);
            else if (what == 2) rc = ps_qap_quotient(dev[d].ctx, dev[d].qap, dev[d].sol, nullptr, nullptr, nullptr, h);
            else rc = ps_qap_quotient(dev[d].ctx, dev[d].qap, dev[d].sol, a, b, nullptr, h);
            if (!rc && *a) rc = g16_download_all(dev[d].ctx, *a, what == 3 ? hA : *dst);
            if (!rc && *b) rc = g16_download_all(dev[d].ctx, *b, what == 3 ? hB : *dst);
            if (!rc && *h) rc = g16_download_all(dev[d].ctx, *h, what == 3 ? hH : *dst);
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
    // ---- per-device sums over the local arrays, one host thread per device; no device waits for another ----
    FirstError ho;
    std::vector<G16Part> parts(ndev);
    auto work = [&](size_t d) {
        ps_ctx* c = dev[d].ctx;
        const ps_groth16_pk& pk = dev[d].pk;
        size_t fn, cn, fh, ch, fq, cq;
        shard_range_c(n, (int)d, (int)ndev, &fn, &cn);
        shard_range_c(n - 1, (int)d, (int)ndev, &fh, &ch);
        shard_range_c(nn, (int)d, (int)ndev, &fq, &cq);
        Scope scope;  // this thread's: freed on it, each handle on its own device
        ps_scalars **a = scope.scalars(), **b = scope.scalars(), **h = scope.scalars(), **sn = scope.scalars();
        int rc = ps_scalars_upload(c, hA.data() + 32 * fn, cn, a);
        if (!rc) rc = ps_scalars_upload(c, hB.data() + 32 * fn, cn, b);
        if (!rc) rc = ps_scalars_upload(c, hH.data() + 32 * fh, ch, h);
        if (!rc) rc = ps_scalars_slice(dev[d].sol, diff + fq, cq, sn);
        // five sums through the queue, as ps_msm_launch places them (the context's own stream included: no quotient runs on it)
        SumQueue sums{c, true};
        uint8_t part[5][192];
        const struct { int kind; const ps_points* pts; const ps_scalars* sc; } five[5] = {
            {G16_B, pk.xi2, *b}, {G16_A, pk.xi, *a}, {G16_B1, pk.xi, *b}, {G16_N, pk.nio_lp, *sn}, {G16_H, pk.xi_t, *h}};
        for (int k = 0; k < 5 && !rc && !sums.err; k++) rc = sums.launch(five[k].kind, five[k].pts, five[k].sc, part[five[k].kind]);  // none after a failed finish
        sums.drain();
        if (!rc) rc = sums.err;
        if (!rc) rc = g16_share_c(part[G16_N], part[G16_H], part[G16_A], part[G16_B1], r_be32, s_be32, parts[d].C);
        if (!rc) {
            memcpy(parts[d].A, part[G16_A], 96);
            memcpy(parts[d].B, part[G16_B], 192);
            if (d == 0) rc = g16_add_fixed_points(pk, r_be32, s_be32, parts[d].A, parts[d].B, parts[d].C);  // of all three elements
        }
        if (rc) ho.set(rc, d, true);
    };
    run_per_device(ndev, work);
    if (ho.err) return fail(ho.err, ho.msg);
    return g16_fold_parts(parts, A_out, B_out, C_out);
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
    if (!g16_holds_ranges(*pk, true, n, nn, rank, world))
        return fail(PS_ERR_LENGTH, "ps_groth16_prove_local: rank " + std::to_string(rank) + " of " + std::to_string(world) +
                                       " does not hold its index range of the CRS arrays");
    size_t fh, ch;
    shard_range_c(n - 1, rank, world, &fh, &ch);
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
