// ps_phgr13_verify_batch: PHGR13Verify (pinochio.go:281-378) for N proofs under one key by random linear combination
// (included by capi.hip after verify_locate.inc).  The five products of ps_phgr13_verify (pairing.inc), each weighted by
// the caller's rho_i and each with its OWN final exponentiation:
//     E0 division  prod_i e(rho_i gv_i, wss_i) prod_k e(P_k, ws_k) e(-S_hs, yts) e(-(S_yss + sum_j t_j ys_j), G2) = 1
//                  gv_i = sum_j io_ij vs_j + vss_i,  P_k = sum_i io_ik (rho_i gv_i),  t_j = sum_i rho_i io_ij
//     E1 v         e(S_vass, G2) e(-S_vss, av) = 1
//     E2 w         e(S_wass, G2) e(-aw, S_wss) = 1
//     E3 y         e(S_yass, G2) e(-S_yss, ay) = 1
//     E4 linear    e(S_gz, gamma) e(-(S_vss + S_yss), bgamma2) e(-bgamma, S_wss) = 1
// with S_X = sum_i rho_i X_i.  E0 is prod_i e(rho_i gv_i, wio_i + wss_i) with wio_i = sum_k io_ik ws_k expanded by
// bilinearity: N + diff Miller loops on the device and no G2 arithmetic per proof.
// No kernel of its own.  rho_i gv_i: k_fr_locate_rows, segment_sums (verify_locate.inc), k_ec_scale and k_g1_pair_sums; P_k:
// ps_msm_batch over the columns of io (k_gather_words transposes them); the eight S_X: ONE ps_msm_multi; t: weighted_columns;
// the loops and their product: k_miller_batch, k_f12_product (verify_batch.inc).  The host runs the remaining eleven loops
// and the five final exponentiations on its threads, as ps_phgr13_verify does.
// The body is phgr13_verify_batch_impl, which ps_phgr13_verify_batch_locate (verify_phgr13_locate.inc) calls too: there it keeps
// the levels of the product tree and hands a rejected batch's device state over (PvbKeep).

constexpr size_t PS_PHGR13_VERIFY_BATCH_MAX = (size_t)1 << 20;
constexpr size_t PS_PHGR13_VERIFY_BATCH_TERMS = (size_t)1 << 24;  // proofs x (diff + 1): the two XYZZ buffers of the segments are 2 x 224 B each

// Wall clock of the stages of the last ps_phgr13_verify_batch on a context with ps_ctx_set_timing on (the stream is drained at
// every stage boundary, as for ps_debug_verify_batch_stage_ms): [0] key checks, upload and subgroup tests  [1] rho_i gv_i
// [2] sums: P_k, the eight S_X, t and its sum over ys  [3] k_miller_batch and the product tree  [4] host: download, eleven
// Miller loops, five final exponentiations.  Measurement hook, not in the header.
constexpr int PS_PVB_STAGES = 5;
extern "C" int ps_debug_phgr13_verify_batch_stage_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "ps_debug_phgr13_verify_batch_stage_ms: NULL argument");
    for (int i = 0; i < PS_PVB_STAGES; i++) ms[i] = c->pvb_ms[i];
    return PS_OK;
}

// Index of the first point of `arr` outside the order-r subgroup, for the message of a batch that ps_points_check_subgroup
// has rejected: halving with the same device test (log2 n launches, failure path only).
static int first_outside_subgroup(ps_ctx* c, const ps_points* arr, size_t* idx) {
    size_t lo = 0, hi = arr->n;  // a bad point lies in [lo, hi)
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        Scope scope;
        ps_points** half = scope.points();
        int in = 0, rc = ps_points_slice(arr, lo, mid - lo, half);
        if (!rc) rc = ps_points_check_subgroup(c, *half, &in);
        if (rc) return rc;
        if (in) lo = mid; else hi = mid;
    }
    *idx = lo;
    return PS_OK;
}

// What a REJECTED batch hands to the descent of ps_phgr13_verify_batch_locate (verify_phgr13_locate.inc) instead of freeing
// it, in the manner of VbKeep: rho (plain words; its Montgomery form stays in c->vb_rho until the next call), the views of the
// seven G1 elements and of wss, rho_i gv_i (affine, the P_k behind them), the transposed inputs, and the key's points.  The
// handles are the holder's from then on.  The Miller values stay where phgr13_miller_levels put them (c->lc_f12).
struct PvbKeep {
    ps_scalars *rho = nullptr, *iot = nullptr;
    ps_points* view[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // vss vass wass yss yass hs gz | wss
    ps_points *g1 = nullptr, *rgv = nullptr;  // what the G1 views are slices of; rho_i gv_i
    Affine<Fp> aw, bgamma;
    Affine<Fp2> av, ay, gamma, bgamma2, yts;
};
// verify_phgr13_locate.inc: k_miller_batch over the n + diff pairs, the product tree over the first n values with every
// level kept (c->lc_f12), the key's loops multiplied in separately; *res is the batch's product
static int phgr13_miller_levels(ps_ctx* c, const std::string& fn, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, size_t diff,
                                const pairing_dev::Fp12** res);

// The batch check behind ps_phgr13_verify_batch (fn = its name, keep = nullptr) and ps_phgr13_verify_batch_locate (its own
// name; keep != nullptr: the levels of the product tree are retained and a rejected batch fills *keep).
static int phgr13_verify_batch_impl(ps_ctx* c, const std::string& fn, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proofs,
                                    size_t nproofs, const uint8_t* rho_be32, int* ok, PvbKeep* keep) {
    VbClock clk(c, c->pvb_ms, PS_PVB_STAGES);
    if (c->q_len) return fail(PS_ERR_ARG, fn + ": sums are pending on this context (ps_msm_finish them first)");
    const size_t N = nproofs, diff = vk->vs_io->n, cols = diff + 1, pd = std::max<size_t>(diff, 1);
    if (N > PS_PHGR13_VERIFY_BATCH_MAX)
        return fail(PS_ERR_ARG, fn + ": more than 2^20 proofs in one batch (split it: the verdicts of the parts AND together)");
    if (diff >= PS_PHGR13_VERIFY_BATCH_TERMS || N * cols >= PS_PHGR13_VERIFY_BATCH_TERMS)
        return fail(PS_ERR_ARG, fn + ": " + std::to_string(N) + " proofs of " + std::to_string(diff) +
                                    " public inputs: proofs x (inputs + 1) must stay below 2^24 (split the batch: the verdicts of the parts AND together)");
    if (vk->vs_io->group != PS_G1 || vk->ws_io->group != PS_G2 || vk->ys_io->group != PS_G1)
        return fail(PS_ERR_ARG, fn + ": vs_io and ys_io must be G1 arrays and ws_io a G2 array");
    if (vk->ws_io->n != diff || vk->ys_io->n != diff)
        return fail(PS_ERR_LENGTH, fn + ": vs_io, ws_io and ys_io have " + std::to_string(diff) + ", " + std::to_string(vk->ws_io->n) + " and " +
                                       std::to_string(vk->ys_io->n) + " points");
    if (io->n != N * diff)
        return fail(PS_ERR_LENGTH, fn + ": " + std::to_string(io->n) + " public inputs for " + std::to_string(N) + " proofs of " +
                                       std::to_string(diff) + " each");
    if (N == 0) { *ok = 1; return PS_OK; }
    u32 rho_sum[8];  // (not needed here: no equation has a term that is the same for every proof)
    int rc = batch_weights(fn, rho_be32, N, rho_sum);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the key: as in ps_phgr13_verify
    for (const ps_points* arr : {vk->vs_io, vk->ws_io, vk->ys_io})
        if ((rc = vk_array_in_subgroup(c, arr, fn.c_str()))) return rc;
    Affine<Fp> aw, bgamma;
    Affine<Fp2> av, ay, gamma, bgamma2, yts;
    if (!read_g2(av, vk->av) || !read_g1(aw, vk->aw) || !read_g2(ay, vk->ay) || !read_g2(gamma, vk->gamma) || !read_g1(bgamma, vk->bgamma) ||
        !read_g2(bgamma2, vk->bgamma2) || !read_g2(yts, vk->yts))
        return fail(PS_ERR_ENCODING, fn + ": bad point encoding in the verification key");
    if (!all_in_subgroup({&aw, &bgamma}, {&av, &ay, &gamma, &bgamma2, &yts}))
        return fail(PS_ERR_ENCODING, fn + ": verification-key point outside the order-r subgroup");
    // the proofs: ONE G1 array of 7 N points, element-major, and one G2 array, through the validating upload; then [r]P on
    // the device -- two launches of that latency chain, not eight
    constexpr int NG1 = 7;
    enum { VSS, VASS, WASS, YSS, YASS, HS, GZ };
    static const char* const g1_names[NG1] = {"vss", "vass", "wass", "yss", "yass", "hs", "gz"};
    static const size_t g1_offs[NG1] = {offsetof(ps_phgr13_proof, vss), offsetof(ps_phgr13_proof, vass), offsetof(ps_phgr13_proof, wass),
                                        offsetof(ps_phgr13_proof, yss), offsetof(ps_phgr13_proof, yass), offsetof(ps_phgr13_proof, hs),
                                        offsetof(ps_phgr13_proof, gz)};
    std::vector<Affine<Fp>> pk(diff);  // P_k on their way to the device: outlives the scope, which waits for the copy
    Scope scope(c->stream);
    ps_points **g1 = scope.points(), **wss = scope.points(), **g1m = scope.points(), **g2m = scope.points(), **rgv = scope.points();
    ps_points* view[NG1 + 1];
    ps_scalars **rho = scope.scalars(), **iot = scope.scalars();
    {
        std::vector<uint8_t> raw(96 * NG1 * N);
        for (int e = 0; e < NG1; e++)
            for (size_t i = 0; i < N; i++) memcpy(raw.data() + 96 * (e * N + i), (const uint8_t*)&proofs[i] + g1_offs[e], 96);
        rc = ps_points_upload(c, PS_G1, raw.data(), NG1 * N, PS_FMT_AFFINE, g1);
        if (rc == PS_ERR_ENCODING) {
            const size_t bad = first_bad_encoding<Fp>(raw, NG1 * N, 96);
            return fail(PS_ERR_ENCODING, fn + ": " + g1_names[bad / N] + " of proof " + std::to_string(bad % N) + " is not a canonical point on the curve");
        }
        if (rc) return rc;
        raw.resize(192 * N);
        for (size_t i = 0; i < N; i++) memcpy(raw.data() + 192 * i, proofs[i].wss, 192);
        rc = ps_points_upload(c, PS_G2, raw.data(), N, PS_FMT_AFFINE, wss);
        if (rc == PS_ERR_ENCODING)
            return fail(PS_ERR_ENCODING, fn + ": wss of proof " + std::to_string(first_bad_encoding<Fp2>(raw, N, 192)) + " is not a canonical point on the curve");
        if (rc) return rc;
    }
    for (const ps_points* arr : {(const ps_points*)*g1, (const ps_points*)*wss}) {
        int in = 0;
        if ((rc = ps_points_check_subgroup(c, arr, &in))) return rc;
        if (in) continue;
        size_t bad = 0;
        if ((rc = first_outside_subgroup(c, arr, &bad))) return rc;
        return fail(PS_ERR_ENCODING, fn + ": " + (arr->group == PS_G1 ? g1_names[bad / N] : "wss") + " of proof " + std::to_string(bad % N) +
                                         " is outside the order-r subgroup");
    }
    ps_points** views[NG1];
    for (int e = 0; e < NG1; e++) {
        ps_points** v = views[e] = scope.points();
        if ((rc = ps_points_slice(*g1, e * N, N, v))) return rc;
        view[e] = *v;
    }
    view[NG1] = *wss;
    clk.mark(0);
    // rho on the device: plain words for the sums, Montgomery form for the scalings and the column sums
    if ((rc = ps_scalars_upload(c, rho_be32, N, rho))) return rc;
    if ((rc = c->vb_rho.ensure(sizeof(Fr) * N))) return rc;
    Fr* rho_m = (Fr*)c->vb_rho.p;
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(N)), dim3(256), 0, c->stream, rho_m, scalars_ptr(*rho), (u64)N);
    if (storage_wait_ready(io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
    // rho_i gv_i = sum_j (rho_i io_ij) vs_j + rho_i vss_i.  Scalars: the rows of the locate descent, their io part in Montgomery
    // form.  Points (c->vb_xyzz): two buffers of N x diff for the segments | vs_io | 2 N for the last addition | N and
    // their chain products for the normalisation.
    const size_t o_t = 32 * cols * N, o_tm = o_t + 32 * pd * N;
    if ((rc = c->pvb_rows.ensure(o_tm + sizeof(Fr) * pd * N))) return rc;
    if ((rc = c->vb_xyzz.ensure(sizeof(Xyzz<Fp>) * (2 * N * pd + pd + 2 * N) + batch_affine_tmp_bytes(N, sizeof(Xyzz<Fp>))))) return rc;
    Xyzz<Fp>*src = (Xyzz<Fp>*)c->vb_xyzz.p, *dst = src + N * pd, *vsx = dst + N * pd, *two = vsx + pd, *sum = two + 2 * N;
    if ((rc = points_alloc(c, PS_G1, N + diff, g1m)) || (rc = points_alloc(c, PS_G2, N + diff, g2m))) return rc;
    const Affine<Fp>* vss_d = (const Affine<Fp>*)points_ptr(view[VSS]);
    auto scaled_vss = [&](Xyzz<Fp>* out) {  // rho_i vss_i
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(N)), dim3(256), 0, c->stream, vss_d, (u32)N, (u32)N, out);
        hipLaunchKernelGGL(k_ec_scale<Fp>, dim3(nblocks(N)), dim3(256), 0, c->stream, out, (u32)N, (const Fr*)rho_m, ~0ull);
    };
    if (diff) {
        u32* rows = (u32*)c->pvb_rows.p;
        u32* tw = (u32*)((char*)c->pvb_rows.p + o_t);
        Fr* tm = (Fr*)((char*)c->pvb_rows.p + o_tm);
        if (storage_wait_ready(vk->vs_io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
        hipLaunchKernelGGL(k_fr_locate_rows, dim3(nblocks(N * cols)), dim3(256), 0, c->stream, scalars_ptr(*rho), (const Fr*)rho_m, scalars_ptr(io), (u32)N,
                           (u32)diff, rows);
        hipLaunchKernelGGL(k_gather_words, dim3(nblocks(N * 8 * diff)), dim3(256), 0, c->stream, (const u32*)rows, (const u32*)nullptr, (u32)N, (u64)(8 * cols),
                           (u64)8, (u32)(8 * diff), tw);
        hipLaunchKernelGGL(k_fr_to_mont, dim3(nblocks(N * diff)), dim3(256), 0, c->stream, tm, (const u32*)tw, (u64)(N * diff));
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(diff)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(vk->vs_io), (u32)diff, (u32)diff, vsx);
        segment_sums(c, vsx, diff, N, tm, &src, &dst);
        // the last addition, complete like every other (vss_i = -vio_i: the identity; vss_i = vio_i: a doubling): the two
        // operands of proof i side by side -- k_g1_pair_sums over segments of ONE point is a strided copy
        scaled_vss(dst);
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(N)), dim3(256), 0, c->stream, (const Xyzz<Fp>*)dst, 1u, (u32)N, 1u, two, 2u);
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(N)), dim3(256), 0, c->stream, (const Xyzz<Fp>*)src, 1u, (u32)N, (u32)diff, two + 1, 2u);
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(N)), dim3(256), 0, c->stream, (const Xyzz<Fp>*)two, 2u, (u32)N, 2u, sum, 1u);
    } else {
        scaled_vss(sum);  // gv_i = vss_i
    }
    batch_to_affine<Fp>(c->stream, (char*)sum, N, (char*)(*g1m)->st->p, (u32)sizeof(Affine<Fp>));
    HIP_TRY(hipGetLastError());
    // the G2 side of the device's loops: wss || ws_io
    if (storage_wait_ready(vk->ws_io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
    HIP_TRY(hipMemcpyAsync((*g2m)->st->p, points_ptr(*wss), sizeof(Affine<Fp2>) * N, hipMemcpyDeviceToDevice, c->stream));
    if (diff)
        HIP_TRY(hipMemcpyAsync((Affine<Fp2>*)(*g2m)->st->p + N, points_ptr(vk->ws_io), sizeof(Affine<Fp2>) * diff, hipMemcpyDeviceToDevice, c->stream));
    clk.mark(1);
    // P_k = sum_i io_ik (rho_i gv_i): one batch of diff sums over the N points, member k = column k of io
    if (diff) {
        if ((rc = scalars_alloc(c, diff * N, iot))) return rc;
        for (size_t k = 0; k < diff; k++)
            hipLaunchKernelGGL(k_gather_words, dim3(nblocks(N * 8)), dim3(256), 0, c->stream, scalars_ptr(io), (const u32*)nullptr, (u32)N, (u64)(8 * diff),
                               (u64)(8 * k), 8u, (u32*)(*iot)->st->p + 8 * N * k);
        HIP_TRY(hipGetLastError());
        if (storage_mark_ready((*iot)->st, c->stream) || storage_mark_ready((*g1m)->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event record failed");
        if ((rc = ps_points_slice(*g1m, 0, N, rgv))) return rc;
        std::vector<uint8_t> pkb(96 * diff);
        if ((rc = ps_msm_batch(c, *rgv, *iot, diff, pkb.data()))) return rc;
        for (size_t k = 0; k < diff; k++)
            if (!read_g1(pk[k], pkb.data() + 96 * k)) return fail(PS_ERR_ENCODING, fn + ": bad point from a sum");
        HIP_TRY(hipMemcpyAsync((Affine<Fp>*)(*g1m)->st->p + N, pk.data(), sizeof(Affine<Fp>) * diff, hipMemcpyHostToDevice, c->stream));
        scope.in_flight();  // pk is read until the stream has passed the copy
    }
    clk.mark(2);
    // the device's share of E0: N + diff loops and their product in ONE launch each, only enqueued here -- the sums below
    // queue up behind them
    const pairing_dev::Fp12* fdev = nullptr;
    rc = keep ? phgr13_miller_levels(c, fn, (const Affine<Fp>*)points_ptr(*g1m), (const Affine<Fp2>*)points_ptr(*g2m), N, diff, &fdev)
              : miller_product_launch(c, (const Affine<Fp>*)points_ptr(*g1m), (const Affine<Fp2>*)points_ptr(*g2m), N + diff, &fdev);
    if (rc) return rc;
    clk.mark(3);
    // the eight S_X: one sort of rho, eight point passes
    uint8_t sb[NG1][96], swss[192], tyb[96];
    uint8_t* outs[NG1 + 1];
    for (int e = 0; e < NG1; e++) outs[e] = sb[e];
    outs[NG1] = swss;
    if ((rc = ps_msm_multi(c, view, NG1 + 1, *rho, outs))) return rc;
    // sum_j t_j ys_j, t_j = sum_i rho_i io_ij: one sum instead of N
    if ((rc = weighted_io_sum(c, fn, scope, rho_m, io, N, vk->ys_io, tyb))) return rc;
    clk.mark(2);
    pairing::Fp12 fdiv;
    if ((rc = miller_product_fetch(c, fdev, &fdiv))) return rc;
    Affine<Fp> s[NG1], ty;
    Affine<Fp2> s_wss;
    bool good = read_g2(s_wss, swss) && read_g1(ty, tyb);
    for (int e = 0; e < NG1; e++) good = good && read_g1(s[e], sb[e]);
    if (!good) return fail(PS_ERR_ENCODING, fn + ": bad point from a sum");
    // the host's share: eleven loops, then the five products and their final exponentiations, on host threads
    using pairing_dev::neg_g1;
    const Affine<Fp2> g2 = generator((const Fp2*)0);
    struct Loop { int eq; Affine<Fp> p; Affine<Fp2> q; };
    const Loop loops[11] = {
        {0, neg_g1(s[HS]), yts},   {0, neg_g1(affine_sum<Fp>(s[YSS], ty)), g2},
        {1, s[VASS], g2},          {1, neg_g1(s[VSS]), av},
        {2, s[WASS], g2},          {2, neg_g1(aw), s_wss},
        {3, s[YASS], g2},          {3, neg_g1(s[YSS]), ay},
        {4, s[GZ], gamma},         {4, neg_g1(affine_sum<Fp>(s[VSS], s[YSS])), bgamma2},  {4, neg_g1(bgamma), s_wss},
    };
    pairing::Fp12 val[11];
    locate_parallel(11, [&](size_t j) { val[j] = pairing::miller(affine_to_host<Fp>(loops[j].p), affine_to_host<Fp2>(loops[j].q)); });
    uint8_t holds[5];
    locate_parallel(5, [&](size_t e) {
        pairing::Fp12 f = e == 0 ? fdiv : pairing::f12_one();
        for (int j = 0; j < 11; j++)
            if (loops[j].eq == (int)e) f = pairing::f12_mul(f, val[j]);
        holds[e] = pairing::f12_eq(pairing::final_exp(f), pairing::f12_one()) ? 1 : 0;
    });
    u32 failed = 0;
    for (int e = 0; e < 5; e++)
        if (!holds[e]) failed |= 1u << e;
    c->pvb_info.failed = failed;
    c->pvb_info.device_loops = (u32)(N + diff);
    *ok = failed ? 0 : 1;
    clk.mark(4);
    if (keep && failed) {  // out of the scope's slots: the holder's from here on
        auto take = [](auto** slot) { auto* h = *slot; *slot = nullptr; return h; };
        for (int e = 0; e < NG1; e++) keep->view[e] = take(views[e]);
        keep->view[NG1] = take(wss);
        keep->g1 = take(g1);
        keep->rgv = take(g1m);
        keep->rho = take(rho);
        keep->iot = take(iot);
        keep->aw = aw; keep->bgamma = bgamma;
        keep->av = av; keep->ay = ay; keep->gamma = gamma; keep->bgamma2 = bgamma2; keep->yts = yts;
    }
    return scope.finish(PS_OK);
}

extern "C" int ps_phgr13_verify_batch(ps_ctx* c, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proofs, size_t nproofs,
                                      const uint8_t* rho_be32, int* ok) {
    if (!c || !vk || !io || !ok || !vk->vs_io || !vk->ws_io || !vk->ys_io || (nproofs && (!proofs || !rho_be32)))
        return fail(PS_ERR_ARG, "ps_phgr13_verify_batch: NULL argument");
    *ok = 0;
    c->pvb_info = ps_phgr13_batch_info{0, 0, {0, 0}};
    return phgr13_verify_batch_impl(c, "ps_phgr13_verify_batch", vk, io, proofs, nproofs, rho_be32, ok, nullptr);
}

extern "C" int ps_phgr13_verify_batch_info(ps_ctx* c, ps_phgr13_batch_info* out) {
    if (!c || !out) return fail(PS_ERR_ARG, "ps_phgr13_verify_batch_info: NULL argument");
    *out = c->pvb_info;
    return PS_OK;
}
