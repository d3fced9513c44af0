// ps_phgr13_verify_batch_locate: WHICH proofs of a rejected PHGR13 batch are invalid, and which of the five equations each one
// violates, by bisection over partial results kept on the device (included by capi.hip after verify_phgr13_batch.inc and
// locate_phgr13_dev.hpp).  Notation of verify_phgr13_batch.inc; for a set S of proofs X_S = sum_{i in S} rho_i X_i,
// t_S,j = sum_S rho_i io_ij, P_S,k = sum_S io_ik (rho_i gv_i), F_S = prod_S miller(rho_i gv_i, wss_i), and
//     E0(S)  final_exp(F_S prod_k miller(P_S,k, ws_k) miller(-hs_S, yts) miller(-(yss_S + sum_j t_S,j ys_j), G2)) == 1
//     E1(S)  final_exp(miller(vass_S, G2) miller(-vss_S, av)) == 1
//     E2(S)  final_exp(miller(wass_S, G2) miller(-aw, wss_S)) == 1
//     E3(S)  final_exp(miller(yass_S, G2) miller(-yss_S, ay)) == 1
//     E4(S)  final_exp(miller(gz_S, gamma) miller(-(vss_S + yss_S), bgamma2) miller(-bgamma, wss_S)) == 1
// are the batch's equations restricted to S, each multiplicative over disjoint unions, and E_c({i}) is proof i's own
// equation c raised to rho_i != 0.
//   1. the batch check of ps_phgr13_verify_batch (phgr13_verify_batch_impl), the levels of its product tree kept:
//      accepted -> done, one check and five products, nothing else launched;
//   2. otherwise the trees the failed equations read (locate_phgr13_dev.hpp), built once;
//   3. the descent: locate_bisect (locate_descent.hpp, shared with verify_locate.inc and run as it ships by
//      tests/host_phgr13_locate_index.cpp) from the root's mask of failed equations.  A round (phgr13_locate_check_sets): the
//      sets' values gathered on the device, sum_j t_S,j ys_j by segment_sums, the K diff loops with the key's ws_k on the
//      device and reduced with F_S to ONE value per set (k_f12_segment_products), one normalisation per group, one download;
//      the remaining loops and one final exponentiation per tested (set, equation) on at most 16 host threads.  The round
//      helpers are those of verify_locate.inc.  No step after the batch check passes over the proofs of a set again.

// The Miller values of a locating batch: k_miller_batch over all n + diff pairs into c->lc_f12, the levels of the product
// tree over the FIRST n (every level kept, as locate_miller_levels keeps them), and the product of the key's diff loops taken
// into the root separately -- so that the root verdict is the batch's and the F tree holds the proofs' loops alone.
static int phgr13_miller_levels(ps_ctx* c, const std::string& fn, const Affine<Fp>* g1, const Affine<Fp2>* g2, size_t n, size_t diff,
                                const pairing_dev::Fp12** res) {
    typedef pairing_dev::Fp12 D12;
    u32 simds = 0;
    int rc = ctx_simds(c, &simds);
    if (rc) return rc;
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    const int nl = locate::tree_levels(n, size, off);
    const size_t bytes = sizeof(D12) * phgr13_locate::f_tree_values(off, nl, diff);
    if (c->lc_f12.ensure(bytes))
        return fail(PS_ERR_HIP, fn + ": no device memory for the levels of the product tree (" + std::to_string(bytes) + " bytes for " + std::to_string(n) +
                                    " proofs of " + std::to_string(diff) + " public inputs)");
    D12* f = (D12*)c->lc_f12.p;
    u32 lpw = pairing_dev::spread_lanes(n + diff, simds);
    hipLaunchKernelGGL(k_miller_batch, dim3((unsigned)((n + diff + lpw - 1) / lpw)), dim3(64), 0, c->stream, g1, g2, (u32)(n + diff), lpw, f);
    locate_product_levels(c, f, size, off, nl, diff, simds);
    // the key's loops: a product tree of their own (a chain of diff products on one lane costs 13 ms at diff = 63), then root x root
    const D12* key = f + n;
    D12* lvl = f + phgr13_locate::f_key_levels_at(off, nl, diff);
    for (size_t m = diff; m > 1;) {
        const size_t h = (m + 1) / 2;
        lpw = pairing_dev::spread_lanes(h, simds);
        hipLaunchKernelGGL(k_f12_product, dim3((unsigned)((h + lpw - 1) / lpw)), dim3(64), 0, c->stream, key, (u32)m, lpw, lvl);
        key = lvl;
        lvl += h;
        m = h;
    }
    D12* out = f + phgr13_locate::f_product_at(off, nl, diff);
    hipLaunchKernelGGL(k_f12_segment_products, dim3(1), dim3(64), 0, c->stream, (const D12*)(f + phgr13_locate::f_level_base(off, nl - 1, diff)), key, 1u,
                       diff ? 1u : 0u, 1u, out);
    HIP_TRY(hipGetLastError());
    *res = out;
    return PS_OK;
}

struct Phgr13Trees {
    int nl = 0;  // levels, the root is level nl - 1
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    size_t N = 0, diff = 0;
    u32 mask = 0;                           // the root's failed equations: what the trees were built for
    int slot[phgr13_locate::G1_ELEMENTS];   // segment of an element's tree, -1: not built
    size_t nseg = 0, segs = 0;              // element trees; all G1 trees (the P trees behind the elements')
    const Xyzz<Fp>* g1 = nullptr;           // level-major (phgr13_locate::segment_node)
    const Xyzz<Fp2>* wss = nullptr;
    const pairing_dev::Fp12* f = nullptr;
    const u32* rows = nullptr;
    const Xyzz<Fp>* ysx = nullptr;          // ys_io in XYZZ form
    bool has(int e) const { return slot[e] >= 0; }
    bool division() const { return mask & 1u; }
    bool g2() const { return mask & phgr13_locate::WSS_EQUATIONS; }
};

// The trees the root's failed equations read, enqueued on c->stream
static int phgr13_locate_build_trees(ps_ctx* c, const std::string& fn, const ps_phgr13_vk* vk, const ps_scalars* io, size_t N, u32 mask, const PvbKeep& keep,
                                     Phgr13Trees* t) {
    constexpr size_t WX = sizeof(Xyzz<Fp>) / 4, WR = sizeof(Fr) / 4;
    const size_t diff = vk->vs_io->n, cols = diff + 1;
    t->N = N;
    t->diff = diff;
    t->mask = mask;
    t->nl = locate::tree_levels(N, t->size, t->off);
    t->nseg = (size_t)phgr13_locate::element_slots(mask, t->slot);
    const bool div = t->division() && diff;  // the trees E0 alone reads beyond hs and yss
    t->segs = t->nseg + (div ? diff : 0);
    const u64 nodes = t->off[t->nl];
    // leaves' workspace: the needed elements side by side (affine) | rho repeated for them | rho_i gv_i in XYZZ form | the
    // transposed inputs in Montgomery form
    LocateCarve carve;
    const size_t o_aff = carve.take(sizeof(Affine<Fp>) * t->nseg * N), o_rho = carve.take(sizeof(Fr) * t->nseg * N),
                 o_gv = carve.take(div ? sizeof(Xyzz<Fp>) * N : 0), o_tm = carve.take(div ? sizeof(Fr) * diff * N : 0), work = carve.total();
    const size_t b_g1 = sizeof(Xyzz<Fp>) * t->segs * nodes, b_g2 = t->g2() ? sizeof(Xyzz<Fp2>) * nodes : 0, b_rows = div ? 32 * cols * nodes : 0,
                 b_ys = sizeof(Xyzz<Fp>) * std::max<size_t>(diff, 1);
    if (c->lc_pts.ensure(b_g1) || c->plc_g2.ensure(b_g2) || c->lc_rows.ensure(b_rows) || c->lc_iolp.ensure(b_ys) || c->lc_work.ensure(work))
        return fail(PS_ERR_HIP, fn + ": no device memory for the trees (" + std::to_string(b_g1 + b_g2 + b_rows + b_ys + work) + " bytes for " +
                                    std::to_string(N) + " proofs of " + std::to_string(diff) + " public inputs)");
    char* w = (char*)c->lc_work.p;
    Xyzz<Fp>* g1 = (Xyzz<Fp>*)c->lc_pts.p;
    const Fr* rho_m = (const Fr*)c->vb_rho.p;
    // element trees: rho_i X_i for the elements in play, one scaling for all of them
    if (t->nseg) {
        for (int e = 0; e < phgr13_locate::G1_ELEMENTS; e++)
            if (t->has(e))
                HIP_TRY(hipMemcpyAsync((Affine<Fp>*)(w + o_aff) + (size_t)t->slot[e] * N, points_ptr(keep.view[e]), sizeof(Affine<Fp>) * N, hipMemcpyDeviceToDevice,
                                       c->stream));
        locate_gather(c, rho_m, nullptr, t->nseg, 0, 0, WR * N, w + o_rho);  // rho, once per element
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(t->nseg * N)), dim3(256), 0, c->stream, (const Affine<Fp>*)(w + o_aff), (u32)(t->nseg * N),
                           (u32)(t->nseg * N), g1);
        hipLaunchKernelGGL(k_ec_scale<Fp>, dim3(nblocks(t->nseg * N)), dim3(256), 0, c->stream, g1, (u32)(t->nseg * N), (const Fr*)(w + o_rho), ~0ull);
    }
    // P trees: leaves io_ik (rho_i gv_i), tree k behind the elements'
    if (div) {
        Xyzz<Fp>* leaves = g1 + t->nseg * N;
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(N)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(keep.rgv), (u32)N, (u32)N,
                           (Xyzz<Fp>*)(w + o_gv));
        locate_gather(c, w + o_gv, nullptr, diff, 0, 0, WX * N, leaves);  // rho_i gv_i, once per public input
        hipLaunchKernelGGL(k_fr_to_mont, dim3(nblocks(diff * N)), dim3(256), 0, c->stream, (Fr*)(w + o_tm), scalars_ptr(keep.iot), (u64)(diff * N));
        hipLaunchKernelGGL(k_ec_scale<Fp>, dim3(nblocks(diff * N)), dim3(256), 0, c->stream, leaves, (u32)(diff * N), (const Fr*)(w + o_tm), ~0ull);
    }
    for (int l = 0; l + 1 < t->nl && t->segs; l++) {
        const u64 n = t->size[l], h = t->size[l + 1];
        hipLaunchKernelGGL(k_g1_pair_sums, dim3(nblocks(t->segs * h)), dim3(256), 0, c->stream, (const Xyzz<Fp>*)(g1 + t->segs * t->off[l]), (u32)n, (u32)t->segs,
                           (u32)n, g1 + t->segs * t->off[l + 1], (u32)h);
    }
    // the wss tree in G2: one lane pair per point
    if (t->g2()) {
        Xyzz<Fp2>* g2 = (Xyzz<Fp2>*)c->plc_g2.p;
        hipLaunchKernelGGL(k_ec_from_affine<Fp2s>, dim3(nblocks(2 * N)), dim3(256), 0, c->stream, (const Affine<Fp2>*)points_ptr(keep.view[phgr13_locate::G1_ELEMENTS]),
                           (u32)N, (u32)N, g2);
        hipLaunchKernelGGL(k_ec_scale<Fp2s>, dim3(nblocks(2 * N)), dim3(256), 0, c->stream, g2, (u32)N, rho_m, ~0ull);
        for (int l = 0; l + 1 < t->nl; l++) {
            const u64 n = t->size[l], h = t->size[l + 1];
            hipLaunchKernelGGL(k_g2_pair_sums, dim3(nblocks(2 * h)), dim3(256), 0, c->stream, (const Xyzz<Fp2>*)(g2 + t->off[l]), (u32)n, 1u, 0u, g2 + t->off[l + 1], 0u);
        }
        t->wss = g2;
    }
    // the scalar tree and ys_io for sum_j t_S,j ys_j
    if (div) {
        u32* rows = (u32*)c->lc_rows.p;
        if (storage_wait_ready(io->st, c->stream) || storage_wait_ready(vk->ys_io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
        hipLaunchKernelGGL(k_fr_locate_rows, dim3(nblocks(N * cols)), dim3(256), 0, c->stream, scalars_ptr(keep.rho), rho_m, scalars_ptr(io), (u32)N, (u32)diff, rows);
        for (int l = 0; l + 1 < t->nl; l++)
            hipLaunchKernelGGL(k_fr_row_pair_sums, dim3(nblocks(t->size[l + 1] * cols)), dim3(256), 0, c->stream, (const u32*)(rows + 8 * cols * t->off[l]),
                               (u32)t->size[l], (u32)cols, rows + 8 * cols * t->off[l + 1]);
        hipLaunchKernelGGL(k_ec_from_affine<Fp>, dim3(nblocks(diff)), dim3(256), 0, c->stream, (const Affine<Fp>*)points_ptr(vk->ys_io), (u32)diff, (u32)diff,
                           (Xyzz<Fp>*)c->lc_iolp.p);
        t->rows = rows;
        t->ysx = (const Xyzz<Fp>*)c->lc_iolp.p;
    }
    HIP_TRY(hipGetLastError());
    t->g1 = g1;
    t->f = (const pairing_dev::Fp12*)c->lc_f12.p;
    return PS_OK;
}

// E_c(S) for the K nodes idx[] of level l and the equations c of pmask[k] (a subset of the trees' mask): fmask[k] = those
// that fail; *products counts the (set, equation) pairs evaluated
static int phgr13_locate_check_sets(ps_ctx* c, const std::string& fn, const ps_phgr13_vk* vk, const Phgr13Trees& t, const PvbKeep& keep, int l, const u32* idx,
                                    const uint8_t* pmask, size_t K, uint8_t* fmask, u32* products) {
    typedef pairing_dev::Fp12 D12;
    using namespace phgr13_locate;
    constexpr size_t WX = sizeof(Xyzz<Fp>) / 4, WX2 = sizeof(Xyzz<Fp2>) / 4, W12 = sizeof(D12) / 4, WA2 = sizeof(Affine<Fp2>) / 4;
    const size_t diff = t.diff, cols = diff + 1, nseg = t.nseg;
    // the sets E0 is tested on: they alone take part in the device's loops
    std::vector<u32> sets0;  // positions k
    for (size_t k = 0; k < K; k++)
        if (pmask[k] & 1u) sets0.push_back((u32)k);
    const size_t K0 = sets0.size(), K0d = diff ? K0 : 0, n1 = nseg * K + K0d + K0d * diff;
    // index words: the nodes of the K sets | those of the K0 sets | the elements' nodes in the G1 trees, element-major | the
    // P nodes, set-major
    std::vector<u32> hidx(K + K0 + nseg * K + K0d * diff);
    u32 *h_all = hidx.data(), *h_div = h_all + K, *h_el = h_div + K0, *h_p = h_el + nseg * K;
    for (size_t k = 0; k < K; k++) h_all[k] = idx[k];
    for (size_t k = 0; k < K0; k++) h_div[k] = idx[sets0[k]];
    for (size_t s = 0; s < nseg; s++)
        for (size_t k = 0; k < K; k++) h_el[s * K + k] = (u32)(segment_node(t.size, t.off, l, t.segs, s) + idx[k]);
    for (size_t k = 0; k < K0d; k++)
        for (size_t j = 0; j < diff; j++) h_p[k * diff + j] = (u32)(segment_node(t.size, t.off, l, t.segs, nseg + j) + h_div[k]);
    // one workspace: index words | F_S | the loops' values | the sets' products | t_S plain, Montgomery | two buffers of
    // K0 x diff points | ws_io K0 times | G1 points to normalise (elements, sum_j t_S,j ys_j, P_S,k) and their chain products
    // | the same, affine | wss_S, chain products | affine
    LocateCarve work;
    const size_t o_idx = work.take(4 * hidx.size()), o_f = work.take(sizeof(D12) * K0), o_m = work.take(sizeof(D12) * K0d * diff),
                 o_fs = work.take(sizeof(D12) * K0), o_t = work.take(32 * K0d * diff), o_tm = work.take(sizeof(Fr) * K0d * diff),
                 o_p0 = work.take(sizeof(Xyzz<Fp>) * K0d * diff), o_p1 = work.take(sizeof(Xyzz<Fp>) * K0d * diff),
                 o_ws = work.take(sizeof(Affine<Fp2>) * K0d * diff), o_n = work.take(batch_affine_tmp_bytes(n1, sizeof(Xyzz<Fp>))),
                 o_a = work.take(sizeof(Affine<Fp>) * n1), o_n2 = work.take(batch_affine_tmp_bytes(K, sizeof(Xyzz<Fp2>))),
                 o_a2 = work.take(sizeof(Affine<Fp2>) * K), total = work.total();
    if (c->lc_work.ensure(total))
        return fail(PS_ERR_HIP, fn + ": no device memory for a round of " + std::to_string(K) + " sets (" + std::to_string(total) + " bytes)");
    char* w = (char*)c->lc_work.p;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(w + o_idx, hidx.data(), 4 * hidx.size(), hipMemcpyHostToDevice, c->stream));
    const u32 *d_all = (const u32*)(w + o_idx), *d_div = d_all + K, *d_el = d_div + K0, *d_p = d_el + nseg * K;
    Xyzz<Fp>* norm = (Xyzz<Fp>*)(w + o_n);
    Affine<Fp>* aff = (Affine<Fp>*)(w + o_a);
    locate_gather(c, t.g1, d_el, nseg * K, WX, 0, WX, norm);
    u32 simds = 0;
    int rc = ctx_simds(c, &simds);
    if (rc) return rc;
    if (K0) {
        locate_gather(c, t.f + f_level_base(t.off, l, diff), d_div, K0, W12, 0, W12, w + o_f);
        if (diff) {
            // sum_j t_S,j ys_j
            locate_gather(c, t.rows + 8 * cols * t.off[l], d_div, K0, 8 * cols, 8, 8 * diff, w + o_t);
            hipLaunchKernelGGL(k_fr_to_mont, dim3(nblocks(K0 * diff)), dim3(256), 0, c->stream, (Fr*)(w + o_tm), (const u32*)(w + o_t), (u64)(K0 * diff));
            Xyzz<Fp>*src = (Xyzz<Fp>*)(w + o_p0), *dst = (Xyzz<Fp>*)(w + o_p1);
            segment_sums(c, t.ysx, diff, K0, (const Fr*)(w + o_tm), &src, &dst);
            locate_gather(c, src, nullptr, K0, WX * diff, 0, WX, norm + nseg * K);
            // P_S,k, and ws_io once per set
            locate_gather(c, t.g1, d_p, K0 * diff, WX, 0, WX, norm + nseg * K + K0);
            if (storage_wait_ready(vk->ws_io->st, c->stream)) return fail(PS_ERR_HIP, fn + ": event wait failed");
            locate_gather(c, points_ptr(vk->ws_io), nullptr, K0, 0, 0, WA2 * diff, w + o_ws);
        }
    }
    if (n1) batch_to_affine<Fp>(c->stream, (char*)norm, n1, (char*)aff, (u32)sizeof(Affine<Fp>));
    if (K0) {
        if (diff) {
            const u32 lpw = pairing_dev::spread_lanes(K0 * diff, simds);
            hipLaunchKernelGGL(k_miller_batch, dim3((unsigned)((K0 * diff + lpw - 1) / lpw)), dim3(64), 0, c->stream, (const Affine<Fp>*)(aff + nseg * K + K0),
                               (const Affine<Fp2>*)(w + o_ws), (u32)(K0 * diff), lpw, (D12*)(w + o_m));
        }
        const u32 lpw = pairing_dev::spread_lanes(K0, simds);
        hipLaunchKernelGGL(k_f12_segment_products, dim3((unsigned)((K0 + lpw - 1) / lpw)), dim3(64), 0, c->stream, (const D12*)(w + o_f), (const D12*)(w + o_m), (u32)K0,
                           (u32)diff, lpw, (D12*)(w + o_fs));
    }
    if (t.g2()) {
        locate_gather(c, t.wss + t.off[l], d_all, K, WX2, 0, WX2, w + o_n2);
        batch_to_affine<Fp2>(c->stream, w + o_n2, K, w + o_a2, (u32)sizeof(Affine<Fp2>));
    }
    HIP_TRY(hipGetLastError());
    std::vector<D12> hf(K0);
    std::vector<Affine<Fp>> ha(nseg * K + K0d);
    std::vector<Affine<Fp2>> hw(t.g2() ? K : 0);
    if (K0) HIP_TRY(hipMemcpyAsync(hf.data(), w + o_fs, sizeof(D12) * K0, hipMemcpyDeviceToHost, c->stream));
    if (!ha.empty()) HIP_TRY(hipMemcpyAsync(ha.data(), aff, sizeof(Affine<Fp>) * ha.size(), hipMemcpyDeviceToHost, c->stream));
    if (!hw.empty()) HIP_TRY(hipMemcpyAsync(hw.data(), w + o_a2, sizeof(Affine<Fp2>) * K, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    locate_lap(&c->plc_ms[1], &t0);
    // the host's share: the loops of every tested (set, equation), then their products and final exponentiations
    using pairing_dev::neg_g1;
    const Affine<Fp2> g2 = generator((const Fp2*)0);
    const Affine<Fp> none{f_zero((const Fp*)0), f_zero((const Fp*)0)};
    std::vector<long> pos0(K, -1);
    for (size_t k = 0; k < K0; k++) pos0[sets0[k]] = (long)k;
    auto el = [&](int e, size_t k) { return ha[(size_t)t.slot[e] * K + k]; };
    struct Loop { Affine<Fp> p; Affine<Fp2> q; };
    struct Test { u32 set; int eq; size_t first; int loops; };
    std::vector<Loop> loops;
    std::vector<Test> tests;
    for (size_t k = 0; k < K; k++)
        for (int e = 0; e < EQUATIONS; e++) {
            if (!((pmask[k] >> e) & 1u)) continue;
            tests.push_back({(u32)k, e, loops.size(), host_loops(e)});
            switch (e) {
            case 0:
                loops.push_back({neg_g1(el(HS, k)), keep.yts});
                loops.push_back({neg_g1(affine_sum<Fp>(el(YSS, k), diff ? ha[nseg * K + (size_t)pos0[k]] : none)), g2});
                break;
            case 1:
                loops.push_back({el(VASS, k), g2});
                loops.push_back({neg_g1(el(VSS, k)), keep.av});
                break;
            case 2:
                loops.push_back({el(WASS, k), g2});
                loops.push_back({neg_g1(keep.aw), hw[k]});
                break;
            case 3:
                loops.push_back({el(YASS, k), g2});
                loops.push_back({neg_g1(el(YSS, k)), keep.ay});
                break;
            default:
                loops.push_back({el(GZ, k), keep.gamma});
                loops.push_back({neg_g1(affine_sum<Fp>(el(VSS, k), el(YSS, k))), keep.bgamma2});
                loops.push_back({neg_g1(keep.bgamma), hw[k]});
            }
        }
    std::vector<pairing::Fp12> val(loops.size());
    locate_parallel(loops.size(), [&](size_t j) { val[j] = pairing::miller(affine_to_host<Fp>(loops[j].p), affine_to_host<Fp2>(loops[j].q)); });
    std::vector<uint8_t> holds(tests.size());
    locate_parallel(tests.size(), [&](size_t i) {
        const Test& ts = tests[i];
        pairing::Fp12 f = ts.eq == 0 ? f12_to_host(hf[(size_t)pos0[ts.set]]) : pairing::f12_one();
        for (int j = 0; j < ts.loops; j++) f = pairing::f12_mul(f, val[ts.first + j]);
        holds[i] = pairing::f12_eq(pairing::final_exp(f), pairing::f12_one()) ? 1 : 0;
    });
    memset(fmask, 0, K);
    for (size_t i = 0; i < tests.size(); i++)
        if (!holds[i]) fmask[tests[i].set] |= (uint8_t)(1u << tests[i].eq);
    *products += (u32)tests.size();
    locate_lap(&c->plc_ms[2], &t0);
    return PS_OK;
}

static int phgr13_locate_descent(ps_ctx* c, const std::string& fn, const ps_phgr13_vk* vk, const ps_scalars* io, size_t N, u32 root, const PvbKeep& keep,
                                 uint8_t* valid, uint8_t* failed, size_t* ninvalid) {
    memset(valid, 1, N);
    if (failed) memset(failed, 0, N);
    ps_phgr13_locate_info& info = c->plc_info;
    Phgr13Trees t;
    if (N > 1) {  // (one proof: the root is the leaf, the descent reads no tree)
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = phgr13_locate_build_trees(c, fn, vk, io, N, root, keep, &t)) return rc;
        if (c->timing) (void)hipStreamSynchronize(c->stream);
        locate_lap(&c->plc_ms[0], &t0);
    }
    std::vector<u32> leaves;
    std::vector<uint8_t> masks;
    auto check = [&](int l, const u32* idx, const uint8_t* pmask, size_t K, uint8_t* fmask) {
        return phgr13_locate_check_sets(c, fn, vk, t, keep, l, idx, pmask, K, fmask, &info.products);
    };
    if (int rc = locate_bisect(N, (uint8_t)root, locate_per_pass(t.diff), check, &leaves, &masks, &info.checks, &info.levels)) return rc;
    for (size_t k = 0; k < leaves.size(); k++) {  // level 0: a failing leaf is an invalid proof
        valid[leaves[k]] = 0;
        if (failed) failed[leaves[k]] = masks[k];
        info.failed |= masks[k];
    }
    *ninvalid = info.invalid = (u32)leaves.size();
    return PS_OK;
}

extern "C" int ps_phgr13_verify_batch_locate(ps_ctx* c, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proofs, size_t nproofs,
                                             const uint8_t* rho_be32, uint8_t* valid, uint8_t* failed, size_t* ninvalid) {
    const std::string fn = "ps_phgr13_verify_batch_locate";
    if (!c || !vk || !io || !ninvalid || !vk->vs_io || !vk->ws_io || !vk->ys_io || (nproofs && (!proofs || !rho_be32 || !valid)))
        return fail(PS_ERR_ARG, fn + ": NULL argument");
    *ninvalid = 0;
    c->pvb_info = ps_phgr13_batch_info{0, 0, {0, 0}};
    c->plc_info = ps_phgr13_locate_info{0, 0, 0, 0, 0, {0, 0, 0}};
    for (float& v : c->plc_ms) v = 0;
    int ok = 0;
    PvbKeep keep;
    int rc = phgr13_verify_batch_impl(c, fn, vk, io, proofs, nproofs, rho_be32, &ok, &keep);
    Scope scope(c->stream);  // what a rejected batch handed over is this call's from here on, on every way out
    scope.in_flight();       // ... and a failed descent leaves copies from this call's vectors behind: wait for them
    for (ps_points* p : keep.view) *scope.points() = p;
    *scope.points() = keep.g1;
    *scope.points() = keep.rgv;
    *scope.scalars() = keep.rho;
    *scope.scalars() = keep.iot;
    if (rc || nproofs == 0) return rc;
    c->plc_info.checks = 1;
    c->plc_info.products = phgr13_locate::EQUATIONS;
    if (ok) {
        memset(valid, 1, nproofs);
        if (failed) memset(failed, 0, nproofs);
        return scope.finish(PS_OK);
    }
    rc = phgr13_locate_descent(c, fn, vk, io, nproofs, c->pvb_info.failed, keep, valid, failed, ninvalid);
    if (rc) *ninvalid = 0;
    return scope.finish(rc);
}

extern "C" int ps_phgr13_verify_batch_locate_info(ps_ctx* c, ps_phgr13_locate_info* out) {
    if (!c || !out) return fail(PS_ERR_ARG, "ps_phgr13_verify_batch_locate_info: NULL argument");
    *out = c->plc_info;
    return PS_OK;
}

// Wall clock of the descent of the last ps_phgr13_verify_batch_locate on the context: [0] building the trees (enqueued only,
// unless ps_ctx_set_timing is on), [1] the rounds' device part (gathers, sums, loops, normalisation, download, up to the
// synchronisation), [2] their host part (Miller loops, final exponentiations).  Measurement hook, not in the header.
extern "C" int ps_debug_phgr13_verify_locate_ms(ps_ctx* c, float* ms) {
    if (!c || !ms) return fail(PS_ERR_ARG, "ps_debug_phgr13_verify_locate_ms: NULL argument");
    for (int i = 0; i < 3; i++) ms[i] = c->plc_ms[i];
    return PS_OK;
}
