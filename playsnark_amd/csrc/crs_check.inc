// Is a key what its powers-of-tau string makes of it?  Without making it again (included by capi.hip after srs_phase1.inc):
//   ps_points_lagrange_check         is `lagr` the Lagrange form of `mono` (ps_points_monomial_to_lagrange)?
//   ps_groth16_crs_check_from_srs    is `key` ps_groth16_setup_from_srs(q, srs) with SOME (delta, gamma) folded in?
// Every key element is a fixed linear function of the string's points, so a random linear combination of a key array equals
// ONE sum over the monomial string whose coefficients come from an interpolation over SCALARS (quotient.hpp, a millisecond)
// instead of a conversion over group elements (lagrange.inc, seconds).  Everything is the existing machinery -- the row SpMV
// and the interpolations of the quotient, ps_poly_mul, the sums, the host pairing of pairing.inc -- but the comparison of two
// resident arrays, which has a kernel here so that no array crosses PCIe.

// *flag = 1 when the two word arrays differ anywhere (stored points are canonical: equal points <=> equal words).  Grid-stride
// over 16-byte words; every thread that sees a difference stores the same 1.
__global__ void __launch_bounds__(256) k_words_differ(const uint4* __restrict__ a, const uint4* __restrict__ b, u64 nq, u32* __restrict__ flag) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u32 diff = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
        const uint4 x = a[i], y = b[i];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    if (diff) *flag = 1;
}
static_assert(sizeof(Affine<Fp>) % 16 == 0 && sizeof(Affine<Fp2>) % 16 == 0, "k_words_differ reads points as 16-byte words");

// Enqueues the comparison of a[0..n) with b[first..first + n) on c->stream; a difference sets c->d_flag (the caller clears it
// before the first comparison and reads it after the last).
static int points_differ_launch(ps_ctx* c, const ps_points* a, const ps_points* b, size_t first, size_t n) {
    if (storage_wait_ready(a->st, c->stream) || storage_wait_ready(b->st, c->stream)) return fail(PS_ERR_HIP, "comparing two point arrays: event wait failed");
    if (!n) return PS_OK;
    const size_t pb = point_bytes(a->group);
    const u64 nq = (u64)n * pb / 16;
    hipLaunchKernelGGL(k_words_differ, dim3((unsigned)std::min<u64>(nblk(nq), 4096)), dim3(256), 0, c->stream, (const uint4*)points_ptr(a),
                       (const uint4*)((const char*)points_ptr(b) + first * pb), nq, c->d_flag);
    return PS_OK;
}

// The coefficients c of the polynomial that takes the values w[0..cnt) on the nodes 1..n (nodes = 0, cnt = n) or n+1..2n-1
// (nodes = 1, cnt = n - 1): sum_j w_j l_j(X) = sum_i c_i X^i, so sum_j w_j {l_j(x) P} = sum_i c_i {x^i P} whatever x and P are.
// q->y[0] holds the values in Montgomery form (as for a solution's L.s); returns with the vector complete.
static int interpolate_weights(ps_ctx* c, const ps_qap* q, const ps_scalars* w, int nodes, ps_scalars** out) {
    const size_t n = q->n, cnt = nodes ? n - 1 : n;
    hipStream_t st = c->stream;
    if (storage_wait_ready(w->st, st)) return fail(PS_ERR_HIP, "interpolating the weights: event wait failed");
    hipLaunchKernelGGL(k_fr_to_mont, dim3(nblk(cnt)), dim3(256), 0, st, q->y[0], scalars_ptr(w), (u64)cnt);
    const QapTables& qt = q->qt;
    hipError_t e = nodes ? interpolate_on_nodes(*ctx_tabs(c), st, qt, q->y[0], cnt, qt.np_h, qt.lognp_h, qt.vhat_h, qt.zhat_h, n)
                         : interpolate_on_1_to_n(*ctx_tabs(c), st, qt, q->y[0]);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("interpolating the weights: ") + hipGetErrorString(e));
    int rc = scalars_from_mont(c, qt.data, cnt, out);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return PS_OK;
}

// Independent sums through the launch / finish queue, PS_MSM_QUEUE of them pending.  An error drains the queue.
struct SumJob { const ps_points* pts; const ps_scalars* sc; uint8_t* out; };
static int sums_run(ps_ctx* c, const std::vector<SumJob>& jobs) {
    size_t launched = 0, done = 0;
    int rc = PS_OK;
    while (!rc && done < jobs.size()) {
        while (!rc && launched < jobs.size() && launched - done < PS_MSM_QUEUE)
            if (!(rc = ps_msm_launch(c, jobs[launched].pts, jobs[launched].sc))) launched++;
        if (!rc) rc = ps_msm_finish(c, jobs[done++].out);
    }
    if (rc) {
        KeepError keep;
        uint8_t sink[192];
        while (c->q_len) (void)ps_msm_finish(c, sink);
    }
    return rc;
}

// The first nw weights as a device vector, validated: canonical (PS_ERR_ENCODING), at least nw of them (PS_ERR_LENGTH)
static int check_weights(ps_ctx* c, const char* who, const uint8_t* rho_be32, size_t nrho, size_t nw, ps_scalars** out) {
    if (nrho < nw || (nw && !rho_be32))
        return fail(PS_ERR_LENGTH, std::string(who) + ": " + std::to_string(nrho) + " weights where " + std::to_string(nw) + " are needed");
    for (size_t i = 0; i < nw; i++) {
        u32 w[8];
        if (!be32_to_words(w, rho_be32 + 32 * i)) return fail(PS_ERR_ENCODING, std::string(who) + ": rho[" + std::to_string(i) + "] is not below r");
    }
    return ps_scalars_upload(c, rho_be32, nw, out);
}

extern "C" int ps_points_lagrange_check(ps_ctx* c, const ps_qap* q, const ps_points* mono, const ps_points* lagr, int nodes, const uint8_t* rho_be32,
                                        size_t nrho, int* ok) {
    const char* who = "ps_points_lagrange_check";
    if (!c || !q || !mono || !lagr || !ok) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    *ok = 0;
    if (nodes != 0 && nodes != 1) return fail(PS_ERR_ARG, std::string(who) + ": nodes must be 0 (1..n) or 1 (n+1..2n-1)");
    if (q->n < 2) return fail(PS_ERR_ARG, std::string(who) + ": needs at least 2 gates");
    if (mono->group != lagr->group) return fail(PS_ERR_ARG, std::string(who) + ": the two arrays are of different groups");
    if (c->q_len) return fail(PS_ERR_ARG, std::string(who) + ": sums are pending on this context (ps_msm_finish them first)");
    const size_t cnt = nodes ? q->n - 1 : q->n;
    for (const ps_points* p : {mono, lagr})
        if (p->n != cnt)  // the arrays are polynomial bases of exactly that degree bound (algebra.go:350-352's rule)
            return fail(PS_ERR_LENGTH, "mismatch of length between poly " + std::to_string(cnt) + " and blinded eval points " + std::to_string(p->n));
    HIP_TRY(hipSetDevice(c->device));
    Scope keep;
    ps_scalars** rho = keep.scalars();
    int rc = check_weights(c, who, rho_be32, nrho, cnt, rho);
    if (rc) return rc;
    ps_scalars** coef = keep.scalars();
    if ((rc = interpolate_weights(c, q, *rho, nodes, coef))) return rc;
    uint8_t by_lagr[192], by_mono[192];
    if ((rc = sums_run(c, {{lagr, *rho, by_lagr}, {mono, *coef, by_mono}}))) return rc;
    *ok = memcmp(by_lagr, by_mono, wire_bytes(mono->group)) == 0;
    return PS_OK;
}

// e(a1, b1) == e(a2, b2) on a host thread of its own (pairing.inc: 11 ms), for encodings this file has validated or made: the
// G2 arguments are generators or tested fixed points of the key, the G1 arguments sums over arrays that were tested or vouched
// for.  The device route of pairing_pair_equal costs 50 ms a call whatever the size -- two Miller loops are two lanes -- and
// four of them in a row were 0.2 s of this check at every size: 220 -> 28 ms at 2^16 gates (profiles/crs_check_from_srs.txt).
static std::future<bool> pair_equal_host(const uint8_t* a1, const uint8_t* b1, const uint8_t* a2, const uint8_t* b2) {
    Affine<Fp> p1, p2;
    Affine<Fp2> q1, q2;
    const bool read = read_affine(p1, a1) && read_affine(q1, b1) && read_affine(p2, a2) && read_affine(q2, b2);
    return std::async(std::launch::async, [=] { return read && product_is_one({{p1, q1}, {pairing_dev::neg_g1(p2), q2}}); });
}

extern "C" int ps_groth16_crs_check_from_srs(ps_ctx* c, const ps_qap* q, const ps_groth16_srs* srs, const ps_groth16_crs* key, const uint8_t* rho_be32,
                                             size_t nrho, int check_subgroup, int* ok) {
    const char* who = "ps_groth16_crs_check_from_srs";
    if (!c || !q || !srs || !key || !ok) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    *ok = 0;
    if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return fail(PS_ERR_ARG, std::string(who) + ": the string lacks an array");
    if (!srs_groups_ok(srs)) return fail(PS_ERR_ARG, std::string(who) + ": tau_g2 is a G2 array, the other three are G1 arrays");
    if (!key->xi || !key->xi2 || !key->io_lp || !key->nio_lp || !key->xi_t) return fail(PS_ERR_ARG, std::string(who) + ": the key lacks an array");
    const size_t n = q->n, m = q->m, diff = q->m - q->nio;
    if (n < 2) return fail(PS_ERR_ARG, std::string(who) + ": needs at least 2 gates");
    // the key's arrays with their groups and the lengths a key of this circuit has; lxi, lxi2, lxi_t are optional
    const struct { const ps_points* p; int group; size_t want; } arrays[8] = {
        {key->xi, PS_G1, n},     {key->xi2, PS_G2, n}, {key->io_lp, PS_G1, diff}, {key->nio_lp, PS_G1, m - diff},
        {key->xi_t, PS_G1, n - 1}, {key->lxi, PS_G1, n}, {key->lxi2, PS_G2, n},   {key->lxi_t, PS_G1, n - 1}};
    for (const auto& a : arrays)
        if (a.p && a.p->group != a.group) return fail(PS_ERR_ARG, std::string(who) + ": xi2 and lxi2 are G2 arrays, the key's other arrays are G1 arrays");
    if (c->q_len) return fail(PS_ERR_ARG, std::string(who) + ": sums are pending on this context (ps_msm_finish them first)");
    const struct { const ps_points* p; size_t want; const char* name; } lens[4] = {
        {srs->tau_g1, 2 * n - 1, "tau_g1"}, {srs->tau_g2, n, "tau_g2"}, {srs->alpha_tau_g1, n, "alpha_tau_g1"}, {srs->beta_tau_g1, n, "beta_tau_g1"}};
    for (const auto& l : lens)
        if (l.p->n != l.want)  // as ps_groth16_setup_from_srs
            return fail(PS_ERR_LENGTH, std::string("mismatch of length between ") + l.name + " " + std::to_string(l.p->n) + " and the " + std::to_string(l.want) +
                                           " powers a circuit of " + std::to_string(n) + " gates needs");
    HIP_TRY(hipSetDevice(c->device));
    Scope keep;
    const size_t nw = std::max(m, n);
    ps_scalars** rho = keep.scalars();
    int rc = check_weights(c, who, rho_be32, nrho, nw, rho);
    if (rc) return rc;
    for (const auto& a : arrays)
        if (a.p && a.p->n != a.want) return PS_OK;  // no key of this circuit

    // ---- the fixed points ----
    uint8_t a0[96], b0[96], gen1[96], gen2[192];
    if ((rc = ps_points_download(c, srs->alpha_tau_g1, 0, 1, a0))) return rc;
    if ((rc = ps_points_download(c, srs->beta_tau_g1, 0, 1, b0))) return rc;
    if (memcmp(key->alpha, a0, 96) || memcmp(key->beta, b0, 96) || memcmp(key->beta2, srs->beta_g2, 192)) return PS_OK;
    {  // delta, delta2, gamma: on the curve (an error otherwise), not the identity and in the subgroup (a rejection): [r]P on host threads
        Affine<Fp> delta;
        Affine<Fp2> delta2, gamma;
        if (!read_affine(delta, key->delta) || !read_affine(delta2, key->delta2) || !read_affine(gamma, key->gamma))
            return fail(PS_ERR_ENCODING, std::string(who) + ": delta, delta2 or gamma is not a canonical point on the curve");
        if (((key->delta[0] | key->delta2[0] | key->gamma[0]) & 0x40) || !all_in_subgroup({&delta}, {&delta2, &gamma})) return PS_OK;
    }
    generator_bytes<Fp>(gen1);
    generator_bytes<Fp2>(gen2);
    // one delta in both groups: e(delta, G2) = e(G1, delta2), beside everything the device does below
    std::future<bool> delta_eq = pair_equal_host(key->delta, gen2, gen1, key->delta2);
    if (check_subgroup)
        for (const auto& a : arrays) {
            int in = 0;
            if (a.p && (rc = ps_points_check_subgroup(c, a.p, &in))) return rc;
            if (a.p && !in) return PS_OK;
        }

    // ---- xi, xi2: the string's first n powers, compared where they are ----
    {
        u32 differ = 0;
        HIP_TRY(hipMemsetAsync(c->d_flag, 0, 4, c->stream));
        if ((rc = points_differ_launch(c, key->xi, srs->tau_g1, 0, n))) return rc;
        if ((rc = points_differ_launch(c, key->xi2, srs->tau_g2, 0, n))) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&differ, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (differ) return PS_OK;
    }

    // ---- the scalar side: every coefficient vector the sums below run over ----
    ps_scalars **r_n = keep.scalars(), **r_n1 = keep.scalars(), **r_io = keep.scalars(), **r_nio = keep.scalars();
    if ((rc = ps_scalars_slice(*rho, 0, n, r_n)) || (rc = ps_scalars_slice(*rho, 0, n - 1, r_n1)) || (rc = ps_scalars_slice(*rho, 0, diff, r_io)) ||
        (rc = ps_scalars_slice(*rho, diff, m - diff, r_nio)))
        return rc;
    const bool lagrange = key->lxi || key->lxi2, lagrange_t = key->lxi_t != nullptr;
    ps_scalars **c0 = keep.scalars(), **c1 = keep.scalars(), **zs = keep.scalars(), **rz = keep.scalars();
    if (lagrange && (rc = interpolate_weights(c, q, *r_n, 0, c0))) return rc;
    if (lagrange_t && (rc = interpolate_weights(c, q, *r_n1, 1, c1))) return rc;
    // rho * z, 2n - 1 coefficients: sum_i rho_i X^i z(X)
    if ((rc = scalars_from_mont(c, q->qt.z, n + 1, zs)) || (rc = ps_poly_mul(c, *r_n1, *zs, rz))) return rc;
    // rho restricted to the IO variables and to the rest; per part the interpolants of L rho_S, R rho_S, O rho_S on 1..n
    ps_scalars** lin[2][3];
    for (int part = 0; part < 2; part++) {
        const size_t first = part ? diff : 0, cnt = part ? m - diff : diff;
        ps_scalars** rs = keep.scalars();
        if ((rc = scalars_alloc(c, m, rs))) return rc;
        HIP_TRY(hipMemsetAsync((*rs)->st->p, 0, 32 * m, c->stream));
        if (cnt)
            HIP_TRY(hipMemcpyAsync((u32*)(*rs)->st->p + 8 * first, scalars_ptr(*rho) + 8 * first, 32 * cnt, hipMemcpyDeviceToDevice, c->stream));
        for (int which = 0; which < 3; which++) {
            lin[part][which] = keep.scalars();
            if ((rc = ps_qap_interpolate(c, q, *rs, which, lin[part][which]))) return rc;
        }
    }

    // ---- the sums: first those that share a scalar vector (one digit sort each), then the lone ones, PS_MSM_QUEUE at a time ----
    uint8_t by_c0[2][192], by_rho[2][192], xt_rho[96], lxt_rho[96], lxt_c1[96], xt_rz[96], io_rho[96], nio_rho[96], e[2][3][96];
    if (lagrange) {
        const ps_points *mono[2], *lagr[2];
        uint8_t *out_m[2], *out_l[2];
        size_t k = 0;
        if (key->lxi) { mono[k] = key->xi; lagr[k] = key->lxi; out_m[k] = by_c0[0]; out_l[k] = by_rho[0]; k++; }
        if (key->lxi2) { mono[k] = key->xi2; lagr[k] = key->lxi2; out_m[k] = by_c0[1]; out_l[k] = by_rho[1]; k++; }
        if ((rc = ps_msm_multi(c, mono, k, *c0, out_m)) || (rc = ps_msm_multi(c, lagr, k, *r_n, out_l))) return rc;
        if (key->lxi && memcmp(by_c0[0], by_rho[0], 96)) return PS_OK;
        if (key->lxi2 && memcmp(by_c0[1], by_rho[1], 192)) return PS_OK;
    }
    {
        const ps_points* over_rho[2] = {key->xi_t, key->lxi_t};
        uint8_t* out[2] = {xt_rho, lxt_rho};
        if ((rc = ps_msm_multi(c, over_rho, lagrange_t ? 2 : 1, *r_n1, out))) return rc;
    }
    ps_points** t1_n = keep.points();
    if ((rc = ps_points_slice(srs->tau_g1, 0, n, t1_n))) return rc;
    std::vector<SumJob> jobs = {{srs->tau_g1, *rz, xt_rz}, {key->io_lp, *r_io, io_rho}, {key->nio_lp, *r_nio, nio_rho}};
    if (lagrange_t) jobs.push_back({key->xi_t, *c1, lxt_c1});
    const ps_points* base[3] = {srs->beta_tau_g1, srs->alpha_tau_g1, *t1_n};  // L goes with beta, R with alpha, O with 1
    for (int part = 0; part < 2; part++)
        for (int which = 0; which < 3; which++) jobs.push_back({base[which], *lin[part][which], e[part][which]});
    if ((rc = sums_run(c, jobs))) return rc;

    // ---- lxi_t against xi_t: both carry 1 / delta ----
    if (lagrange_t && memcmp(lxt_rho, lxt_c1, 96)) return PS_OK;
    // ---- io_lp against gamma, nio_lp against delta2: E_S = <cU, B> + <cV, A> + <cW, T1> ----
    uint8_t e_io[96], e_nio[96];
    if ((rc = ps_points_sum(PS_G1, e[0][0], 3, e_io)) || (rc = ps_points_sum(PS_G1, e[1][0], 3, e_nio))) return rc;
    // Each equation is a product of its own (two errors cannot cancel), each on a host thread of its own:
    //   e(sum rho_i xi_t[i], delta2) = e((rho z)(x) G1, G2);   e(sum rho_i io_lp[i], gamma) = e(E_io, G2);
    //   e(sum rho_i nio_lp[i - diff], delta2) = e(E_nio, G2)
    std::future<bool> eqs[3] = {pair_equal_host(xt_rho, key->delta2, xt_rz, gen2), pair_equal_host(io_rho, key->gamma, e_io, gen2),
                                pair_equal_host(nio_rho, key->delta2, e_nio, gen2)};
    bool all = delta_eq.get();
    for (auto& f : eqs) all = f.get() && all;
    *ok = all ? 1 : 0;
    return PS_OK;
}
