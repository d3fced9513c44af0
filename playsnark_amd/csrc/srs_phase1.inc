// Phase 1 of a Groth16 ceremony: making and checking the powers-of-tau string ps_groth16_setup_from_srs starts from (included
// by capi.hip after srs_setup.inc):
//   ps_scalars_powers            out[i] = c s^i                         (k_fr_powers of quotient.hpp, the trusted setups' kernel)
//   ps_groth16_srs_contribute    tau *= t, alpha *= a, beta *= b, and the contributor's public share
//   ps_groth16_srs_check         is the string {x^i G1}, {x^i G2}, {alpha x^i G1}, {beta x^i G1}, beta G2 for SOME x, alpha, beta?
//   ps_groth16_srs_check_update  ... and was it made from `before` by the holder of `share`?
// Nothing here needs a kernel of its own: the power sequence is the one ps_groth16_setup commits to, the multiplications are the
// per-index form of k_ec_scale (lagrange.inc, points_scale_each), the sums ps_msm_multi over shifted views, the tests
// ps_points_check_subgroup and ps_pairing_product_is_one.

// out[i] = c s^i (Montgomery form), i < n < 2^32, enqueued on c->stream: the host squares s 31 times, thread i multiplies the
// entries its index bits select -- none for i = 0, so s^0 = 1 also for s = 0
static void fr_powers_launch(ps_ctx* c, const Fr& s_mont, const Fr& c_mont, size_t n, Fr* out) {
    FrPow2Table tab;
    tab.p[0] = s_mont;
    for (int k = 1; k < 32; k++) tab.p[k] = fr_mul(tab.p[k - 1], tab.p[k - 1]);
    hipLaunchKernelGGL(k_fr_powers, dim3(nblk(n)), dim3(256), 0, c->stream, out, tab, c_mont, (u64)n);
}
// a canonical scalar in Montgomery form; false: not below r
static bool fr_mont_from_canonical_be32(Fr* out, const uint8_t* be) {
    u32 w[8];
    if (!be32_to_words(w, be)) return false;
    *out = fr_to_mont(fr_from_words8(w));
    return true;
}

extern "C" int ps_scalars_powers(ps_ctx* c, const uint8_t* s_be32, const uint8_t* c_be32, size_t n, ps_scalars** out) {
    if (!c || !s_be32 || !c_be32 || !out) return fail(PS_ERR_ARG, "ps_scalars_powers: NULL argument");
    *out = nullptr;
    Fr s, k;
    if (!fr_mont_from_canonical_be32(&s, s_be32) || !fr_mont_from_canonical_be32(&k, c_be32))
        return fail(PS_ERR_ENCODING, "ps_scalars_powers: s and c must be below r");
    if ((unsigned long long)n >= (1ull << 32)) return fail(PS_ERR_ARG, "ps_scalars_powers: 2^32 powers or more");
    HIP_TRY(hipSetDevice(c->device));
    Scope scope(c->stream);
    Fr* pw = nullptr;
    hipError_t e = scope.device(&pw, n);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_scalars_powers: hipMalloc: ") + hipGetErrorString(e));
    if (n) fr_powers_launch(c, s, k, n, pw);
    int rc = scalars_from_mont(c, pw, n, scope.result(out));
    if (rc) return rc;
    if ((e = hipGetLastError()) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_scalars_powers: kernels: ") + hipGetErrorString(e));
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_scalars_powers: run: ") + hipGetErrorString(e));
    return scope.finish(PS_OK);
}

static bool srs_groups_ok(const ps_groth16_srs* s) {
    return s->tau_g1->group == PS_G1 && s->tau_g2->group == PS_G2 && s->alpha_tau_g1->group == PS_G1 && s->beta_tau_g1->group == PS_G1;
}

// The four scaled arrays into a zeroed `out`, arguments validated: all four or none
static int srs_contribute_run(ps_ctx* c, const ps_groth16_srs* in, const uint8_t* t_be32, const uint8_t* a_be32, const uint8_t* b_be32, const Fr& t, const Fr& a,
                              const Fr& b, ps_groth16_srs* out, ps_groth16_srs_share* share) {
    const size_t longest = std::max(std::max(in->tau_g1->n, in->tau_g2->n), std::max(in->alpha_tau_g1->n, in->beta_tau_g1->n));
    if ((unsigned long long)longest >= (1ull << 32)) return fail(PS_ERR_ARG, "ps_groth16_srs_contribute: an array of 2^32 points or more");
    ps_points *t1, *t2, *ta, *tb;  // the string's (const) arrays once all four are made
    Scope scope(c->stream);
    for (ps_points** made : {&t1, &t2, &ta, &tb}) scope.result(made);
    Fr* pw = nullptr;  // ONE table, as long as the longest array: t^i, then a t^i, then b t^i (each scaling returns complete)
    hipError_t e = scope.device(&pw, longest);
    if (e != hipSuccess) return fail(PS_ERR_HIP, std::string("ps_groth16_srs_contribute: hipMalloc: ") + hipGetErrorString(e));
    int rc;
    uint8_t gen2[192];
    generator_bytes<Fp2>(gen2);
    if ((rc = ps_points_lincomb(PS_G2, in->beta_g2, b_be32, 1, out->beta_g2))) return rc;
    if ((rc = ps_points_lincomb(PS_G2, gen2, t_be32, 1, share->t_g2))) return rc;
    if ((rc = ps_points_lincomb(PS_G2, gen2, a_be32, 1, share->a_g2))) return rc;
    if ((rc = ps_points_lincomb(PS_G2, gen2, b_be32, 1, share->b_g2))) return rc;
    if (longest) fr_powers_launch(c, t, fr_one(), longest, pw);
    if ((rc = points_scale_each(c, in->tau_g1, pw, &t1))) return rc;
    if ((rc = points_scale_each(c, in->tau_g2, pw, &t2))) return rc;
    if (in->alpha_tau_g1->n) fr_powers_launch(c, t, a, in->alpha_tau_g1->n, pw);
    if ((rc = points_scale_each(c, in->alpha_tau_g1, pw, &ta))) return rc;
    if (in->beta_tau_g1->n) fr_powers_launch(c, t, b, in->beta_tau_g1->n, pw);
    if ((rc = points_scale_each(c, in->beta_tau_g1, pw, &tb))) return rc;
    out->tau_g1 = t1;
    out->tau_g2 = t2;
    out->alpha_tau_g1 = ta;
    out->beta_tau_g1 = tb;
    return scope.finish(PS_OK);
}
extern "C" int ps_groth16_srs_contribute(ps_ctx* c, const ps_groth16_srs* in, const uint8_t* t_be32, const uint8_t* a_be32, const uint8_t* b_be32,
                                         ps_groth16_srs* out, ps_groth16_srs_share* share) {
    if (!c || !in || !t_be32 || !a_be32 || !b_be32 || !out || !share || in == out || !in->tau_g1 || !in->tau_g2 || !in->alpha_tau_g1 || !in->beta_tau_g1)
        return fail(PS_ERR_ARG, "ps_groth16_srs_contribute: NULL argument (or out == in)");
    memset(out, 0, sizeof *out);
    memset(share, 0, sizeof *share);
    if (!srs_groups_ok(in)) return fail(PS_ERR_ARG, "ps_groth16_srs_contribute: tau_g2 is a G2 array, the other three are G1 arrays");
    Fr t, a, b;
    if (!fr_mont_from_canonical_be32(&t, t_be32) || !fr_mont_from_canonical_be32(&a, a_be32) || !fr_mont_from_canonical_be32(&b, b_be32))
        return fail(PS_ERR_ENCODING, "ps_groth16_srs_contribute: t, a and b must be below r");
    if (fr_is_zero(t) || fr_is_zero(a) || fr_is_zero(b)) return fail(PS_ERR_ARG, "ps_groth16_srs_contribute: the shares t, a and b must be non-zero");
    HIP_TRY(hipSetDevice(c->device));
    const int rc = srs_contribute_run(c, in, t_be32, a_be32, b_be32, t, a, b, out, share);
    if (rc) {  // (the run has freed the arrays it made)
        memset(out, 0, sizeof *out);
        memset(share, 0, sizeof *share);
    }
    return rc;
}

// e(a1, b1) == e(a2, b2) for points the caller has validated (no subgroup test here): e(a1, b1) e(-a2, b2) == 1
static int pairing_pair_equal_trusted(ps_ctx* c, const uint8_t* a1, const uint8_t* b1, const uint8_t* a2, const uint8_t* b2, int* equal) {
    uint8_t g1[2 * 96], g2[2 * 192];
    *equal = 0;
    memcpy(g1, a1, 96);
    g1_negated(g1 + 96, a2);
    memcpy(g2, b1, 192);
    memcpy(g2 + 192, b2, 192);
    Scope scope;
    ps_points **p1 = scope.points(), **p2 = scope.points();
    int rc = ps_points_upload(c, PS_G1, g1, 2, PS_FMT_AFFINE, p1);
    if (!rc) rc = ps_points_upload(c, PS_G2, g2, 2, PS_FMT_AFFINE, p2);
    if (!rc) rc = ps_pairing_product_is_one(c, *p1, *p2, 0, equal);
    return rc;
}
// every one of k G2 encodings decodes (PS_ERR_ENCODING otherwise); *good = none is the identity and all lie in the subgroup
static int g2_points_usable(ps_ctx* c, const char* who, const uint8_t* enc, size_t k, bool subgroup, bool* good) {
    *good = false;
    bool identity = false;
    for (size_t i = 0; i < k; i++) {
        Affine<Fp2> p;
        if (!read_affine(p, enc + 192 * i)) return fail(PS_ERR_ENCODING, std::string(who) + ": a G2 point is not a canonical point on the curve");
        identity = identity || (enc[192 * i] & 0x40);
    }
    if (identity) return PS_OK;
    if (subgroup) {
        Scope scope;
        ps_points** up = scope.points();
        int in = 0;
        int rc = ps_points_upload(c, PS_G2, enc, k, PS_FMT_AFFINE, up);
        if (!rc) rc = ps_points_check_subgroup(c, *up, &in);
        if (rc || !in) return rc;
    }
    *good = true;
    return PS_OK;
}

// The first two points of the four arrays, fetched once: the generators, tau G1, tau G2, alpha G1, beta G1
struct SrsHeads {
    uint8_t t1[2][96], t2[2][192], a0[96], b0[96];
};
static int srs_heads(ps_ctx* c, const ps_groth16_srs* s, SrsHeads* h) {
    int rc = ps_points_download(c, s->tau_g1, 0, 2, h->t1[0]);
    if (!rc) rc = ps_points_download(c, s->tau_g2, 0, 2, h->t2[0]);
    if (!rc) rc = ps_points_download(c, s->alpha_tau_g1, 0, 1, h->a0);
    if (!rc) rc = ps_points_download(c, s->beta_tau_g1, 0, 1, h->b0);
    return rc;
}

static int srs_check_args(const char* who, ps_ctx* c, const ps_groth16_srs* s, const uint8_t* rho_be32, size_t nrho, size_t* pairs) {
    if (!s->tau_g1 || !s->tau_g2 || !s->alpha_tau_g1 || !s->beta_tau_g1) return fail(PS_ERR_ARG, std::string(who) + ": the string lacks an array");
    if (!srs_groups_ok(s)) return fail(PS_ERR_ARG, std::string(who) + ": tau_g2 is a G2 array, the other three are G1 arrays");
    if (s->tau_g1->n < 2 || s->tau_g2->n < 2) return fail(PS_ERR_ARG, std::string(who) + ": tau_g1 and tau_g2 need at least two points each (1 and tau)");
    if (s->alpha_tau_g1->n < 1 || s->beta_tau_g1->n < 1) return fail(PS_ERR_ARG, std::string(who) + ": alpha_tau_g1 and beta_tau_g1 need at least one point each");
    if (c->q_len) return fail(PS_ERR_ARG, std::string(who) + ": sums are pending on this context (ps_msm_finish them first)");
    const size_t longest = std::max(std::max(s->tau_g1->n, s->tau_g2->n), std::max(s->alpha_tau_g1->n, s->beta_tau_g1->n));
    *pairs = longest - 1;  // neighbouring pairs (i, i + 1) of the longest array: one weight each
    if (nrho < *pairs || !rho_be32)
        return fail(PS_ERR_LENGTH, std::string(who) + ": " + std::to_string(nrho) + " weights for arrays of up to " + std::to_string(*pairs) + " neighbouring pairs");
    for (size_t i = 0; i < *pairs; i++) {
        u32 w[8];
        if (!be32_to_words(w, rho_be32 + 32 * i)) return fail(PS_ERR_ENCODING, std::string(who) + ": rho[" + std::to_string(i) + "] is not below r");
    }
    return PS_OK;
}

// The body of ps_groth16_srs_check once the arguments are sound; `h` receives the heads of the arrays for the caller's own tests.
static int srs_check_impl(ps_ctx* c, const char* who, const ps_groth16_srs* s, const uint8_t* rho_be32, size_t pairs, bool subgroup, SrsHeads* h, int* ok) {
    *ok = 0;
    int rc = srs_heads(c, s, h);
    if (rc) return rc;
    uint8_t gen1[96], gen2[192];
    generator_bytes<Fp>(gen1);
    generator_bytes<Fp2>(gen2);
    // T1[0] = G1, T2[0] = G2; tau, alpha, beta are not zero
    if (memcmp(h->t1[0], gen1, 96) || memcmp(h->t2[0], gen2, 192)) return PS_OK;
    if ((h->t1[1][0] & 0x40) || (h->a0[0] & 0x40) || (h->b0[0] & 0x40)) return PS_OK;
    bool good = false;
    if ((rc = g2_points_usable(c, who, s->beta_g2, 1, subgroup, &good))) return rc;
    if (!good) return PS_OK;
    const ps_points* arr[4] = {s->tau_g1, s->tau_g2, s->alpha_tau_g1, s->beta_tau_g1};
    if (subgroup)
        for (const ps_points* p : arr) {
            int in = 0;
            if ((rc = ps_points_check_subgroup(c, p, &in))) return rc;
            if (!in) return PS_OK;
        }
    // Per array of m points the sums over the views [0, m - 1) and [1, m) with the SAME weights: lo = sum rho_i X[i],
    // hi = sum rho_i X[i + 1], i < m - 1 -- every point, X[m - 1] included, is in a pair (i, i + 1).  Arrays of one length share
    // one ps_msm_multi and so one digit sort (tau_g2, alpha_tau_g1 and beta_tau_g1 of a string cut for a circuit).
    uint8_t lo[4][192], hi[4][192];
    bool summed[4] = {false, false, false, false};
    Scope scope;
    ps_scalars** rho = scope.scalars();
    if (pairs && (rc = ps_scalars_upload(c, rho_be32, pairs, rho))) return rc;
    for (int i = 0; i < 4; i++) {
        const size_t m = arr[i]->n;
        if (summed[i] || m < 2) continue;  // a lone point has no neighbour to be tested against
        ps_points* views[8] = {};
        uint8_t* outs[8];
        size_t k = 0;
        for (int j = i; j < 4; j++) {
            if (arr[j]->n != m) continue;
            summed[j] = true;
            outs[k] = lo[j];
            outs[k + 1] = hi[j];
            ps_points **first = scope.points(), **next = scope.points();
            if ((rc = ps_points_slice(arr[j], 0, m - 1, first)) || (rc = ps_points_slice(arr[j], 1, m - 1, next))) return rc;
            views[k] = *first;
            views[k + 1] = *next;
            k += 2;
        }
        ps_scalars** w = scope.scalars();
        if ((rc = ps_scalars_slice(*rho, 0, m - 1, w)) || (rc = ps_msm_multi(c, views, k, *w, outs))) return rc;
    }
    // Each equation is a product of its own: two errors cannot cancel.
    int eq = 0;
    //   e(sum rho_i X[i], tau G2) = e(sum rho_i X[i + 1], G2) for X = T1, A, B: X[i + 1] = tau X[i]
    for (int i : {0, 2, 3}) {
        if (arr[i]->n < 2) continue;
        if ((rc = pairing_pair_equal_trusted(c, lo[i], h->t2[1], hi[i], gen2, &eq)) || !eq) return rc;
    }
    //   e(tau G1, sum rho_i T2[i]) = e(G1, sum rho_i T2[i + 1]): the same tau in G2
    if ((rc = pairing_pair_equal_trusted(c, h->t1[1], lo[1], gen1, hi[1], &eq)) || !eq) return rc;
    //   e(B[0], G2) = e(G1, beta_g2): the same beta in G2
    if ((rc = pairing_pair_equal_trusted(c, h->b0, gen2, gen1, s->beta_g2, &eq)) || !eq) return rc;
    *ok = 1;
    return PS_OK;
}

extern "C" int ps_groth16_srs_check(ps_ctx* c, const ps_groth16_srs* srs, const uint8_t* rho_be32, size_t nrho, int check_subgroup, int* ok) {
    if (!c || !srs || !ok) return fail(PS_ERR_ARG, "ps_groth16_srs_check: NULL argument");
    *ok = 0;
    size_t pairs = 0;
    int rc = srs_check_args("ps_groth16_srs_check", c, srs, rho_be32, nrho, &pairs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    SrsHeads h;
    return srs_check_impl(c, "ps_groth16_srs_check", srs, rho_be32, pairs, check_subgroup != 0, &h, ok);
}

extern "C" int ps_groth16_srs_check_update(ps_ctx* c, const ps_groth16_srs* before, const ps_groth16_srs* after, const ps_groth16_srs_share* share,
                                           const uint8_t* rho_be32, size_t nrho, int* ok) {
    const char* who = "ps_groth16_srs_check_update";
    if (!c || !before || !after || !share || !ok) return fail(PS_ERR_ARG, std::string(who) + ": NULL argument");
    *ok = 0;
    if (!before->tau_g1 || !before->tau_g2 || !before->alpha_tau_g1 || !before->beta_tau_g1) return fail(PS_ERR_ARG, std::string(who) + ": the string lacks an array");
    if (!srs_groups_ok(before)) return fail(PS_ERR_ARG, std::string(who) + ": tau_g2 is a G2 array, the other three are G1 arrays");
    size_t pairs = 0;
    int rc = srs_check_args(who, c, after, rho_be32, nrho, &pairs);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (before->tau_g1->n != after->tau_g1->n || before->tau_g2->n != after->tau_g2->n || before->alpha_tau_g1->n != after->alpha_tau_g1->n ||
        before->beta_tau_g1->n != after->beta_tau_g1->n)
        return PS_OK;
    // the share is untrusted: encoding and curve (an error), not the identity and in the subgroup (a rejection)
    bool good = false;
    uint8_t sh[3 * 192];
    memcpy(sh, share->t_g2, 192);
    memcpy(sh + 192, share->a_g2, 192);
    memcpy(sh + 384, share->b_g2, 192);
    if ((rc = g2_points_usable(c, who, sh, 3, true, &good))) return rc;
    if (!good) return PS_OK;
    SrsHeads was, is;
    int formed = 0;
    if ((rc = srs_check_impl(c, who, after, rho_be32, pairs, true, &is, &formed)) || !formed) return rc;
    if ((rc = srs_heads(c, before, &was))) return rc;
    uint8_t gen1[96], gen2[192];
    generator_bytes<Fp>(gen1);
    generator_bytes<Fp2>(gen2);
    int eq = 0;
    // tau' = t tau, alpha' = a alpha, beta' = b beta (in G1, and beta' in G2 as well) for the t, a, b behind the share
    if ((rc = pairing_pair_equal_trusted(c, is.t1[1], gen2, was.t1[1], share->t_g2, &eq)) || !eq) return rc;
    if ((rc = pairing_pair_equal_trusted(c, is.a0, gen2, was.a0, share->a_g2, &eq)) || !eq) return rc;
    if ((rc = pairing_pair_equal_trusted(c, is.b0, gen2, was.b0, share->b_g2, &eq)) || !eq) return rc;
    if ((rc = pairing_pair_equal_trusted(c, gen1, after->beta_g2, was.b0, share->b_g2, &eq)) || !eq) return rc;
    *ok = 1;
    return PS_OK;
}
