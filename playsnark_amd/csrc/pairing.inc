// Host-side BLS12-381 ate pairing and the two verifiers (SURVEY.md section 8 row f1):
//   ps_groth16_verify <- Groth16Verify (groth16.go:214-233)  4 pairings + one IO MSM
//   ps_phgr13_verify  <- PHGR13Verify  (pinochio.go:281-378) 12 pairings + three IO MSMs
// The reference gets Pair() from kilic/bls12-381 through kyber (curve.go:33-38).  Verification
// only compares products of pairings, so any non-degenerate bilinear e: G1 x G2 -> GT on the curve
// serves; this is the ate Miller loop with an inversion-free running point and sparse line products, and the
// final exponentiation f -> f^(3 (p^12 - 1) / r) by the x-chain (pairing_math.inc; the literal affine loop and the
// 2030-bit exponentiation it replaced stay there as the reference of tests/host_limb_check.cpp: 73 -> 11 ms for
// ps_pairing_equal).  A handful of pairings per proof: CPU is the right
// place (the IO MSMs -- size nbVars-nbIO because of the reference's `diff` convention -- go
// through the GPU MSM).  MANY proofs under one key are another matter: verify_batch.inc runs their Miller loops on the
// device (pairing_dev.hpp) and shares one final exponentiation.  Included by capi.hip; host code only.

#define PS_HOSTFIELD 1
#include "pairing_math.inc"

// The verifiers read, validate and add points in the device representation (the same read_affine / affine_sum the rest of
// the library uses); the pairings themselves run over the host field.
static bool product_is_one(const std::vector<std::pair<Affine<Fp>, Affine<Fp2>>>& pairs) {
    std::vector<std::pair<Affine<Fq>, Affine<Fq2>>> h;
    h.reserve(pairs.size());
    for (auto& pq : pairs) h.push_back({affine_to_host<Fp>(pq.first), affine_to_host<Fp2>(pq.second)});
    return pairing::pairing_product_is_one(h);
}

// Untrusted points (proof elements, verification-key points): canonical encoding, on the curve AND in the
// order-r subgroup -- what kyber's UnmarshalBinary enforces [upstream]; the Miller loop's "T = kQ, 1 < k < r"
// needs it.  The [r]P tests of one verification run on host threads.
static bool read_g1(Affine<Fp>& a, const uint8_t* p) { return read_affine(a, p); }
static bool read_g2(Affine<Fp2>& a, const uint8_t* p) { return read_affine(a, p); }
static bool all_in_subgroup(const std::vector<const Affine<Fp>*>& g1, const std::vector<const Affine<Fp2>*>& g2) {
    std::vector<std::future<bool>> jobs;
    // [r]P in the host representation (hostfield.inc)
    auto in_subgroup = [](auto h) {
        typedef decltype(h.x) H;
        if (affine_is_identity<H>(h)) return true;
        u32 r[8];
        for (int i = 0; i < 8; i++) r[i] = FrParams::mod(i);
        return xyzz_is_identity(xyzz_mul_scalar<H>(xyzz_from_affine<H>(h.x, h.y), r));
    };
    for (auto* p : g1) jobs.push_back(std::async(std::launch::async, [p, in_subgroup] { return in_subgroup(affine_to_host<Fp>(*p)); }));
    for (auto* p : g2) jobs.push_back(std::async(std::launch::async, [p, in_subgroup] { return in_subgroup(affine_to_host<Fp2>(*p)); }));
    bool all = true;
    for (auto& j : jobs) all = j.get() && all;
    return all;
}
static int vk_array_in_subgroup(ps_ctx* c, const ps_points* arr, const char* who) {
    int ok = 0;
    int rc = PS_OK;
    if (arr->n <= 64) {
        // A handful of points (the IO part of a verification key): [r]P is 380 dependent group operations, 6 ms for one GPU
        // lane (16 for G2) and 0.3 ms for a host thread -- download them and test here.
        const size_t wb = wire_bytes(arr->group);
        std::vector<uint8_t> raw(wb * arr->n);
        if (arr->n && (rc = ps_points_download(c, arr, 0, arr->n, raw.data()))) return rc;
        std::vector<Affine<Fp>> g1(arr->group == PS_G1 ? arr->n : 0);
        std::vector<Affine<Fp2>> g2(arr->group == PS_G2 ? arr->n : 0);
        std::vector<const Affine<Fp>*> p1;
        std::vector<const Affine<Fp2>*> p2;
        for (size_t i = 0; i < arr->n; i++) {
            const bool good = arr->group == PS_G1 ? read_affine(g1[i], raw.data() + wb * i) : read_affine(g2[i], raw.data() + wb * i);
            if (!good) return fail(PS_ERR_ENCODING, std::string(who) + ": bad point in a verification-key array");
            if (arr->group == PS_G1) p1.push_back(&g1[i]); else p2.push_back(&g2[i]);
        }
        ok = all_in_subgroup(p1, p2) ? 1 : 0;
    } else {
        rc = ps_points_check_subgroup(c, arr, &ok);
    }
    if (rc) return rc;
    return ok ? PS_OK : fail(PS_ERR_ENCODING, std::string(who) + ": verification-key array holds a point outside the order-r subgroup");
}

template <class F>
static Affine<F> affine_sum(const Affine<F>& a, const Affine<F>& b) {
    Xyzz<F> acc = xyzz_identity<F>();
    if (!affine_is_identity<F>(a)) xyzz_madd<F>(acc, a.x, a.y);
    if (!affine_is_identity<F>(b)) xyzz_madd<F>(acc, b.x, b.y);
    Affine<F> r;
    if (!xyzz_to_affine<F>(acc, r.x, r.y)) { r.x = f_zero((const F*)0); r.y = f_zero((const F*)0); }
    return r;
}

// e(a, b) for tests of the pairing itself: 1 if e(a1,b1) == e(a2,b2)
extern "C" int ps_pairing_equal(const uint8_t* a1_g1, const uint8_t* b1_g2, const uint8_t* a2_g1, const uint8_t* b2_g2, int* equal) {
    if (!a1_g1 || !b1_g2 || !a2_g1 || !b2_g2 || !equal) return fail(PS_ERR_ARG, "ps_pairing_equal: NULL argument");
    Affine<Fp> p1, p2;
    Affine<Fp2> q1, q2;
    if (!read_g1(p1, a1_g1) || !read_g2(q1, b1_g2) || !read_g1(p2, a2_g1) || !read_g2(q2, b2_g2))
        return fail(PS_ERR_ENCODING, "ps_pairing_equal: bad point encoding");
    if (!all_in_subgroup({&p1, &p2}, {&q1, &q2})) return fail(PS_ERR_ENCODING, "ps_pairing_equal: point outside the order-r subgroup");
    *equal = product_is_one({{p1, q1}, {pairing_dev::neg_g1(p2), q2}}) ? 1 : 0;
    return PS_OK;
}

// Groth16Verify (groth16.go:214-233):  e(A,B) == e(Alpha,Beta2) * e(sum io_i IoLP_i, Gamma) * e(C,Delta2)
extern "C" int ps_groth16_verify(ps_ctx* c, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t* A, const uint8_t* B,
                                 const uint8_t* C, int* ok) {
    if (!c || !vk || !io || !A || !B || !C || !ok || !vk->io_lp) return fail(PS_ERR_ARG, "ps_groth16_verify: NULL argument");
    *ok = 0;
    uint8_t b1[96];
    int rc = vk_array_in_subgroup(c, vk->io_lp, "ps_groth16_verify");
    if (rc) return rc;
    rc = ps_msm(c, vk->io_lp, io, b1);  // groth16.go:225-228; length mismatch -> PS_ERR_LENGTH
    if (rc) return rc;
    Affine<Fp> a, cc, alpha, x;
    Affine<Fp2> b, beta2, gamma, delta2;
    if (!read_g1(a, A) || !read_g2(b, B) || !read_g1(cc, C) || !read_g1(alpha, vk->alpha) || !read_g2(beta2, vk->beta2) ||
        !read_g2(gamma, vk->gamma) || !read_g2(delta2, vk->delta2) || !read_g1(x, b1))
        return fail(PS_ERR_ENCODING, "ps_groth16_verify: bad point encoding");
    if (!all_in_subgroup({&a, &cc, &alpha}, {&b, &beta2, &gamma, &delta2}))
        return fail(PS_ERR_ENCODING, "ps_groth16_verify: point outside the order-r subgroup");
    using pairing_dev::neg_g1;
    *ok = product_is_one({{a, b}, {neg_g1(alpha), beta2}, {neg_g1(x), gamma}, {neg_g1(cc), delta2}}) ? 1 : 0;
    return PS_OK;
}

// PHGR13Verify (pinochio.go:281-378): division check, knowledge (CRS) checks, linear check
extern "C" int ps_phgr13_verify(ps_ctx* c, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* pf, int* ok) {
    if (!c || !vk || !io || !pf || !ok || !vk->vs_io || !vk->ws_io || !vk->ys_io) return fail(PS_ERR_ARG, "ps_phgr13_verify: NULL argument");
    *ok = 0;
    uint8_t gvk[96], gwk[192], gyk[96];
    int rc;
    for (const ps_points* arr : {vk->vs_io, vk->ws_io, vk->ys_io})
        if ((rc = vk_array_in_subgroup(c, arr, "ps_phgr13_verify"))) return rc;
    if ((rc = ps_msm(c, vk->vs_io, io, gvk))) return rc;  // computeCommitIOSolution, pinochio.go:293-295
    if ((rc = ps_msm(c, vk->ws_io, io, gwk))) return rc;
    if ((rc = ps_msm(c, vk->ys_io, io, gyk))) return rc;
    Affine<Fp> vio, yio, vss, vass, wass, yss, yass, hs, gz, aw, bgamma;
    Affine<Fp2> wio, wss, av, ay, gamma, bgamma2, yts;
    bool good = read_g1(vio, gvk) && read_g2(wio, gwk) && read_g1(yio, gyk) && read_g1(vss, pf->vss) && read_g1(vass, pf->vass) &&
                read_g2(wss, pf->wss) && read_g1(wass, pf->wass) && read_g1(yss, pf->yss) && read_g1(yass, pf->yass) &&
                read_g1(hs, pf->hs) && read_g1(gz, pf->gz) && read_g2(av, vk->av) && read_g1(aw, vk->aw) && read_g2(ay, vk->ay) &&
                read_g2(gamma, vk->gamma) && read_g1(bgamma, vk->bgamma) && read_g2(bgamma2, vk->bgamma2) && read_g2(yts, vk->yts);
    if (!good) return fail(PS_ERR_ENCODING, "ps_phgr13_verify: bad point encoding");
    if (!all_in_subgroup({&vss, &vass, &wass, &yss, &yass, &hs, &gz, &aw, &bgamma}, {&wss, &av, &ay, &gamma, &bgamma2, &yts}))
        return fail(PS_ERR_ENCODING, "ps_phgr13_verify: point outside the order-r subgroup");
    using pairing_dev::neg_g1;
    const Affine<Fp2> g2 = generator((const Fp2*)0);
    // division check :297-322   e(gv, gw) == e(hs, yts) * e(gy, G2)
    Affine<Fp> gv = affine_sum<Fp>(vio, vss), gy = affine_sum<Fp>(yio, yss);
    Affine<Fp2> gw = affine_sum<Fp2>(wio, wss);
    // linear check :359-372   e(gz, gamma) == e(vss + yss, bgamma2) * e(bgamma, wss)
    Affine<Fp> lt1 = affine_sum<Fp>(vss, yss);
    // the five checks are independent: each on its own host thread
    typedef std::vector<std::pair<Affine<Fp>, Affine<Fp2>>> Pairs;
    const Pairs checks[5] = {
        {{gv, gw}, {neg_g1(hs), yts}, {neg_g1(gy), g2}},             // division
        {{vass, g2}, {neg_g1(vss), av}},                             // knowledge checks :333-350
        {{wass, g2}, {neg_g1(aw), wss}},
        {{yass, g2}, {neg_g1(yss), ay}},
        {{gz, gamma}, {neg_g1(lt1), bgamma2}, {neg_g1(bgamma), wss}},  // linear
    };
    std::future<bool> res[5];
    for (int i = 0; i < 5; i++) res[i] = std::async(std::launch::async, [&checks, i] { return product_is_one(checks[i]); });
    bool all = true;
    for (int i = 0; i < 5; i++) all = res[i].get() && all;
    if (!all) return PS_OK;
    *ok = 1;
    return PS_OK;
}
