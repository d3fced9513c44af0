/* abi_smoke_srs.c -- a Groth16 key from a powers-of-tau string through the C ABI, the way a cgo caller uses it: plain C99,
 * nothing but include/playsnark_hip.h.  For the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198, witness
 * r1cs.go:67-76):
 *   - a phase-1 string from small caller-chosen values (x = 11, alpha = 5, beta = 7: every power fits 64 bits);
 *   - ps_groth16_setup_from_srs: NioLP, IoLP, XiT and LXiT byte-equal to ps_groth16_setup with delta = gamma = 1;
 *   - ps_groth16_crs_contribute with (d, g), ps_groth16_crs_check_update: accepted; with Alpha swapped for Beta, or with the
 *     old XiT kept: rejected; too few weights: PS_ERR_LENGTH; d = 0: PS_ERR_ARG; a string one point short: PS_ERR_LENGTH;
 *   - one proof under the contributed key, verified with ps_groth16_verify.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_srs.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_srs
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_srs: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define N 4    /* gates */
#define DIFF 3 /* nbVars - nbIO = 6 - 3 */

/* {scale * x^i G}, i < cnt */
static int powers(ps_ctx* ctx, int group, unsigned long long scale, unsigned long long x, size_t cnt, ps_points** out) {
    uint8_t k[(2 * N - 1) * 32];
    unsigned long long p = scale;
    for (size_t i = 0; i < cnt; i++, p *= x) be32_small(k + 32 * i, p);
    ps_scalars* s = NULL;
    int rc = ps_scalars_upload(ctx, k, cnt, &s);
    if (rc == PS_OK) rc = ps_points_from_scalars(ctx, group, s, out);
    ps_scalars_free(s);
    return rc;
}

static int same_points(ps_ctx* ctx, const ps_points* a, const ps_points* b) {
    uint8_t x[8 * 96], y[8 * 96];
    const size_t n = ps_points_len(a);
    if (n != ps_points_len(b) || n > 8) return 0;
    if (ps_points_download(ctx, a, 0, n, x) != PS_OK || ps_points_download(ctx, b, 0, n, y) != PS_OK) return 0;
    return memcmp(x, y, 96 * n) == 0;
}

static void crs_free(ps_groth16_crs* k) {
    ps_points_free(k->xi); ps_points_free(k->xi2); ps_points_free(k->io_lp); ps_points_free(k->nio_lp); ps_points_free(k->xi_t);
    ps_points_free(k->lxi); ps_points_free(k->lxi2); ps_points_free(k->lxi_t);
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    /* the toy R1CS, rows = gates, columns = [const, x, out, u, v, w] (r1cs.go:178-198): n = 4 gates, nbIO = 3 */
    const uint32_t l_ptr[5] = {0, 1, 2, 4, 6}, l_col[6] = {1, 3, 1, 4, 0, 5};
    const int64_t l_val[6] = {1, 1, 1, 1, 5, 1};
    const uint32_t r_ptr[5] = {0, 1, 2, 3, 4}, r_col[4] = {1, 1, 0, 0};
    const int64_t r_val[4] = {1, 1, 1, 1};
    const uint32_t o_ptr[5] = {0, 1, 2, 3, 4}, o_col[4] = {3, 4, 5, 2};
    const int64_t o_val[4] = {1, 1, 1, 1};
    const ps_csr L = {l_ptr, l_col, l_val}, R = {r_ptr, r_col, r_val}, O = {o_ptr, o_col, o_val};
    const int64_t witness[6] = {1, 3, 35, 9, 27, 30}; /* createWitness, r1cs.go:67-76 */
    ps_qap* qap = NULL;
    ps_scalars* sol = NULL;
    CHECK(ps_qap_create(ctx, N, 6, 3, &L, &R, &O, &qap) == PS_OK);
    CHECK(ps_scalars_upload_i64(ctx, witness, 6, &sol) == PS_OK);

    /* phase 1, as a ceremony would publish it */
    const unsigned long long x = 11, alpha = 5, beta = 7;
    ps_points *tau1 = NULL, *tau2 = NULL, *atau = NULL, *btau = NULL, *b2 = NULL, *tau1_short = NULL;
    CHECK(powers(ctx, PS_G1, 1, x, 2 * N - 1, &tau1) == PS_OK && powers(ctx, PS_G2, 1, x, N, &tau2) == PS_OK);
    CHECK(powers(ctx, PS_G1, alpha, x, N, &atau) == PS_OK && powers(ctx, PS_G1, beta, x, N, &btau) == PS_OK);
    CHECK(powers(ctx, PS_G2, beta, x, 1, &b2) == PS_OK);
    ps_groth16_srs srs;
    memset(&srs, 0, sizeof srs);
    srs.tau_g1 = tau1; srs.tau_g2 = tau2; srs.alpha_tau_g1 = atau; srs.beta_tau_g1 = btau;
    CHECK(ps_points_download(ctx, b2, 0, 1, srs.beta_g2) == PS_OK);

    /* phase 2, step 0: the circuit's key with delta = gamma = 1 -- the key the toxic-waste setup makes from the same values */
    ps_groth16_crs k0, ref, k1, bad;
    CHECK(ps_groth16_setup_from_srs(ctx, qap, &srs, &k0) == PS_OK);
    ps_groth16_toxic tw;
    be32_small(tw.alpha, alpha); be32_small(tw.beta, beta); be32_small(tw.delta, 1); be32_small(tw.x, x); be32_small(tw.gamma, 1);
    CHECK(ps_groth16_setup(ctx, qap, &tw, &ref) == PS_OK);
    CHECK(ps_points_len(k0.io_lp) == DIFF && ps_points_len(k0.xi_t) == N - 1);
    CHECK(same_points(ctx, k0.nio_lp, ref.nio_lp) && same_points(ctx, k0.io_lp, ref.io_lp));
    CHECK(same_points(ctx, k0.xi_t, ref.xi_t) && same_points(ctx, k0.lxi_t, ref.lxi_t) && same_points(ctx, k0.xi, ref.xi));
    CHECK(memcmp(k0.alpha, ref.alpha, 96) == 0 && memcmp(k0.beta2, ref.beta2, 192) == 0 && memcmp(k0.delta2, ref.delta2, 192) == 0);
    CHECK(ps_points_slice(tau1, 0, 2 * N - 2, &tau1_short) == PS_OK);
    srs.tau_g1 = tau1_short;
    CHECK(ps_groth16_setup_from_srs(ctx, qap, &srs, &bad) == PS_ERR_LENGTH);

    /* one party's share, and anybody's check of it */
    uint8_t d[32], g[32], zero[32], rho[8 * 32];
    be32_small(d, 424243ull); be32_small(g, 31337ull); be32_small(zero, 0);
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < 8; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(41 * i + 13 * k + 3); /* 128-bit weights */
    CHECK(ps_groth16_crs_contribute(ctx, &k0, zero, g, &k1) == PS_ERR_ARG);
    CHECK(ps_groth16_crs_contribute(ctx, &k0, d, g, &k1) == PS_OK);
    CHECK(!same_points(ctx, k0.nio_lp, k1.nio_lp) && same_points(ctx, k0.xi, k1.xi));
    int ok = -1;
    CHECK(ps_groth16_crs_check_update(ctx, &k0, &k1, rho, 8, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_crs_check_update(ctx, &k0, &k1, rho, 2, &ok) == PS_ERR_LENGTH);
    bad = k1;
    memcpy(bad.alpha, k1.beta, 96);
    CHECK(ps_groth16_crs_check_update(ctx, &k0, &bad, rho, 8, &ok) == PS_OK && ok == 0);
    bad = k1;
    bad.xi_t = k0.xi_t; /* not scaled with the rest */
    CHECK(ps_groth16_crs_check_update(ctx, &k0, &bad, rho, 8, &ok) == PS_OK && ok == 0);

    /* a proof under the contributed key */
    ps_groth16_pk pk;
    memset(&pk, 0, sizeof pk); /* the header requires zero-initialised structs */
    memcpy(pk.alpha, k1.alpha, 96); memcpy(pk.beta, k1.beta, 96); memcpy(pk.delta, k1.delta, 96);
    memcpy(pk.beta2, k1.beta2, 192); memcpy(pk.delta2, k1.delta2, 192);
    pk.xi = k1.xi; pk.xi2 = k1.xi2; pk.nio_lp = k1.nio_lp; pk.xi_t = k1.xi_t;
    pk.lxi = k1.lxi; pk.lxi2 = k1.lxi2; pk.lxi_t = k1.lxi_t;
    ps_groth16_vk vk;
    memset(&vk, 0, sizeof vk);
    memcpy(vk.alpha, k1.alpha, 96); memcpy(vk.beta2, k1.beta2, 192); memcpy(vk.gamma, k1.gamma, 192); memcpy(vk.delta2, k1.delta2, 192);
    vk.io_lp = k1.io_lp;
    uint8_t r[32], s[32], A[96], B[192], C[96], io_be[DIFF * 32];
    be32_small(r, 1000003ull); be32_small(s, 777ull);
    CHECK(ps_groth16_prove(ctx, &pk, qap, sol, r, s, A, B, C) == PS_OK);
    for (int j = 0; j < DIFF; j++) be32_small(io_be + 32 * j, (unsigned long long)witness[j]);
    ps_scalars* io = NULL;
    CHECK(ps_scalars_upload(ctx, io_be, DIFF, &io) == PS_OK);
    ok = -1;
    CHECK(ps_groth16_verify(ctx, &vk, io, A, B, C, &ok) == PS_OK && ok == 1);
    vk.io_lp = k0.io_lp; /* the key before the share does not accept it */
    CHECK(ps_groth16_verify(ctx, &vk, io, A, B, C, &ok) == PS_OK && ok == 0);

    /* both keys are freed handle by handle, in either order (k1's xi, xi2, lxi, lxi2 are views of k0's storage) */
    crs_free(&k0); crs_free(&k1); crs_free(&ref);
    ps_scalars_free(io); ps_scalars_free(sol);
    ps_points_free(tau1_short); ps_points_free(tau1); ps_points_free(tau2); ps_points_free(atau); ps_points_free(btau); ps_points_free(b2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_srs ok\n");
    return 0;
}
