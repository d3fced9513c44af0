/* abi_smoke_crs_check.c -- the check of a Groth16 key against its powers-of-tau string through the C ABI, the way a cgo caller
 * uses it: plain C99, nothing but include/playsnark_hip.h.  For the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198):
 *   - a phase-1 string from small caller-chosen values (x = 11, alpha = 5, beta = 7: every power fits 64 bits);
 *   - the key ps_groth16_setup makes from the same values with delta = gamma = 1, and that key with a share (d, g) folded in:
 *     ps_groth16_crs_check_from_srs accepts both, with the subgroup tests on and off, and the key without its Lagrange form;
 *   - with Alpha swapped for Beta, with the unscaled XiT kept, or with an array one point short: rejected;
 *   - too few weights, or a string one point short: PS_ERR_LENGTH;
 *   - ps_points_lagrange_check: lxi belongs to xi (nodes = 0) and lxi_t to xi_t (nodes = 1); lxi as the form of xi on the
 *     other nodes: rejected.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_crs_check.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_crs_check
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_crs_check: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define N 4     /* gates */
#define NVARS 6 /* [const, x, out, u, v, w] */

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
    ps_qap* qap = NULL;
    CHECK(ps_qap_create(ctx, N, NVARS, 3, &L, &R, &O, &qap) == PS_OK);

    /* phase 1, as a ceremony would publish it */
    const unsigned long long x = 11, alpha = 5, beta = 7;
    ps_points *tau1 = NULL, *tau2 = NULL, *atau = NULL, *btau = NULL, *b2 = NULL, *tau1_short = NULL, *nio_short = NULL, *xi_head = NULL, *lxi_head = NULL;
    CHECK(powers(ctx, PS_G1, 1, x, 2 * N - 1, &tau1) == PS_OK && powers(ctx, PS_G2, 1, x, N, &tau2) == PS_OK);
    CHECK(powers(ctx, PS_G1, alpha, x, N, &atau) == PS_OK && powers(ctx, PS_G1, beta, x, N, &btau) == PS_OK);
    CHECK(powers(ctx, PS_G2, beta, x, 1, &b2) == PS_OK);
    ps_groth16_srs srs;
    memset(&srs, 0, sizeof srs);
    srs.tau_g1 = tau1; srs.tau_g2 = tau2; srs.alpha_tau_g1 = atau; srs.beta_tau_g1 = btau;
    CHECK(ps_points_download(ctx, b2, 0, 1, srs.beta_g2) == PS_OK);

    /* the circuit's key for the same values, and that key after one party's share */
    ps_groth16_crs k0, k1, bad;
    ps_groth16_toxic tw;
    be32_small(tw.alpha, alpha); be32_small(tw.beta, beta); be32_small(tw.delta, 1); be32_small(tw.x, x); be32_small(tw.gamma, 1);
    CHECK(ps_groth16_setup(ctx, qap, &tw, &k0) == PS_OK);
    uint8_t d[32], g[32], rho[8 * 32];
    be32_small(d, 424243ull); be32_small(g, 31337ull);
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < 8; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(41 * i + 13 * k + 3); /* 128-bit weights */
    CHECK(ps_groth16_crs_contribute(ctx, &k0, d, g, &k1) == PS_OK);

    /* accepted: max(n_vars, n_gates) = 6 weights are enough */
    int ok = -1;
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &k0, rho, NVARS, 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &k1, rho, 8, 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &k1, rho, 8, 0, &ok) == PS_OK && ok == 1);
    bad = k1;
    bad.lxi = NULL; bad.lxi2 = NULL; bad.lxi_t = NULL; /* a monomial-only key */
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &bad, rho, 8, 1, &ok) == PS_OK && ok == 1);

    /* rejected */
    bad = k1;
    memcpy(bad.alpha, k1.beta, 96);
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &bad, rho, 8, 1, &ok) == PS_OK && ok == 0);
    bad = k1;
    bad.xi_t = k0.xi_t; /* not scaled with the rest */
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &bad, rho, 8, 1, &ok) == PS_OK && ok == 0);
    CHECK(ps_points_slice(k1.nio_lp, 0, ps_points_len(k1.nio_lp) - 1, &nio_short) == PS_OK);
    bad = k1;
    bad.nio_lp = nio_short; /* a key array of the wrong length is a rejection, not an error */
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &bad, rho, 8, 1, &ok) == PS_OK && ok == 0);

    /* errors */
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &k1, rho, NVARS - 1, 1, &ok) == PS_ERR_LENGTH);
    CHECK(ps_points_slice(tau1, 0, 2 * N - 2, &tau1_short) == PS_OK);
    srs.tau_g1 = tau1_short;
    CHECK(ps_groth16_crs_check_from_srs(ctx, qap, &srs, &k1, rho, 8, 1, &ok) == PS_ERR_LENGTH);
    srs.tau_g1 = tau1;

    /* one array against another */
    CHECK(ps_points_lagrange_check(ctx, qap, k1.xi, k1.lxi, 0, rho, N, &ok) == PS_OK && ok == 1);
    CHECK(ps_points_lagrange_check(ctx, qap, k1.xi2, k1.lxi2, 0, rho, N, &ok) == PS_OK && ok == 1);
    CHECK(ps_points_lagrange_check(ctx, qap, k1.xi_t, k1.lxi_t, 1, rho, N - 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_points_slice(k1.xi, 0, N - 1, &xi_head) == PS_OK && ps_points_slice(k1.lxi, 0, N - 1, &lxi_head) == PS_OK);
    CHECK(ps_points_lagrange_check(ctx, qap, xi_head, lxi_head, 1, rho, N - 1, &ok) == PS_OK && ok == 0);
    CHECK(ps_points_lagrange_check(ctx, qap, k1.xi, k1.lxi, 1, rho, N, &ok) == PS_ERR_LENGTH);
    CHECK(ps_points_lagrange_check(ctx, qap, k1.xi, k1.lxi2, 0, rho, N, &ok) == PS_ERR_ARG);

    crs_free(&k0); crs_free(&k1);
    ps_points_free(nio_short); ps_points_free(xi_head); ps_points_free(lxi_head);
    ps_points_free(tau1_short); ps_points_free(tau1); ps_points_free(tau2); ps_points_free(atau); ps_points_free(btau); ps_points_free(b2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_crs_check ok\n");
    return 0;
}
