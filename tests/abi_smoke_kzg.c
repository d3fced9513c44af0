/* abi_smoke_kzg.c -- a KZG commitment through the C ABI, the way a cgo caller uses it: plain C99, nothing but
 * include/playsnark_hip.h.  Over a string in the clear (tau = 11: 6 points of tau_g1, tau G2) and p = (3, 1, 4, 1, 5):
 *   - ps_kzg_commit, ps_kzg_open at z = 7 and 2, ps_kzg_verify of both openings, ps_kzg_verify_batch of the two;
 *   - ps_poly_eval agrees with the opening's values; a changed value is rejected by both verifiers;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_kzg: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}
static void print_hex(const char* name, const uint8_t* b, size_t n) {
    printf("%s ", name);
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
    printf("\n");
}

#define N 5      /* coefficients */
#define LEN 6    /* points of the string: longer than p */
#define K 2      /* points opened */
#define TAU 11ull

/* {x^i G}, i < cnt, from a tau held in the clear (what a test may do and a ceremony must not) */
static int powers(ps_ctx* ctx, int group, unsigned long long x, size_t cnt, ps_points** out) {
    uint8_t k[LEN * 32];
    unsigned long long p = 1;
    for (size_t i = 0; i < cnt; i++, p *= x) be32_small(k + 32 * i, p);
    ps_scalars* s = NULL;
    int rc = ps_scalars_upload(ctx, k, cnt, &s);
    if (rc == PS_OK) rc = ps_points_from_scalars(ctx, group, s, out);
    ps_scalars_free(s);
    return rc;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(ps_poly_scan_tile() >= 256 && ps_poly_scan_tile() % 256 == 0);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    ps_points *tau_g1 = NULL, *tau_g2 = NULL;
    uint8_t t2[192];
    CHECK(powers(ctx, PS_G1, TAU, LEN, &tau_g1) == PS_OK && powers(ctx, PS_G2, TAU, 2, &tau_g2) == PS_OK);
    CHECK(ps_points_download(ctx, tau_g2, 1, 1, t2) == PS_OK);

    const unsigned long long coef[N] = {3, 1, 4, 1, 5}, zs[K] = {7, 2};
    uint8_t p_be[N * 32], z_be[K * 32];
    for (int i = 0; i < N; i++) be32_small(p_be + 32 * i, coef[i]);
    for (int j = 0; j < K; j++) be32_small(z_be + 32 * j, zs[j]);
    ps_scalars* p = NULL;
    CHECK(ps_scalars_upload(ctx, p_be, N, &p) == PS_OK);

    uint8_t commit[96], y[K * 32], y2[K * 32], proofs[K * 96], want[32];
    CHECK(ps_kzg_commit(ctx, tau_g1, p, commit) == PS_OK);
    CHECK(ps_kzg_open(ctx, tau_g1, p, z_be, K, y, proofs) == PS_OK);
    CHECK(ps_poly_eval(ctx, p, z_be, K, y2) == PS_OK && memcmp(y, y2, sizeof y) == 0);
    for (int j = 0; j < K; j++) { /* Horner in 64-bit arithmetic */
        unsigned long long v = 0;
        for (int i = N - 1; i >= 0; i--) v = v * zs[j] + coef[i];
        be32_small(want, v);
        CHECK(memcmp(y + 32 * j, want, 32) == 0);
    }

    /* the quotient rows themselves: (p - p(7)) / (X - 7) = 5 X^3 + 36 X^2 + 256 X + 1793 */
    ps_scalars* q = NULL;
    uint8_t rem[K * 32], qb[K * (N - 1) * 32];
    const unsigned long long q7[N - 1] = {1793, 256, 36, 5};
    CHECK(ps_poly_div_linear(ctx, p, z_be, K, &q, rem) == PS_OK && ps_scalars_len(q) == K * (N - 1));
    CHECK(memcmp(rem, y, sizeof rem) == 0);
    CHECK(ps_scalars_download(ctx, q, 0, K * (N - 1), qb) == PS_OK);
    for (int i = 0; i < N - 1; i++) {
        be32_small(want, q7[i]);
        CHECK(memcmp(qb + 32 * i, want, 32) == 0);
    }
    ps_scalars_free(q);

    int ok = -1;
    for (int j = 0; j < K; j++) {
        CHECK(ps_kzg_verify(t2, commit, z_be + 32 * j, y + 32 * j, proofs + 96 * j, &ok) == PS_OK && ok == 1);
    }
    uint8_t commits[K * 96], rho[K * 32], bad[K * 32];
    for (int j = 0; j < K; j++) memcpy(commits + 96 * j, commit, 96);
    memset(rho, 0, sizeof rho);
    for (int j = 0; j < K; j++)
        for (int b = 16; b < 32; b++) rho[32 * j + b] = (uint8_t)(41 * j + 13 * b + 3); /* 128-bit weights */
    CHECK(ps_kzg_verify_batch(ctx, t2, commits, z_be, y, proofs, rho, K, 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_kzg_verify_batch(ctx, t2, commits, z_be, y, proofs, rho, 0, 1, &ok) == PS_OK && ok == 1);
    /* another value for the second point */
    memcpy(bad, y, sizeof bad);
    bad[63] ^= 1;
    CHECK(ps_kzg_verify(t2, commit, z_be + 32, bad + 32, proofs + 96, &ok) == PS_OK && ok == 0);
    CHECK(ps_kzg_verify_batch(ctx, t2, commits, z_be, bad, proofs, rho, K, 1, &ok) == PS_OK && ok == 0);
    /* argument checks: a point that is not below r, a string shorter than p, k = 0 */
    uint8_t big[32];
    memset(big, 0xff, 32);
    CHECK(ps_poly_eval(ctx, p, big, 1, y2) == PS_ERR_ENCODING);
    ps_points* shorter = NULL;
    CHECK(ps_points_slice(tau_g1, 0, N - 1, &shorter) == PS_OK);
    CHECK(ps_kzg_commit(ctx, shorter, p, commit) == PS_ERR_LENGTH);
    CHECK(ps_kzg_open(ctx, tau_g1, p, z_be, 0, NULL, NULL) == PS_OK);
    CHECK(ps_kzg_commit(ctx, tau_g1, p, commit) == PS_OK);

    print_hex("commit", commit, 96);
    print_hex("y", y, sizeof y);
    print_hex("proofs", proofs, sizeof proofs);

    ps_points_free(shorter);
    ps_scalars_free(p);
    ps_points_free(tau_g1);
    ps_points_free(tau_g2);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg ok\n");
    return 0;
}
