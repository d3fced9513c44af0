/* abi_smoke_kzg_set.c -- one polynomial opened at a SET of points with ONE proof, through the C ABI the way a cgo caller uses
 * it: plain C99, nothing but include/playsnark_hip.h.  Over a string in the clear (tau = 11: 7 points of tau_g1, 3 of tau_g2),
 * p = (3, 1, 4, 1, 5, 9) and the set {2, 7}:
 *   - ps_poly_div_roots gives the 4 quotient coefficients by (X - 2)(X - 7), both values and the 2 remainder coefficients;
 *   - ps_kzg_open_set gives the same values and one proof, which ps_kzg_verify_set accepts and, with a changed value or with the
 *     two values swapped, rejects;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_set_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg_set.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg_set
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_kzg_set: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
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

#define N 6      /* coefficients of p */
#define K 2      /* points of the set */
#define LEN 7    /* points of tau_g1: longer than p */
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
    CHECK(ps_poly_scan_set_group() >= 1);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    ps_points *tau_g1 = NULL, *tau_g2 = NULL;
    CHECK(powers(ctx, PS_G1, TAU, LEN, &tau_g1) == PS_OK && powers(ctx, PS_G2, TAU, K + 1, &tau_g2) == PS_OK);

    const unsigned long long c[N] = {3, 1, 4, 1, 5, 9}, zs[K] = {2, 7};
    uint8_t p_be[N * 32], z_be[K * 32], want[32];
    for (int i = 0; i < N; i++) be32_small(p_be + 32 * i, c[i]);
    for (int j = 0; j < K; j++) be32_small(z_be + 32 * j, zs[j]);
    ps_scalars* p = NULL;
    CHECK(ps_scalars_upload(ctx, p_be, N, &p) == PS_OK);

    /* the division: N - K quotient coefficients, the values, the remainder */
    ps_scalars* q = NULL;
    uint8_t q_be[(N - K) * 32], y[K * 32], rem[K * 32];
    CHECK(ps_poly_div_roots(ctx, p, z_be, K, &q, y, rem) == PS_OK && ps_scalars_len(q) == N - K);
    CHECK(ps_scalars_download(ctx, q, 0, N - K, q_be) == PS_OK);
    for (int j = 0; j < K; j++) { /* Horner in 64-bit arithmetic */
        unsigned long long v = 0;
        for (int i = N - 1; i >= 0; i--) v = v * zs[j] + c[i];
        be32_small(want, v);
        CHECK(memcmp(y + 32 * j, want, 32) == 0);
    }
    be32_small(want, c[N - 1]); /* the divisor is monic: the quotient's leading coefficient is p's */
    CHECK(memcmp(q_be + 32 * (N - K - 1), want, 32) == 0);
    ps_scalars_free(q);
    q = NULL;
    CHECK(ps_poly_div_roots(ctx, p, z_be, K, &q, y, NULL) == PS_OK && ps_scalars_len(q) == N - K); /* the remainder is optional */
    ps_scalars_free(q);
    q = NULL;

    /* one proof for both points */
    uint8_t commit[96], y2[K * 32], proof[96], bad[K * 32];
    CHECK(ps_kzg_commit(ctx, tau_g1, p, commit) == PS_OK);
    CHECK(ps_kzg_open_set(ctx, tau_g1, p, z_be, K, y2, proof) == PS_OK);
    CHECK(memcmp(y, y2, sizeof y) == 0);
    int ok = -1;
    CHECK(ps_kzg_verify_set(ctx, tau_g1, tau_g2, commit, z_be, y, K, proof, 1, &ok) == PS_OK && ok == 1);
    memcpy(bad, y, sizeof bad);
    bad[63] ^= 1; /* another value at the second point */
    CHECK(ps_kzg_verify_set(ctx, tau_g1, tau_g2, commit, z_be, bad, K, proof, 1, &ok) == PS_OK && ok == 0);
    memcpy(bad, y + 32, 32); /* the two values swapped */
    memcpy(bad + 32, y, 32);
    CHECK(ps_kzg_verify_set(ctx, tau_g1, tau_g2, commit, z_be, bad, K, proof, 1, &ok) == PS_OK && ok == 0);

    /* argument checks: two equal points, the empty set, a point that is not below r, strings that are too short */
    uint8_t twice[K * 32], big[K * 32];
    memcpy(twice, z_be, 32);
    memcpy(twice + 32, z_be, 32);
    memset(big, 0xff, sizeof big);
    CHECK(ps_kzg_open_set(ctx, tau_g1, p, twice, K, y2, proof) == PS_ERR_ARG);
    CHECK(ps_poly_div_roots(ctx, p, twice, K, &q, y2, NULL) == PS_ERR_ARG && q == NULL);
    CHECK(ps_kzg_open_set(ctx, tau_g1, p, z_be, 0, y2, proof) == PS_ERR_ARG);
    CHECK(ps_poly_div_roots(ctx, p, z_be, 0, &q, y2, NULL) == PS_ERR_ARG && q == NULL);
    CHECK(ps_kzg_open_set(ctx, tau_g1, p, big, K, y2, proof) == PS_ERR_ENCODING);
    ps_points *shorter = NULL, *shorter2 = NULL;
    CHECK(ps_points_slice(tau_g1, 0, N - 1, &shorter) == PS_OK && ps_points_slice(tau_g2, 0, K, &shorter2) == PS_OK);
    CHECK(ps_kzg_open_set(ctx, shorter, p, z_be, K, y2, proof) == PS_ERR_LENGTH);
    CHECK(ps_kzg_verify_set(ctx, tau_g1, shorter2, commit, z_be, y, K, proof, 1, &ok) == PS_ERR_LENGTH);
    CHECK(ps_kzg_open_set(ctx, tau_g1, p, z_be, K, y2, proof) == PS_OK);

    print_hex("q", q_be, sizeof q_be);
    print_hex("y", y, sizeof y);
    print_hex("rem", rem, sizeof rem);
    print_hex("proof", proof, sizeof proof);

    ps_points_free(shorter);
    ps_points_free(shorter2);
    ps_scalars_free(p);
    ps_points_free(tau_g1);
    ps_points_free(tau_g2);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg_set ok\n");
    return 0;
}
