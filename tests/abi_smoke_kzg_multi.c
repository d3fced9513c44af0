/* abi_smoke_kzg_multi.c -- two polynomials opened at one point with ONE proof, through the C ABI the way a cgo caller uses it:
 * plain C99, nothing but include/playsnark_hip.h.  Over a string in the clear (tau = 11: 6 points of tau_g1, tau G2),
 * p0 = (3, 1, 4, 1, 5), p1 = (2, 7) and the weights (1, 2):
 *   - ps_scalars_lincomb gives p0 + 2 p1 = (7, 15, 4, 1, 5);
 *   - ps_kzg_open_multi at z = 7 gives both values and one proof, which ps_kzg_verify_multi accepts and, with a changed value,
 *     rejects;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_multi_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg_multi.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg_multi
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_kzg_multi: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
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

#define N0 5     /* coefficients of p0 */
#define N1 2     /* coefficients of p1 */
#define LEN 6    /* points of the string: longer than both */
#define M 2      /* polynomials */
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
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    ps_points *tau_g1 = NULL, *tau_g2 = NULL;
    uint8_t t2[192];
    CHECK(powers(ctx, PS_G1, TAU, LEN, &tau_g1) == PS_OK && powers(ctx, PS_G2, TAU, 2, &tau_g2) == PS_OK);
    CHECK(ps_points_download(ctx, tau_g2, 1, 1, t2) == PS_OK);

    const unsigned long long c0[N0] = {3, 1, 4, 1, 5}, c1[N1] = {2, 7}, sum[N0] = {7, 15, 4, 1, 5};
    uint8_t p0_be[N0 * 32], p1_be[N1 * 32], z_be[32], coef[M * 32], want[32];
    for (int i = 0; i < N0; i++) be32_small(p0_be + 32 * i, c0[i]);
    for (int i = 0; i < N1; i++) be32_small(p1_be + 32 * i, c1[i]);
    be32_small(z_be, 7);
    be32_small(coef, 1);
    be32_small(coef + 32, 2);
    ps_scalars* polys[M] = {NULL, NULL};
    CHECK(ps_scalars_upload(ctx, p0_be, N0, &polys[0]) == PS_OK && ps_scalars_upload(ctx, p1_be, N1, &polys[1]) == PS_OK);
    const ps_scalars* const in[M] = {polys[0], polys[1]};

    /* the combination itself: one row, as long as the longer input */
    ps_scalars* f = NULL;
    uint8_t f_be[N0 * 32];
    CHECK(ps_scalars_lincomb(ctx, in, M, coef, 1, &f) == PS_OK && ps_scalars_len(f) == N0);
    CHECK(ps_scalars_download(ctx, f, 0, N0, f_be) == PS_OK);
    for (int i = 0; i < N0; i++) {
        be32_small(want, sum[i]);
        CHECK(memcmp(f_be + 32 * i, want, 32) == 0);
    }
    ps_scalars_free(f);
    f = NULL;
    CHECK(ps_scalars_lincomb(ctx, in, M, coef, 0, &f) == PS_OK && ps_scalars_len(f) == 0); /* t = 0 */
    ps_scalars_free(f);
    CHECK(ps_scalars_lincomb(ctx, in, 0, coef, 1, &f) == PS_ERR_ARG);

    /* both polynomials at z = 7, ONE proof */
    uint8_t commits[M * 96], y[M * 32], proof[96];
    for (int i = 0; i < M; i++) CHECK(ps_kzg_commit(ctx, tau_g1, polys[i], commits + 96 * i) == PS_OK);
    CHECK(ps_kzg_open_multi(ctx, tau_g1, in, M, z_be, 1, coef, y, proof) == PS_OK);
    be32_small(want, 3 + 7 * (1 + 7 * (4 + 7 * (1 + 7 * 5ull)))); /* Horner in 64-bit arithmetic */
    CHECK(memcmp(y, want, 32) == 0);
    be32_small(want, 2 + 7 * 7ull);
    CHECK(memcmp(y + 32, want, 32) == 0);

    uint8_t rho[32], bad[M * 32];
    memset(rho, 0, sizeof rho);
    for (int b = 16; b < 32; b++) rho[b] = (uint8_t)(13 * b + 3); /* a 128-bit weight */
    int ok = -1;
    CHECK(ps_kzg_verify_multi(ctx, t2, commits, M, z_be, 1, coef, y, proof, rho, 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_kzg_verify_multi(ctx, t2, commits, M, z_be, 0, coef, y, proof, rho, 1, &ok) == PS_OK && ok == 1); /* t = 0 */
    memcpy(bad, y, sizeof bad);
    bad[63] ^= 1; /* another value for p1 */
    CHECK(ps_kzg_verify_multi(ctx, t2, commits, M, z_be, 1, coef, bad, proof, rho, 1, &ok) == PS_OK && ok == 0);
    /* argument checks: a weight that is not below r, a string shorter than the longer polynomial, a zero rho */
    uint8_t big[M * 32], zero[32];
    memset(big, 0xff, sizeof big);
    memset(zero, 0, sizeof zero);
    CHECK(ps_kzg_open_multi(ctx, tau_g1, in, M, z_be, 1, big, y, proof) == PS_ERR_ENCODING);
    ps_points* shorter = NULL;
    CHECK(ps_points_slice(tau_g1, 0, N0 - 1, &shorter) == PS_OK);
    CHECK(ps_kzg_open_multi(ctx, shorter, in, M, z_be, 1, coef, y, proof) == PS_ERR_LENGTH);
    CHECK(ps_kzg_verify_multi(ctx, t2, commits, M, z_be, 1, coef, y, proof, zero, 1, &ok) == PS_ERR_ARG);
    CHECK(ps_kzg_open_multi(ctx, tau_g1, in, M, z_be, 1, coef, y, proof) == PS_OK);

    print_hex("y", y, sizeof y);
    print_hex("proof", proof, sizeof proof);

    ps_points_free(shorter);
    ps_scalars_free(polys[0]);
    ps_scalars_free(polys[1]);
    ps_points_free(tau_g1);
    ps_points_free(tau_g2);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg_multi ok\n");
    return 0;
}
