/* abi_smoke_srs_phase1.c -- phase 1 of a Groth16 ceremony through the C ABI, the way a cgo caller uses it: plain C99, nothing
 * but include/playsnark_hip.h.  For a string of the toy size (4 gates: 7, 4, 4, 4 points):
 *   - ps_scalars_powers: [3, 3*11, 3*11^2, ..] against 64-bit arithmetic; n = 0; a scalar that is not below r: PS_ERR_ENCODING;
 *   - the trivial string (every point a generator) passes ps_groth16_srs_check;
 *   - ps_groth16_srs_contribute with small (t, a, b) gives, byte for byte, the string ps_points_from_scalars makes for them; a
 *     second fold gives the string of the products; t = 0: PS_ERR_ARG;
 *   - ps_groth16_srs_check accepts both, and rejects the string with its LAST tau_g1 point replaced, and one whose beta_g2
 *     belongs to another beta; too few weights: PS_ERR_LENGTH;
 *   - ps_groth16_srs_check_update accepts each fold with its own share and rejects it with the other fold's share.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_srs_phase1.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_srs_phase1
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_srs_phase1: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define N 4 /* gates */
#define LONGEST (2 * N - 1)

/* {scale * x^i G}, i < cnt, from scalars held in the clear (what a test may do and a ceremony must not) */
static int powers(ps_ctx* ctx, int group, unsigned long long scale, unsigned long long x, size_t cnt, ps_points** out) {
    uint8_t k[LONGEST * 32];
    unsigned long long p = scale;
    for (size_t i = 0; i < cnt; i++, p *= x) be32_small(k + 32 * i, p);
    ps_scalars* s = NULL;
    int rc = ps_scalars_upload(ctx, k, cnt, &s);
    if (rc == PS_OK) rc = ps_points_from_scalars(ctx, group, s, out);
    ps_scalars_free(s);
    return rc;
}
static int clear_string(ps_ctx* ctx, unsigned long long x, unsigned long long alpha, unsigned long long beta, ps_groth16_srs* out) {
    ps_points *t1 = NULL, *t2 = NULL, *ta = NULL, *tb = NULL, *b2 = NULL;
    memset(out, 0, sizeof *out);
    if (powers(ctx, PS_G1, 1, x, LONGEST, &t1) != PS_OK || powers(ctx, PS_G2, 1, x, N, &t2) != PS_OK) return 0;
    if (powers(ctx, PS_G1, alpha, x, N, &ta) != PS_OK || powers(ctx, PS_G1, beta, x, N, &tb) != PS_OK) return 0;
    if (powers(ctx, PS_G2, beta, x, 1, &b2) != PS_OK || ps_points_download(ctx, b2, 0, 1, out->beta_g2) != PS_OK) return 0;
    ps_points_free(b2);
    out->tau_g1 = t1; out->tau_g2 = t2; out->alpha_tau_g1 = ta; out->beta_tau_g1 = tb;
    return 1;
}
static void srs_free(ps_groth16_srs* s) {
    ps_points_free((ps_points*)s->tau_g1); ps_points_free((ps_points*)s->tau_g2);
    ps_points_free((ps_points*)s->alpha_tau_g1); ps_points_free((ps_points*)s->beta_tau_g1);
}

static int same_points(ps_ctx* ctx, const ps_points* a, const ps_points* b) {
    uint8_t x[LONGEST * 192], y[LONGEST * 192];
    const size_t n = ps_points_len(a), wb = ps_points_group(a) == PS_G1 ? 96 : 192;
    if (n != ps_points_len(b) || n > LONGEST || ps_points_group(a) != ps_points_group(b)) return 0;
    if (ps_points_download(ctx, a, 0, n, x) != PS_OK || ps_points_download(ctx, b, 0, n, y) != PS_OK) return 0;
    return memcmp(x, y, wb * n) == 0;
}
static int same_string(ps_ctx* ctx, const ps_groth16_srs* a, const ps_groth16_srs* b) {
    return same_points(ctx, a->tau_g1, b->tau_g1) && same_points(ctx, a->tau_g2, b->tau_g2) && same_points(ctx, a->alpha_tau_g1, b->alpha_tau_g1) &&
           same_points(ctx, a->beta_tau_g1, b->beta_tau_g1) && memcmp(a->beta_g2, b->beta_g2, 192) == 0;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    /* the power sequence */
    uint8_t s_be[32], c_be[32], big[32], got[LONGEST * 32], want[32];
    be32_small(s_be, 11); be32_small(c_be, 3);
    memset(big, 0xff, 32);
    ps_scalars* pw = NULL;
    CHECK(ps_scalars_powers(ctx, s_be, c_be, LONGEST, &pw) == PS_OK && ps_scalars_len(pw) == LONGEST);
    CHECK(ps_scalars_download(ctx, pw, 0, LONGEST, got) == PS_OK);
    unsigned long long p = 3;
    for (int i = 0; i < LONGEST; i++, p *= 11) {
        be32_small(want, p);
        CHECK(memcmp(got + 32 * i, want, 32) == 0);
    }
    ps_scalars_free(pw);
    CHECK(ps_scalars_powers(ctx, s_be, c_be, 0, &pw) == PS_OK && ps_scalars_len(pw) == 0);
    ps_scalars_free(pw);
    CHECK(ps_scalars_powers(ctx, big, c_be, 4, &pw) == PS_ERR_ENCODING);

    uint8_t rho[LONGEST * 32];
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < LONGEST; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(41 * i + 13 * k + 3); /* 128-bit weights */
    int ok = -1;

    /* the trivial string, then two folds */
    const unsigned long long t1 = 11, a1 = 5, b1 = 7, t2 = 3, a2 = 13, b2 = 2;
    ps_groth16_srs s0, s1, s2, want1, want2, bad;
    ps_groth16_srs_share sh1, sh2;
    uint8_t t_be[32], a_be[32], b_be[32], zero[32];
    be32_small(zero, 0);
    CHECK(clear_string(ctx, 1, 1, 1, &s0));
    CHECK(ps_groth16_srs_check(ctx, &s0, rho, LONGEST - 1, 1, &ok) == PS_OK && ok == 1);
    be32_small(t_be, t1); be32_small(a_be, a1); be32_small(b_be, b1);
    CHECK(ps_groth16_srs_contribute(ctx, &s0, zero, a_be, b_be, &s1, &sh1) == PS_ERR_ARG);
    CHECK(ps_groth16_srs_contribute(ctx, &s0, big, a_be, b_be, &s1, &sh1) == PS_ERR_ENCODING);
    CHECK(ps_groth16_srs_contribute(ctx, &s0, t_be, a_be, b_be, &s1, &sh1) == PS_OK);
    be32_small(t_be, t2); be32_small(a_be, a2); be32_small(b_be, b2);
    CHECK(ps_groth16_srs_contribute(ctx, &s1, t_be, a_be, b_be, &s2, &sh2) == PS_OK);
    CHECK(clear_string(ctx, t1, a1, b1, &want1) && clear_string(ctx, t1 * t2, a1 * a2, b1 * b2, &want2));
    CHECK(same_string(ctx, &s1, &want1) && same_string(ctx, &s2, &want2));
    CHECK(memcmp(sh2.b_g2, sh1.b_g2, 192) != 0);

    /* anybody's checks */
    ok = -1;
    CHECK(ps_groth16_srs_check(ctx, &s1, rho, LONGEST - 1, 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_srs_check(ctx, &s2, rho, LONGEST, 0, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_srs_check(ctx, &s2, rho, LONGEST - 2, 1, &ok) == PS_ERR_LENGTH);
    /* the last power replaced by a point of the subgroup that is not tau^6 G1 */
    uint8_t raw[LONGEST * 96];
    ps_points* tampered = NULL;
    CHECK(ps_points_download(ctx, s2.tau_g1, 0, LONGEST, raw) == PS_OK);
    memcpy(raw + 96 * (LONGEST - 1), raw + 96 * (LONGEST - 2), 96);
    CHECK(ps_points_upload(ctx, PS_G1, raw, LONGEST, PS_FMT_AFFINE, &tampered) == PS_OK);
    bad = s2;
    bad.tau_g1 = tampered;
    CHECK(ps_groth16_srs_check(ctx, &bad, rho, LONGEST - 1, 1, &ok) == PS_OK && ok == 0);
    bad = s2;
    memcpy(bad.beta_g2, s1.beta_g2, 192);
    CHECK(ps_groth16_srs_check(ctx, &bad, rho, LONGEST - 1, 1, &ok) == PS_OK && ok == 0);

    CHECK(ps_groth16_srs_check_update(ctx, &s0, &s1, &sh1, rho, LONGEST - 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_srs_check_update(ctx, &s1, &s2, &sh2, rho, LONGEST - 1, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_srs_check_update(ctx, &s1, &s2, &sh1, rho, LONGEST - 1, &ok) == PS_OK && ok == 0);
    CHECK(ps_groth16_srs_check_update(ctx, &s0, &s2, &sh2, rho, LONGEST - 1, &ok) == PS_OK && ok == 0);
    CHECK(ps_groth16_srs_check_update(ctx, &s1, &s2, &sh2, rho, 1, &ok) == PS_ERR_LENGTH);

    ps_points_free(tampered);
    srs_free(&s0); srs_free(&s1); srs_free(&s2); srs_free(&want1); srs_free(&want2);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_srs_phase1 ok\n");
    return 0;
}
