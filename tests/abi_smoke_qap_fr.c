/* abi_smoke_qap_fr.c -- a circuit with field-valued coefficients through the C ABI, the way a cgo caller uses it: plain C99,
 * nothing but include/playsnark_hip.h.  Three rounds of x -> (x + c_i)^3 (6 gates, 8 variables [const, x, out, t0, x1, t1, x2,
 * t2], nbIO = 3) with the round constants 2^64 (the first magnitude the 64-bit column sums cannot hold), r - 1 (-1 written
 * out: narrow) and 2^253 + 5, all as 32-byte big-endian values:
 *   - ps_qap_create_fr, ps_qap_wide_entries = (2, 4, 0); a coefficient equal to r is PS_ERR_ENCODING, a column index out of
 *     range PS_ERR_ARG;
 *   - the witness satisfies the circuit (ps_qap_is_valid);
 *   - ps_groth16_setup_from_srs over a phase-1 string from small caller-chosen values: NioLP, IoLP, XiT byte-equal to
 *     ps_groth16_setup with delta = gamma = 1 (the column sums over points with wide coefficients);
 *   - one proof under that key, verified with ps_groth16_verify; rejected with another public input.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_qap_fr.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_qap_fr
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_qap_fr: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

#define N 6     /* gates */
#define NVARS 8
#define DIFF 5  /* nbVars - nbIO */

static const char* ONE = "0000000000000000000000000000000000000000000000000000000000000001";
static const char* C0 = "0000000000000000000000000000000000000000000000010000000000000000";  /* 2^64 */
static const char* C1 = "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000";  /* r - 1 */
static const char* C2 = "2000000000000000000000000000000000000000000000000000000000000005";  /* 2^253 + 5 */
static const char* R_HEX = "73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001"; /* r itself: not canonical */
/* x = 3 and what the three rounds make of it, mod r */
static const char* WITNESS[NVARS] = {
    "0000000000000000000000000000000000000000000000000000000000000001",
    "0000000000000000000000000000000000000000000000000000000000000003",
    "1217d15b6d7965af30c9c946fa3a780103c5bcaca60ac48df61a92790c142da9",
    "0000000000000000000000000000000100000000000000060000000000000009",
    "00000000000000010000000000000009000000000000001b000000000000001b",
    "39a57377c968fcb99f9b9fc57bc15a7105f9a77cafca1e03fb2021460c7f8beb",
    "3c8cf6aa5c6e62511c892cf6fbb30b56336f5ffe1eb136e73f5e745bd05eb41e",
    "49914021ac8ff75410613b3d226b3974b0fdb4434ab4cb9d2085892b4523b65c",
};

static void be32_hex(uint8_t out[32], const char* hex) {
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        sscanf(hex + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

static void be32_small(uint8_t out[32], unsigned long long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

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

    /* rows = gates; round i:  (cur + c_i const) (cur + c_i const) = t_i,   t_i (cur + c_i const) = next */
    const uint32_t l_ptr[N + 1] = {0, 2, 3, 5, 6, 8, 9}, l_col[9] = {1, 0, 3, 4, 0, 5, 6, 0, 7};
    const char* l_src[9] = {ONE, C0, ONE, ONE, C1, ONE, ONE, C2, ONE};
    const uint32_t r_ptr[N + 1] = {0, 2, 4, 6, 8, 10, 12}, r_col[12] = {1, 0, 1, 0, 4, 0, 4, 0, 6, 0, 6, 0};
    const char* r_src[12] = {ONE, C0, ONE, C0, ONE, C1, ONE, C1, ONE, C2, ONE, C2};
    const uint32_t o_ptr[N + 1] = {0, 1, 2, 3, 4, 5, 6}, o_col[6] = {3, 4, 5, 6, 7, 2};
    uint32_t bad_col[6] = {3, 4, 5, 6, NVARS, 2};
    uint8_t l_val[9 * 32], r_val[12 * 32], o_val[6 * 32], bad_val[12 * 32];
    for (int e = 0; e < 9; e++) be32_hex(l_val + 32 * e, l_src[e]);
    for (int e = 0; e < 12; e++) be32_hex(r_val + 32 * e, r_src[e]);
    for (int e = 0; e < 6; e++) be32_hex(o_val + 32 * e, ONE);
    memcpy(bad_val, r_val, sizeof r_val);
    be32_hex(bad_val + 32 * 7, R_HEX);
    const ps_csr_fr L = {l_ptr, l_col, l_val}, R = {r_ptr, r_col, r_val}, O = {o_ptr, o_col, o_val};
    const ps_csr_fr R_bad = {r_ptr, r_col, bad_val}, O_bad = {o_ptr, bad_col, o_val};
    ps_qap* qap = NULL;
    CHECK(ps_qap_create_fr(ctx, N, NVARS, 3, &L, &R_bad, &O, &qap) == PS_ERR_ENCODING && qap == NULL);
    CHECK(ps_qap_create_fr(ctx, N, NVARS, 3, &L, &R, &O_bad, &qap) == PS_ERR_ARG && qap == NULL);
    CHECK(ps_qap_create_fr(ctx, N, NVARS, 3, &L, NULL, &O, &qap) == PS_ERR_ARG);
    CHECK(ps_qap_create_fr(ctx, N, NVARS, 3, &L, &R, &O, &qap) == PS_OK);
    size_t wide[3] = {9, 9, 9};
    CHECK(ps_qap_wide_entries(qap, wide) == PS_OK && wide[0] == 2 && wide[1] == 4 && wide[2] == 0);

    uint8_t wit[NVARS * 32];
    for (int i = 0; i < NVARS; i++) be32_hex(wit + 32 * i, WITNESS[i]);
    ps_scalars *sol = NULL, *io = NULL;
    CHECK(ps_scalars_upload(ctx, wit, NVARS, &sol) == PS_OK && ps_scalars_upload(ctx, wit, DIFF, &io) == PS_OK);
    int ok = -1;
    CHECK(ps_qap_is_valid(ctx, qap, sol, &ok) == PS_OK && ok == 1);

    /* phase 1, as a ceremony would publish it (x = 13, off the nodes 1..11; alpha = 5, beta = 7: every power fits 64 bits) */
    const unsigned long long x = 13, alpha = 5, beta = 7;
    ps_points *tau1 = NULL, *tau2 = NULL, *atau = NULL, *btau = NULL, *b2 = NULL;
    CHECK(powers(ctx, PS_G1, 1, x, 2 * N - 1, &tau1) == PS_OK && powers(ctx, PS_G2, 1, x, N, &tau2) == PS_OK);
    CHECK(powers(ctx, PS_G1, alpha, x, N, &atau) == PS_OK && powers(ctx, PS_G1, beta, x, N, &btau) == PS_OK);
    CHECK(powers(ctx, PS_G2, beta, x, 1, &b2) == PS_OK);
    ps_groth16_srs srs;
    memset(&srs, 0, sizeof srs);
    srs.tau_g1 = tau1; srs.tau_g2 = tau2; srs.alpha_tau_g1 = atau; srs.beta_tau_g1 = btau;
    CHECK(ps_points_download(ctx, b2, 0, 1, srs.beta_g2) == PS_OK);

    /* the circuit's key from the string: the column sums over points, against the key made from the values in the clear */
    ps_groth16_crs k0, ref;
    CHECK(ps_groth16_setup_from_srs(ctx, qap, &srs, &k0) == PS_OK);
    ps_groth16_toxic tw;
    be32_small(tw.alpha, alpha); be32_small(tw.beta, beta); be32_small(tw.delta, 1); be32_small(tw.x, x); be32_small(tw.gamma, 1);
    CHECK(ps_groth16_setup(ctx, qap, &tw, &ref) == PS_OK);
    CHECK(ps_points_len(k0.io_lp) == DIFF && ps_points_len(k0.nio_lp) == NVARS - DIFF && ps_points_len(k0.xi_t) == N - 1);
    CHECK(same_points(ctx, k0.nio_lp, ref.nio_lp) && same_points(ctx, k0.io_lp, ref.io_lp) && same_points(ctx, k0.xi_t, ref.xi_t));

    /* a proof under that key */
    ps_groth16_pk pk;
    memset(&pk, 0, sizeof pk); /* the header requires zero-initialised structs */
    memcpy(pk.alpha, k0.alpha, 96); memcpy(pk.beta, k0.beta, 96); memcpy(pk.delta, k0.delta, 96);
    memcpy(pk.beta2, k0.beta2, 192); memcpy(pk.delta2, k0.delta2, 192);
    pk.xi = k0.xi; pk.xi2 = k0.xi2; pk.nio_lp = k0.nio_lp; pk.xi_t = k0.xi_t;
    pk.lxi = k0.lxi; pk.lxi2 = k0.lxi2; pk.lxi_t = k0.lxi_t;
    ps_groth16_vk vk;
    memset(&vk, 0, sizeof vk);
    memcpy(vk.alpha, k0.alpha, 96); memcpy(vk.beta2, k0.beta2, 192); memcpy(vk.gamma, k0.gamma, 192); memcpy(vk.delta2, k0.delta2, 192);
    vk.io_lp = k0.io_lp;
    uint8_t r[32], s[32], A[96], B[192], C[96];
    be32_small(r, 1000003ull); be32_small(s, 777ull);
    CHECK(ps_groth16_prove(ctx, &pk, qap, sol, r, s, A, B, C) == PS_OK);
    ok = -1;
    CHECK(ps_groth16_verify(ctx, &vk, io, A, B, C, &ok) == PS_OK && ok == 1);
    ps_scalars* other_io = NULL;
    wit[32 + 31] ^= 1; /* another x */
    CHECK(ps_scalars_upload(ctx, wit, DIFF, &other_io) == PS_OK);
    CHECK(ps_groth16_verify(ctx, &vk, other_io, A, B, C, &ok) == PS_OK && ok == 0);

    crs_free(&k0); crs_free(&ref);
    ps_scalars_free(io); ps_scalars_free(other_io); ps_scalars_free(sol);
    ps_points_free(tau1); ps_points_free(tau2); ps_points_free(atau); ps_points_free(btau); ps_points_free(b2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_qap_fr ok\n");
    return 0;
}
