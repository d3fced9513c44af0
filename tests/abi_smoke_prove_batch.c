/* abi_smoke_prove_batch.c -- ps_groth16_prove_batch, ps_msm_batch and ps_msm_batch_set_chunk through the C ABI, the way a cgo
 * caller uses them: plain C99, nothing but include/playsnark_hip.h.  The circuit is the reference's toy gate pattern
 * (Mul, Mul, Add, AddConst; r1cs.go:178-198) tiled to 7 gates, 9 variables [const, x, out, u, v, w, x', u', v'], nbIO = 3;
 * three witnesses from x = 3, 5, 7.  Checks
 *   - the three proofs of ONE batch call against three ps_groth16_prove calls: the same 384 bytes each, and again with passes
 *     of two members (ps_msm_batch_set_chunk);
 *   - a violated gate in witness 1: with `valid` PS_OK and [1, 0, 1], proof 1 zero bytes, the others unchanged; without
 *     `valid` PS_ERR_NOT_DIVISIBLE, and the context proves right after;
 *   - a key without its Lagrange form is PS_ERR_ARG; a solution vector one short is PS_ERR_ARG; no proofs at all is PS_OK;
 *   - ps_msm_batch of two scalar vectors over Xi against two ps_msm calls on slices; a wrong length is PS_ERR_LENGTH.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_prove_batch.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_prove_batch
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_prove_batch: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define K 3
#define N 7
#define M 9

static void witness(int64_t w[M], int64_t x) {
    const int64_t u = x * x, v = u * x, ww = v + x, x2 = ww + 5, u2 = x2 * x2, v2 = u2 * x2;
    w[0] = 1; w[1] = x; w[2] = v2 + x2; w[3] = u; w[4] = v; w[5] = ww; w[6] = x2; w[7] = u2; w[8] = v2;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    const uint32_t l_ptr[N + 1] = {0, 1, 2, 4, 6, 7, 8, 10}, l_col[10] = {1, 3, 4, 1, 0, 5, 6, 7, 8, 6};
    const int64_t l_val[10] = {1, 1, 1, 1, 5, 1, 1, 1, 1, 1};
    const uint32_t r_ptr[N + 1] = {0, 1, 2, 3, 4, 5, 6, 7}, r_col[N] = {1, 1, 0, 0, 6, 6, 0};
    const int64_t r_val[N] = {1, 1, 1, 1, 1, 1, 1};
    const uint32_t o_ptr[N + 1] = {0, 1, 2, 3, 4, 5, 6, 7}, o_col[N] = {3, 4, 5, 6, 7, 8, 2};
    const int64_t o_val[N] = {1, 1, 1, 1, 1, 1, 1};
    const ps_csr L = {l_ptr, l_col, l_val}, R = {r_ptr, r_col, r_val}, O = {o_ptr, o_col, o_val};
    ps_qap* qap = NULL;
    CHECK(ps_qap_create(ctx, N, M, 3, &L, &R, &O, &qap) == PS_OK);

    int64_t wit[K * M];
    for (int j = 0; j < K; j++) witness(wit + M * j, 3 + 2 * j);
    ps_scalars *sols = NULL, *sol[K] = {NULL, NULL, NULL};
    CHECK(ps_scalars_upload_i64(ctx, wit, K * M, &sols) == PS_OK);
    for (int j = 0; j < K; j++) CHECK(ps_scalars_upload_i64(ctx, wit + M * j, M, &sol[j]) == PS_OK);

    ps_groth16_toxic tw;
    be32_small(tw.alpha, 1234577ul); be32_small(tw.beta, 7654321ul); be32_small(tw.delta, 424243ul);
    be32_small(tw.x, 998877665ul); be32_small(tw.gamma, 31337ul);
    ps_groth16_crs crs;
    memset(&crs, 0, sizeof crs);
    CHECK(ps_groth16_setup(ctx, qap, &tw, &crs) == PS_OK);
    ps_groth16_pk pk;
    memset(&pk, 0, sizeof pk); /* the header requires zero-initialised structs */
    memcpy(pk.alpha, crs.alpha, 96); memcpy(pk.beta, crs.beta, 96); memcpy(pk.delta, crs.delta, 96);
    memcpy(pk.beta2, crs.beta2, 192); memcpy(pk.delta2, crs.delta2, 192);
    pk.xi = crs.xi; pk.xi2 = crs.xi2; pk.nio_lp = crs.nio_lp; pk.xi_t = crs.xi_t;
    pk.lxi = crs.lxi; pk.lxi2 = crs.lxi2; pk.lxi_t = crs.lxi_t;
    CHECK(pk.lxi && pk.lxi2 && pk.lxi_t);

    uint8_t r[K * 32], s[K * 32];
    for (int j = 0; j < K; j++) {
        be32_small(r + 32 * j, 1000003ul * (unsigned long)(j + 1));
        be32_small(s + 32 * j, 777ul + 13ul * (unsigned long)j);
    }
    /* three single calls */
    static uint8_t A1[K * 96], B1[K * 192], C1[K * 96];
    for (int j = 0; j < K; j++)
        CHECK(ps_groth16_prove(ctx, &pk, qap, sol[j], r + 32 * j, s + 32 * j, A1 + 96 * j, B1 + 192 * j, C1 + 96 * j) == PS_OK);
    CHECK(memcmp(A1, A1 + 96, 96) != 0);
    /* one batch call */
    static uint8_t A[K * 96], B[K * 192], C[K * 96];
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, sols, K, r, s, A, B, C, NULL) == PS_OK);
    CHECK(!memcmp(A, A1, sizeof A) && !memcmp(B, B1, sizeof B) && !memcmp(C, C1, sizeof C));
    /* passes of two members, and the flags of a valid batch */
    int valid[K] = {-1, -1, -1};
    memset(A, 0xee, sizeof A); memset(B, 0xee, sizeof B); memset(C, 0xee, sizeof C);
    CHECK(ps_msm_batch_set_chunk(ctx, 2) == PS_OK);
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, sols, K, r, s, A, B, C, valid) == PS_OK);
    CHECK(ps_msm_batch_set_chunk(ctx, 0) == PS_OK);
    CHECK(ps_msm_batch_set_chunk(ctx, -1) == PS_ERR_ARG);
    CHECK(valid[0] == 1 && valid[1] == 1 && valid[2] == 1);
    CHECK(!memcmp(A, A1, sizeof A) && !memcmp(B, B1, sizeof B) && !memcmp(C, C1, sizeof C));

    /* witness 1 violates gate 1 (v != u x) */
    int64_t bad[K * M];
    memcpy(bad, wit, sizeof bad);
    bad[M + 4] += 1;
    ps_scalars* bsols = NULL;
    CHECK(ps_scalars_upload_i64(ctx, bad, K * M, &bsols) == PS_OK);
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, bsols, K, r, s, A, B, C, valid) == PS_OK);
    CHECK(valid[0] == 1 && valid[1] == 0 && valid[2] == 1);
    static const uint8_t zeros[192] = {0};
    CHECK(!memcmp(A + 96, zeros, 96) && !memcmp(B + 192, zeros, 192) && !memcmp(C + 96, zeros, 96));
    CHECK(!memcmp(A, A1, 96) && !memcmp(B, B1, 192) && !memcmp(C, C1, 96));
    CHECK(!memcmp(A + 192, A1 + 192, 96) && !memcmp(B + 384, B1 + 384, 192) && !memcmp(C + 192, C1 + 192, 96));
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, bsols, K, r, s, A, B, C, NULL) == PS_ERR_NOT_DIVISIBLE);
    CHECK(strstr(ps_last_error(), "witness 1 ") != NULL);
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, sols, K, r, s, A, B, C, NULL) == PS_OK);
    CHECK(!memcmp(A, A1, sizeof A) && !memcmp(B, B1, sizeof B) && !memcmp(C, C1, sizeof C));

    /* refusals */
    ps_groth16_pk mono = pk;
    mono.lxi = NULL; mono.lxi2 = NULL; mono.lxi_t = NULL;
    CHECK(ps_groth16_prove_batch(ctx, &mono, qap, sols, K, r, s, A, B, C, NULL) == PS_ERR_ARG);
    CHECK(strstr(ps_last_error(), "ps_points_monomial_to_lagrange") != NULL);
    ps_scalars *shorter = NULL, *none = NULL;
    CHECK(ps_scalars_slice(sols, 0, K * M - 1, &shorter) == PS_OK && ps_scalars_slice(sols, 0, 0, &none) == PS_OK);
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, shorter, K, r, s, A, B, C, NULL) == PS_ERR_ARG);
    CHECK(ps_groth16_prove_batch(ctx, &pk, qap, none, 0, NULL, NULL, NULL, NULL, NULL, NULL) == PS_OK);

    /* the sum underneath: two scalar vectors over Xi */
    uint8_t k2[2 * N * 32], two[2 * 96], each[2 * 96];
    for (int i = 0; i < 2 * N; i++) be32_small(k2 + 32 * i, 1000000007ul * (unsigned long)(i + 1) + 12345ul);
    ps_scalars *kv = NULL, *half = NULL;
    CHECK(ps_scalars_upload(ctx, k2, 2 * N, &kv) == PS_OK);
    CHECK(ps_msm_batch(ctx, crs.xi, kv, 2, two) == PS_OK);
    for (int j = 0; j < 2; j++) {
        CHECK(ps_scalars_slice(kv, (size_t)(N * j), N, &half) == PS_OK);
        CHECK(ps_msm(ctx, crs.xi, half, each + 96 * j) == PS_OK);
        ps_scalars_free(half);
    }
    CHECK(!memcmp(two, each, sizeof two) && memcmp(two, two + 96, 96) != 0);
    CHECK(ps_msm_batch(ctx, crs.xi, kv, 3, two) == PS_ERR_LENGTH);
    CHECK(ps_msm_batch(ctx, crs.xi, none, 0, NULL) == PS_OK);

    ps_scalars_free(kv); ps_scalars_free(shorter); ps_scalars_free(none); ps_scalars_free(bsols); ps_scalars_free(sols);
    for (int j = 0; j < K; j++) ps_scalars_free(sol[j]);
    ps_points_free(crs.xi); ps_points_free(crs.xi2); ps_points_free(crs.io_lp); ps_points_free(crs.nio_lp); ps_points_free(crs.xi_t);
    ps_points_free(crs.lxi); ps_points_free(crs.lxi2); ps_points_free(crs.lxi_t);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_prove_batch ok\n");
    return 0;
}
