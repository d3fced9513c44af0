/* abi_smoke_phgr13_batch.c -- ps_phgr13_prove_batch and ps_msm_batch_multi through the C ABI, the way a cgo caller uses them:
 * plain C99, nothing but include/playsnark_hip.h.  The circuit is the reference's toy gate pattern (Mul, Mul, Add, AddConst;
 * r1cs.go:178-198) tiled to 7 gates, 9 variables [const, x, out, u, v, w, x', u', v'], nbIO = 3; three witnesses from
 * x = 3, 5, 7.  Checks
 *   - the three proofs of ONE batch call against three ps_phgr13_prove calls: the same 864 bytes each, and again with passes
 *     of two members (ps_msm_batch_set_chunk);
 *   - a violated gate in witness 1: with `valid` PS_OK and [1, 0, 1], proof 1 zero bytes, the others unchanged; without
 *     `valid` PS_ERR_NOT_DIVISIBLE naming the witness, and the context proves right after;
 *   - a key without lgsi is PS_ERR_ARG naming the conversion; a solution vector one short is PS_ERR_ARG; no proofs is PS_OK;
 *   - ps_msm_batch_multi of the three witnesses over {vs, ws (G2), ys} with stride M and first = diff against ps_msm on
 *     slices, and against the proofs' own vss / wss / yss; refusals with their codes.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_phgr13_batch.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_phgr13_batch
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_phgr13_batch: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
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
#define NIO 3
#define DIFF (M - NIO) /* pinochio.go:219 */
#define NN (M - DIFF) /* points of each solution array: computeSolCommit runs over solution[diff:] */

static void witness(int64_t w[M], int64_t x) {
    const int64_t u = x * x, v = u * x, ww = v + x, x2 = ww + 5, u2 = x2 * x2, v2 = u2 * x2;
    w[0] = 1; w[1] = x; w[2] = v2 + x2; w[3] = u; w[4] = v; w[5] = ww; w[6] = x2; w[7] = u2; w[8] = v2;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(sizeof(ps_phgr13_proof) == 864);
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
    CHECK(ps_qap_create(ctx, N, M, NIO, &L, &R, &O, &qap) == PS_OK);

    int64_t wit[K * M];
    for (int j = 0; j < K; j++) witness(wit + M * j, 3 + 2 * j);
    ps_scalars *sols = NULL, *sol[K] = {NULL, NULL, NULL};
    CHECK(ps_scalars_upload_i64(ctx, wit, K * M, &sols) == PS_OK);
    for (int j = 0; j < K; j++) CHECK(ps_scalars_upload_i64(ctx, wit + M * j, M, &sol[j]) == PS_OK);

    ps_phgr13_toxic tw;
    be32_small(tw.s, 998877665ul); be32_small(tw.av, 1234577ul); be32_small(tw.aw, 7654321ul); be32_small(tw.ay, 424243ul);
    be32_small(tw.rv, 31337ul); be32_small(tw.rw, 271829ul); be32_small(tw.beta, 3141593ul); be32_small(tw.gamma, 1618033ul);
    ps_phgr13_crs crs;
    memset(&crs, 0, sizeof crs);
    CHECK(ps_phgr13_setup(ctx, qap, &tw, &crs) == PS_OK);
    ps_phgr13_ek ek;
    memset(&ek, 0, sizeof ek); /* the header requires zero-initialised structs */
    ek.vs = crs.vs; ek.ws = crs.ws; ek.ys = crs.ys; ek.vas = crs.vas; ek.was = crs.was; ek.yas = crs.yas;
    ek.gsi = crs.gsi; ek.vbs = crs.vbs; ek.wbs = crs.wbs; ek.ybs = crs.ybs; ek.lgsi = crs.lgsi;
    CHECK(ek.lgsi != NULL);

    /* three single calls */
    static ps_phgr13_proof one[K], got[K];
    for (int j = 0; j < K; j++) CHECK(ps_phgr13_prove(ctx, &ek, qap, sol[j], &one[j]) == PS_OK);
    CHECK(memcmp(&one[0], &one[1], sizeof one[0]) != 0);
    /* one batch call */
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, sols, K, got, NULL) == PS_OK);
    CHECK(!memcmp(got, one, sizeof got));
    /* passes of two members, and the flags of a valid batch */
    int valid[K] = {-1, -1, -1};
    memset(got, 0xee, sizeof got);
    CHECK(ps_msm_batch_set_chunk(ctx, 2) == PS_OK);
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, sols, K, got, valid) == PS_OK);
    CHECK(ps_msm_batch_set_chunk(ctx, 0) == PS_OK);
    CHECK(valid[0] == 1 && valid[1] == 1 && valid[2] == 1);
    CHECK(!memcmp(got, one, sizeof got));

    /* witness 1 violates gate 1 (v != u x) */
    int64_t bad[K * M];
    memcpy(bad, wit, sizeof bad);
    bad[M + 4] += 1;
    ps_scalars* bsols = NULL;
    CHECK(ps_scalars_upload_i64(ctx, bad, K * M, &bsols) == PS_OK);
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, bsols, K, got, valid) == PS_OK);
    CHECK(valid[0] == 1 && valid[1] == 0 && valid[2] == 1);
    static const ps_phgr13_proof zero = {{0}};
    CHECK(!memcmp(&got[1], &zero, sizeof zero));
    CHECK(!memcmp(&got[0], &one[0], sizeof zero) && !memcmp(&got[2], &one[2], sizeof zero));
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, bsols, K, got, NULL) == PS_ERR_NOT_DIVISIBLE);
    CHECK(strstr(ps_last_error(), "witness 1 ") != NULL);
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, sols, K, got, NULL) == PS_OK);
    CHECK(!memcmp(got, one, sizeof got));

    /* refusals */
    ps_phgr13_ek mono = ek;
    mono.lgsi = NULL;
    CHECK(ps_phgr13_prove_batch(ctx, &mono, qap, sols, K, got, NULL) == PS_ERR_ARG);
    CHECK(strstr(ps_last_error(), "ps_points_monomial_to_lagrange") != NULL);
    ps_scalars *shorter = NULL, *none = NULL;
    CHECK(ps_scalars_slice(sols, 0, K * M - 1, &shorter) == PS_OK && ps_scalars_slice(sols, 0, 0, &none) == PS_OK);
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, shorter, K, got, NULL) == PS_ERR_ARG);
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, none, 0, NULL, NULL) == PS_OK);

    /* the sum underneath: the three witnesses in place over vs, ws and ys */
    const ps_points* arr[3] = {crs.vs, crs.ws, crs.ys};
    static uint8_t s0[K * 96], s1[K * 192], s2[K * 96], each[192];
    uint8_t* dst[3] = {s0, s1, s2};
    CHECK(ps_points_len(crs.vs) == NN);
    CHECK(ps_msm_batch_multi(ctx, arr, 3, sols, K, M, DIFF, dst) == PS_OK);
    for (int j = 0; j < K; j++) {
        ps_scalars* part = NULL;
        CHECK(ps_scalars_slice(sols, (size_t)(M * j + DIFF), NN, &part) == PS_OK);
        CHECK(ps_msm(ctx, crs.vs, part, each) == PS_OK && !memcmp(s0 + 96 * j, each, 96));
        CHECK(ps_msm(ctx, crs.ws, part, each) == PS_OK && !memcmp(s1 + 192 * j, each, 192));
        CHECK(ps_msm(ctx, crs.ys, part, each) == PS_OK && !memcmp(s2 + 96 * j, each, 96));
        ps_scalars_free(part);
        CHECK(!memcmp(s0 + 96 * j, one[j].vss, 96) && !memcmp(s1 + 192 * j, one[j].wss, 192) && !memcmp(s2 + 96 * j, one[j].yss, 96));
    }
    CHECK(ps_msm_batch_multi(ctx, arr, 3, sols, K, M, DIFF + 1, dst) == PS_ERR_LENGTH); /* first + n > stride */
    CHECK(ps_msm_batch_multi(ctx, arr, 3, sols, K + 1, M, DIFF, dst) == PS_ERR_LENGTH); /* len(scalars) != k * stride */
    const ps_points* uneven[2] = {crs.vs, crs.vk_vs}; /* 3 and 9 points */
    CHECK(ps_msm_batch_multi(ctx, uneven, 2, sols, K, M, 0, dst) == PS_ERR_LENGTH);
    const ps_points* hole[2] = {crs.vs, NULL};
    CHECK(ps_msm_batch_multi(ctx, hole, 2, sols, K, M, DIFF, dst) == PS_ERR_ARG);
    CHECK(ps_msm_batch_multi(ctx, arr, 0, sols, K, M, DIFF, dst) == PS_OK);
    CHECK(ps_msm_batch_multi(ctx, arr, 3, none, 0, M, DIFF, dst) == PS_OK);

    ps_scalars_free(shorter); ps_scalars_free(none); ps_scalars_free(bsols); ps_scalars_free(sols);
    for (int j = 0; j < K; j++) ps_scalars_free(sol[j]);
    ps_phgr13_crs_free(&crs);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_phgr13_batch ok\n");
    return 0;
}
