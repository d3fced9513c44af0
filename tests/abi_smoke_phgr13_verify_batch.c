/* abi_smoke_phgr13_verify_batch.c -- ps_phgr13_verify_batch and ps_phgr13_verify_batch_info through the C ABI, the way a
 * cgo caller uses them: plain C99, nothing but include/playsnark_hip.h.  The circuit is the reference's toy gate pattern
 * (Mul, Mul, Add, AddConst; r1cs.go:178-198) tiled to 7 gates, 9 variables [const, x, out, u, v, w, x', u', v'], nbIO = 3,
 * diff = 6; two witnesses from x = 3, 5, proved in one ps_phgr13_prove_batch.  Checks
 *   - the two proofs as ONE batch (io as 2 x diff scalars proof-major, rho as 2 x 32 B big-endian): accepted, failed = 0,
 *     device_loops = 2 + diff;
 *   - each proof alone with rho = 1 against ps_phgr13_verify: the same verdict;
 *   - the batch with the vass of proof 1 replaced by the vass of proof 0: rejected, failed = {E1};
 *   - the batch with a wrong public input of proof 1: rejected, failed = {E0};
 *   - rho = 0 is PS_ERR_ARG, an io vector one short is PS_ERR_LENGTH, more than 2^20 proofs is PS_ERR_ARG, no proofs is 1.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_phgr13_verify_batch.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_phgr13_verify_batch
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_phgr13_verify_batch: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define K 2
#define N 7
#define M 9
#define NIO 3
#define DIFF (M - NIO) /* pinochio.go:219 */

static void witness(int64_t w[M], int64_t x) {
    const int64_t u = x * x, v = u * x, ww = v + x, x2 = ww + 5, u2 = x2 * x2, v2 = u2 * x2;
    w[0] = 1; w[1] = x; w[2] = v2 + x2; w[3] = u; w[4] = v; w[5] = ww; w[6] = x2; w[7] = u2; w[8] = v2;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(sizeof(ps_phgr13_proof) == 864 && sizeof(ps_phgr13_batch_info) == 16);
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
    ps_scalars* sols = NULL;
    CHECK(ps_scalars_upload_i64(ctx, wit, K * M, &sols) == PS_OK);

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
    static ps_phgr13_proof proofs[K];
    CHECK(ps_phgr13_prove_batch(ctx, &ek, qap, sols, K, proofs, NULL) == PS_OK);

    /* the verifier's key: the fixed points and the first diff points of vk.vs, vk.ws, vk.ys */
    ps_phgr13_vk vk;
    memset(&vk, 0, sizeof vk);
    memcpy(vk.av, crs.av, 192); memcpy(vk.aw, crs.aw, 96); memcpy(vk.ay, crs.ay, 192); memcpy(vk.gamma, crs.gamma, 192);
    memcpy(vk.bgamma, crs.bgamma, 96); memcpy(vk.bgamma2, crs.bgamma2, 192); memcpy(vk.yts, crs.yts, 192);
    ps_points *vs_io = NULL, *ws_io = NULL, *ys_io = NULL;
    CHECK(ps_points_slice(crs.vk_vs, 0, DIFF, &vs_io) == PS_OK && ps_points_slice(crs.vk_ws, 0, DIFF, &ws_io) == PS_OK &&
          ps_points_slice(crs.vk_ys, 0, DIFF, &ys_io) == PS_OK);
    vk.vs_io = vs_io; vk.ws_io = ws_io; vk.ys_io = ys_io;

    /* io = sol[:diff] of every proof, proof-major */
    uint8_t io_be[K * DIFF * 32], rho[K * 32], one[32];
    for (int i = 0; i < K; i++)
        for (int j = 0; j < DIFF; j++) be32_small(io_be + 32 * (DIFF * i + j), (unsigned long)wit[M * i + j]);
    ps_scalars *io = NULL, *io_each[K] = {NULL, NULL};
    CHECK(ps_scalars_upload(ctx, io_be, K * DIFF, &io) == PS_OK);
    for (int i = 0; i < K; i++) CHECK(ps_scalars_slice(io, (size_t)(DIFF * i), DIFF, &io_each[i]) == PS_OK);
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < K; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(37 * i + 11 * k + 5); /* 128-bit weights */
    be32_small(one, 1);

    int ok = -1;
    ps_phgr13_batch_info info;
    memset(&info, 0xee, sizeof info);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io, proofs, K, rho, &ok) == PS_OK && ok == 1);
    CHECK(ps_phgr13_verify_batch_info(ctx, &info) == PS_OK && info.failed == 0 && info.device_loops == K + DIFF);
    for (int i = 0; i < K; i++) {
        int single = -1;
        CHECK(ps_phgr13_verify(ctx, &vk, io_each[i], &proofs[i], &single) == PS_OK && single == 1);
        CHECK(ps_phgr13_verify_batch(ctx, &vk, io_each[i], &proofs[i], 1, one, &ok) == PS_OK && ok == single);
    }

    /* a valid subgroup point in the wrong place: the vass of proof 0 as the vass of proof 1 */
    static ps_phgr13_proof bad[K];
    memcpy(bad, proofs, sizeof bad);
    memcpy(bad[1].vass, proofs[0].vass, 96);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io, bad, K, rho, &ok) == PS_OK && ok == 0);
    CHECK(ps_phgr13_verify_batch_info(ctx, &info) == PS_OK && info.failed == (1u << 1) && info.device_loops == K + DIFF);
    {
        int single = -1;
        CHECK(ps_phgr13_verify(ctx, &vk, io_each[1], &bad[1], &single) == PS_OK && single == 0);
    }
    /* a wrong public input of proof 1 */
    uint8_t io_bad[K * DIFF * 32];
    memcpy(io_bad, io_be, sizeof io_bad);
    io_bad[32 * (DIFF * 1 + 1) + 31] ^= 1;
    ps_scalars* iob = NULL;
    CHECK(ps_scalars_upload(ctx, io_bad, K * DIFF, &iob) == PS_OK);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, iob, proofs, K, rho, &ok) == PS_OK && ok == 0);
    CHECK(ps_phgr13_verify_batch_info(ctx, &info) == PS_OK && info.failed == 1u);

    /* refusals */
    uint8_t rho_bad[K * 32];
    memcpy(rho_bad, rho, sizeof rho);
    memset(rho_bad + 32, 0, 32);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io, proofs, K, rho_bad, &ok) == PS_ERR_ARG && ok == 0);
    ps_scalars *io_short = NULL, *io_none = NULL;
    CHECK(ps_scalars_slice(io, 0, K * DIFF - 1, &io_short) == PS_OK && ps_scalars_slice(io, 0, 0, &io_none) == PS_OK);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io_short, proofs, K, rho, &ok) == PS_ERR_LENGTH);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io, proofs, ((size_t)1 << 20) + 1, rho, &ok) == PS_ERR_ARG);
    CHECK(strstr(ps_last_error(), "split") != NULL);
    ok = -1;
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io_none, NULL, 0, NULL, &ok) == PS_OK && ok == 1);
    CHECK(ps_phgr13_verify_batch(ctx, &vk, io, proofs, K, rho, &ok) == PS_OK && ok == 1);

    ps_scalars_free(io_none); ps_scalars_free(io_short); ps_scalars_free(iob);
    for (int i = 0; i < K; i++) ps_scalars_free(io_each[i]);
    ps_scalars_free(io); ps_scalars_free(sols);
    ps_points_free(vs_io); ps_points_free(ws_io); ps_points_free(ys_io);
    ps_phgr13_crs_free(&crs);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_phgr13_verify_batch ok\n");
    return 0;
}
