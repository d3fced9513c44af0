/* abi_smoke_phgr13_verify_locate.c -- ps_phgr13_verify_batch_locate and ps_phgr13_verify_batch_locate_info through the C ABI,
 * the way a cgo caller uses them: plain C99, nothing but include/playsnark_hip.h.  The circuit is that of
 * tests/abi_smoke_phgr13_verify_batch.c (7 gates, 9 variables, diff = 6); seven witnesses from x = 3, 5, .., 15, proved in one
 * ps_phgr13_prove_batch.  Checks
 *   - the seven proofs as one batch: nothing invalid, checks 1, products 5, levels 0;
 *   - the batch with the vass of proof 4 replaced by the vass of proof 0: exactly proof 4 is reported, with the mask {E1},
 *     levels = 3, checks <= 1 + 2 * 3, products <= 5 + 2 * 3; ps_phgr13_verify on every proof gives the same verdicts;
 *     ps_phgr13_verify_batch_info reports the batch's mask; `failed` may be NULL;
 *   - a wrong public input of proof 6 (the carried node): proof 6 with the mask {E0};
 *   - rho = 0 is PS_ERR_ARG and leaves *ninvalid = 0; no proofs: *ninvalid = 0.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_phgr13_verify_locate.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_phgr13_verify_locate
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_phgr13_verify_locate: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}

#define K 7
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
    CHECK(sizeof(ps_phgr13_proof) == 864 && sizeof(ps_phgr13_locate_info) == 32);
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

    /* io = sol[:diff] of every proof, proof-major; 128-bit weights */
    static uint8_t io_be[K * DIFF * 32], rho[K * 32];
    for (int i = 0; i < K; i++)
        for (int j = 0; j < DIFF; j++) be32_small(io_be + 32 * (DIFF * i + j), (unsigned long)wit[M * i + j]);
    ps_scalars *io = NULL, *io_each[K];
    CHECK(ps_scalars_upload(ctx, io_be, K * DIFF, &io) == PS_OK);
    for (int i = 0; i < K; i++) {
        io_each[i] = NULL;
        CHECK(ps_scalars_slice(io, (size_t)(DIFF * i), DIFF, &io_each[i]) == PS_OK);
    }
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < K; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(37 * i + 11 * k + 5);

    uint8_t valid[K], failed[K];
    size_t ninvalid = 99;
    ps_phgr13_locate_info info;
    ps_phgr13_batch_info binfo;
    memset(&info, 0xee, sizeof info);
    memset(valid, 0xee, sizeof valid);
    memset(failed, 0xee, sizeof failed);
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io, proofs, K, rho, valid, failed, &ninvalid) == PS_OK && ninvalid == 0);
    for (int i = 0; i < K; i++) CHECK(valid[i] == 1 && failed[i] == 0);
    CHECK(ps_phgr13_verify_batch_locate_info(ctx, &info) == PS_OK);
    CHECK(info.checks == 1 && info.products == 5 && info.levels == 0 && info.invalid == 0 && info.failed == 0);

    /* a valid subgroup point in the wrong place: the vass of proof 0 as the vass of proof 4 */
    static ps_phgr13_proof bad[K];
    memcpy(bad, proofs, sizeof bad);
    memcpy(bad[4].vass, proofs[0].vass, 96);
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io, bad, K, rho, valid, failed, &ninvalid) == PS_OK && ninvalid == 1);
    for (int i = 0; i < K; i++) {
        int single = -1;
        CHECK(ps_phgr13_verify(ctx, &vk, io_each[i], &bad[i], &single) == PS_OK);
        CHECK(single == (i != 4) && valid[i] == (uint8_t)single && failed[i] == (i == 4 ? 1u << 1 : 0u));
    }
    CHECK(ps_phgr13_verify_batch_locate_info(ctx, &info) == PS_OK);
    CHECK(info.levels == 3 && info.invalid == 1 && info.failed == (1u << 1));
    CHECK(info.checks >= 2 && info.checks <= 1 + 2 * 3 && info.products >= 6 && info.products <= 5 + 2 * 3);
    CHECK(ps_phgr13_verify_batch_info(ctx, &binfo) == PS_OK && binfo.failed == (1u << 1) && binfo.device_loops == K + DIFF);
    memset(valid, 0xee, sizeof valid);
    ninvalid = 99;
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io, bad, K, rho, valid, NULL, &ninvalid) == PS_OK && ninvalid == 1);
    for (int i = 0; i < K; i++) CHECK(valid[i] == (i != 4));

    /* a wrong public input of the last proof, whose leaf is carried up two levels */
    static uint8_t io_bad[K * DIFF * 32];
    memcpy(io_bad, io_be, sizeof io_bad);
    io_bad[32 * (DIFF * 6 + 1) + 31] ^= 1;
    ps_scalars* iob = NULL;
    CHECK(ps_scalars_upload(ctx, io_bad, K * DIFF, &iob) == PS_OK);
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, iob, proofs, K, rho, valid, failed, &ninvalid) == PS_OK && ninvalid == 1);
    for (int i = 0; i < K; i++) CHECK(valid[i] == (i != 6) && failed[i] == (i == 6 ? 1u : 0u));
    CHECK(ps_phgr13_verify_batch_locate_info(ctx, &info) == PS_OK && info.levels == 3 && info.failed == 1u && info.checks <= 1 + 2 * 3);

    /* refusals */
    static uint8_t rho_bad[K * 32];
    memcpy(rho_bad, rho, sizeof rho);
    memset(rho_bad + 32, 0, 32);
    ninvalid = 99;
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io, proofs, K, rho_bad, valid, failed, &ninvalid) == PS_ERR_ARG && ninvalid == 0);
    ps_scalars* io_none = NULL;
    CHECK(ps_scalars_slice(io, 0, 0, &io_none) == PS_OK);
    ninvalid = 99;
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io_none, NULL, 0, NULL, NULL, NULL, &ninvalid) == PS_OK && ninvalid == 0);
    CHECK(ps_phgr13_verify_batch_locate(ctx, &vk, io, proofs, K, rho, valid, failed, &ninvalid) == PS_OK && ninvalid == 0);

    ps_scalars_free(io_none); ps_scalars_free(iob);
    for (int i = 0; i < K; i++) ps_scalars_free(io_each[i]);
    ps_scalars_free(io); ps_scalars_free(sols);
    ps_points_free(vs_io); ps_points_free(ws_io); ps_points_free(ys_io);
    ps_phgr13_crs_free(&crs);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_phgr13_verify_locate ok\n");
    return 0;
}
