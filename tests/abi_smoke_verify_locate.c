/* abi_smoke_verify_locate.c -- ps_groth16_verify_batch_locate through the C ABI: plain C99, nothing but
 * include/playsnark_hip.h.  A key for the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198), seven proofs with
 * different (r, s), and
 *   - the seven as one batch: every verdict 1, no invalid proof, one check, depth 0;
 *   - the batch with the C of proof 4 replaced by the C of proof 0: the verdicts are those of ps_groth16_verify on every
 *     proof in this program (only proof 4 invalid), at most 1 + 2 ceil(log2 7) = 7 checks, depth 3;
 *   - no proofs at all: *ninvalid = 0 and valid is not touched; a zero weight is PS_ERR_ARG with *ninvalid = 0.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_verify_locate.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_verify_locate
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_verify_locate: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}
#define NP 7
#define DIFF 3 /* nbVars - nbIO = 6 - 3 */

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
    const int64_t witness[6] = {1, 3, 35, 9, 27, 30}; /* createWitness, r1cs.go:67-76 */
    ps_qap* qap = NULL;
    ps_scalars* sol = NULL;
    CHECK(ps_qap_create(ctx, 4, 6, 3, &L, &R, &O, &qap) == PS_OK);
    CHECK(ps_scalars_upload_i64(ctx, witness, 6, &sol) == PS_OK);

    ps_groth16_toxic tw;
    be32_small(tw.alpha, 1234577ul); be32_small(tw.beta, 7654321ul); be32_small(tw.delta, 424243ul);
    be32_small(tw.x, 998877665ul); be32_small(tw.gamma, 31337ul);
    ps_groth16_crs crs;
    memset(&crs, 0, sizeof crs);
    CHECK(ps_groth16_setup(ctx, qap, &tw, &crs) == PS_OK);
    CHECK(ps_points_len(crs.io_lp) == DIFF);
    ps_groth16_pk pk;
    memset(&pk, 0, sizeof pk); /* the header requires zero-initialised structs */
    memcpy(pk.alpha, crs.alpha, 96); memcpy(pk.beta, crs.beta, 96); memcpy(pk.delta, crs.delta, 96);
    memcpy(pk.beta2, crs.beta2, 192); memcpy(pk.delta2, crs.delta2, 192);
    pk.xi = crs.xi; pk.xi2 = crs.xi2; pk.nio_lp = crs.nio_lp; pk.xi_t = crs.xi_t;
    ps_groth16_vk vk;
    memset(&vk, 0, sizeof vk);
    memcpy(vk.alpha, crs.alpha, 96); memcpy(vk.beta2, crs.beta2, 192); memcpy(vk.gamma, crs.gamma, 192); memcpy(vk.delta2, crs.delta2, 192);
    vk.io_lp = crs.io_lp;

    /* seven proofs, fresh (r, s) each */
    static uint8_t proofs[NP * 384];
    for (int i = 0; i < NP; i++) {
        uint8_t r[32], s[32];
        be32_small(r, 1000003ul * (unsigned long)(i + 1));
        be32_small(s, 777ul + 13ul * (unsigned long)i);
        CHECK(ps_groth16_prove(ctx, &pk, qap, sol, r, s, proofs + 384 * i, proofs + 384 * i + 96, proofs + 384 * i + 288) == PS_OK);
    }
    uint8_t io_be[NP * DIFF * 32], rho[NP * 32];
    for (int i = 0; i < NP; i++)
        for (int j = 0; j < DIFF; j++) be32_small(io_be + 32 * (DIFF * i + j), (unsigned long)witness[j]);
    ps_scalars *io = NULL, *io1 = NULL;
    CHECK(ps_scalars_upload(ctx, io_be, NP * DIFF, &io) == PS_OK);
    CHECK(ps_scalars_upload(ctx, io_be, DIFF, &io1) == PS_OK);
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < NP; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(37 * i + 11 * k + 5); /* 128-bit weights */

    /* a valid batch */
    uint8_t valid[NP];
    size_t ninvalid = 99;
    ps_verify_locate_info info;
    memset(valid, 7, sizeof valid);
    CHECK(ps_groth16_verify_batch_locate(ctx, &vk, io, proofs, NP, rho, valid, &ninvalid) == PS_OK && ninvalid == 0);
    for (int i = 0; i < NP; i++) CHECK(valid[i] == 1);
    CHECK(ps_groth16_verify_batch_locate_info(ctx, &info) == PS_OK && info.checks == 1 && info.levels == 0 && info.invalid == 0);

    /* a valid subgroup point in the wrong place: the C of proof 0 as the C of proof 4 */
    static uint8_t bad[NP * 384];
    memcpy(bad, proofs, sizeof bad);
    memcpy(bad + 4 * 384 + 288, proofs + 288, 96);
    int ok = -1;
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, bad, NP, rho, &ok) == PS_OK && ok == 0);
    memset(valid, 7, sizeof valid);
    CHECK(ps_groth16_verify_batch_locate(ctx, &vk, io, bad, NP, rho, valid, &ninvalid) == PS_OK && ninvalid == 1);
    for (int i = 0; i < NP; i++) {
        int single = -1;
        CHECK(ps_groth16_verify(ctx, &vk, io1, bad + 384 * i, bad + 384 * i + 96, bad + 384 * i + 288, &single) == PS_OK);
        CHECK(single == (i == 4 ? 0 : 1) && valid[i] == (uint8_t)single);
    }
    CHECK(ps_groth16_verify_batch_locate_info(ctx, &info) == PS_OK && info.invalid == 1 && info.levels == 3);
    CHECK(info.checks >= 2 && info.checks <= 1 + 2 * 3);

    /* nothing to do, and a refusal */
    ps_scalars* io_none = NULL;
    CHECK(ps_scalars_slice(io, 0, 0, &io_none) == PS_OK);
    ninvalid = 99;
    memset(valid, 7, sizeof valid);
    CHECK(ps_groth16_verify_batch_locate(ctx, &vk, io_none, NULL, 0, NULL, NULL, &ninvalid) == PS_OK && ninvalid == 0);
    uint8_t rho_bad[NP * 32];
    memcpy(rho_bad, rho, sizeof rho);
    memset(rho_bad + 32, 0, 32);
    ninvalid = 99;
    CHECK(ps_groth16_verify_batch_locate(ctx, &vk, io, bad, NP, rho_bad, valid, &ninvalid) == PS_ERR_ARG && ninvalid == 0);

    ps_scalars_free(io_none); ps_scalars_free(io1); ps_scalars_free(io);
    ps_points_free(crs.xi); ps_points_free(crs.xi2); ps_points_free(crs.io_lp); ps_points_free(crs.nio_lp); ps_points_free(crs.xi_t);
    ps_points_free(crs.lxi); ps_points_free(crs.lxi2); ps_points_free(crs.lxi_t);
    ps_scalars_free(sol);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_verify_locate ok\n");
    return 0;
}
