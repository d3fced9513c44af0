/* abi_smoke_verify_batch.c -- ps_groth16_verify_batch through the C ABI, the way a cgo caller uses it: plain C99, nothing
 * but include/playsnark_hip.h.  Sets up a key for the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198, witness
 * r1cs.go:67-76) with caller-drawn toxic waste, proves it three times with different (r, s), and checks
 *   - the three proofs as ONE batch (proofs as 3 x (A 96 B || B 192 B || C 96 B), io as 3 x diff scalars proof-major,
 *     rho as 3 x 32 B big-endian): accepted;
 *   - each proof alone with rho = 1 against ps_groth16_verify: the same verdict;
 *   - the batch with the C of the middle proof replaced by the C of the first: rejected;
 *   - the batch with a wrong public input of the last proof: rejected;
 *   - rho = 0 is PS_ERR_ARG, rho = r is PS_ERR_ENCODING, an io vector one short is PS_ERR_LENGTH, no proofs at all is 1;
 *   - ps_pairing_product_is_one on e(2 G1, 3 G2) e(-6 G1, G2) (one) and on e(2 G1, 3 G2) e(-5 G1, G2) (not one).
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_verify_batch.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_verify_batch
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_verify_batch: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

static void be32_small(uint8_t out[32], unsigned long v) {
    memset(out, 0, 32);
    for (int i = 0; i < 8; i++) out[31 - i] = (uint8_t)(v >> (8 * i));
}
/* r - k for a small k: the scalar -k (r = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001) */
static void be32_neg_small(uint8_t out[32], unsigned k) {
    static const uint8_t r[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8, 0x08, 0x09, 0xa1, 0xd8, 0x05,
                                  0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
    memcpy(out, r, 32);
    unsigned borrow = k;
    for (int i = 31; i >= 0 && borrow; i--) {
        unsigned b = borrow & 0xff;
        borrow >>= 8;
        if (out[i] >= b) out[i] = (uint8_t)(out[i] - b);
        else { out[i] = (uint8_t)(out[i] + 256 - b); borrow += 1; }
    }
}

#define NP 3
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

    /* three proofs, fresh (r, s) each */
    static uint8_t proofs[NP * 384];
    for (int i = 0; i < NP; i++) {
        uint8_t r[32], s[32];
        be32_small(r, 1000003ul * (unsigned long)(i + 1));
        be32_small(s, 777ul + 13ul * (unsigned long)i);
        CHECK(ps_groth16_prove(ctx, &pk, qap, sol, r, s, proofs + 384 * i, proofs + 384 * i + 96, proofs + 384 * i + 288) == PS_OK);
    }
    CHECK(memcmp(proofs, proofs + 384, 384) != 0);

    /* io = sol[:diff] of every proof, proof-major */
    uint8_t io_be[NP * DIFF * 32], rho[NP * 32];
    for (int i = 0; i < NP; i++)
        for (int j = 0; j < DIFF; j++) be32_small(io_be + 32 * (DIFF * i + j), (unsigned long)witness[j]);
    ps_scalars *io = NULL, *io1 = NULL;
    CHECK(ps_scalars_upload(ctx, io_be, NP * DIFF, &io) == PS_OK);
    CHECK(ps_scalars_upload(ctx, io_be, DIFF, &io1) == PS_OK);
    memset(rho, 0, sizeof rho);
    for (int i = 0; i < NP; i++)
        for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(37 * i + 11 * k + 5); /* 128-bit weights */

    int ok = -1;
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, proofs, NP, rho, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, proofs, NP, rho, &ok) == PS_OK && ok == 1); /* again, warm */
    uint8_t one[32];
    be32_small(one, 1);
    for (int i = 0; i < NP; i++) {
        int single = -1;
        CHECK(ps_groth16_verify(ctx, &vk, io1, proofs + 384 * i, proofs + 384 * i + 96, proofs + 384 * i + 288, &single) == PS_OK && single == 1);
        CHECK(ps_groth16_verify_batch(ctx, &vk, io1, proofs + 384 * i, 1, one, &ok) == PS_OK && ok == single);
    }

    /* a valid subgroup point in the wrong place: the C of proof 0 as the C of proof 1 */
    static uint8_t bad[NP * 384];
    memcpy(bad, proofs, sizeof bad);
    memcpy(bad + 384 + 288, proofs + 288, 96);
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, bad, NP, rho, &ok) == PS_OK && ok == 0);
    {
        int single = -1;
        CHECK(ps_groth16_verify(ctx, &vk, io1, bad + 384, bad + 384 + 96, bad + 384 + 288, &single) == PS_OK && single == 0);
        CHECK(ps_groth16_verify_batch(ctx, &vk, io1, bad + 384, 1, one, &ok) == PS_OK && ok == 0);
    }
    /* a wrong public input of the last proof */
    uint8_t io_bad[NP * DIFF * 32];
    memcpy(io_bad, io_be, sizeof io_bad);
    io_bad[32 * (DIFF * 2 + 1) + 31] ^= 1;
    ps_scalars* iob = NULL;
    CHECK(ps_scalars_upload(ctx, io_bad, NP * DIFF, &iob) == PS_OK);
    CHECK(ps_groth16_verify_batch(ctx, &vk, iob, proofs, NP, rho, &ok) == PS_OK && ok == 0);

    /* refusals */
    uint8_t rho_bad[NP * 32];
    memcpy(rho_bad, rho, sizeof rho);
    memset(rho_bad + 32, 0, 32);
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, proofs, NP, rho_bad, &ok) == PS_ERR_ARG);
    be32_neg_small(rho_bad + 32, 0); /* r itself */
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, proofs, NP, rho_bad, &ok) == PS_ERR_ENCODING);
    ps_scalars* io_short = NULL;
    CHECK(ps_scalars_slice(io, 0, NP * DIFF - 1, &io_short) == PS_OK);
    CHECK(ps_groth16_verify_batch(ctx, &vk, io_short, proofs, NP, rho, &ok) == PS_ERR_LENGTH);
    ps_scalars* io_none = NULL;
    CHECK(ps_scalars_slice(io, 0, 0, &io_none) == PS_OK);
    ok = -1;
    CHECK(ps_groth16_verify_batch(ctx, &vk, io_none, NULL, 0, NULL, &ok) == PS_OK && ok == 1);
    CHECK(ps_groth16_verify_batch(ctx, &vk, io, proofs, NP, rho, &ok) == PS_OK && ok == 1);

    /* the product of pairings underneath */
    uint8_t k1[2 * 32], k2[2 * 32];
    ps_scalars *s1 = NULL, *s2 = NULL;
    ps_points *g1 = NULL, *g2 = NULL;
    for (unsigned miss = 0; miss < 2; miss++) {
        be32_small(k1, 2); be32_neg_small(k1 + 32, 6 - miss);
        be32_small(k2, 3); be32_small(k2 + 32, 1);
        CHECK(ps_scalars_upload(ctx, k1, 2, &s1) == PS_OK && ps_scalars_upload(ctx, k2, 2, &s2) == PS_OK);
        CHECK(ps_points_from_scalars(ctx, PS_G1, s1, &g1) == PS_OK && ps_points_from_scalars(ctx, PS_G2, s2, &g2) == PS_OK);
        int is_one = -1;
        CHECK(ps_pairing_product_is_one(ctx, g1, g2, 1, &is_one) == PS_OK && is_one == (miss ? 0 : 1));
        ps_points_free(g1); ps_points_free(g2); ps_scalars_free(s1); ps_scalars_free(s2);
    }

    ps_scalars_free(io_none); ps_scalars_free(io_short); ps_scalars_free(iob); ps_scalars_free(io1); ps_scalars_free(io);
    ps_points_free(crs.xi); ps_points_free(crs.xi2); ps_points_free(crs.io_lp); ps_points_free(crs.nio_lp); ps_points_free(crs.xi_t);
    ps_points_free(crs.lxi); ps_points_free(crs.lxi2); ps_points_free(crs.lxi_t);
    ps_scalars_free(sol);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_verify_batch ok\n");
    return 0;
}
