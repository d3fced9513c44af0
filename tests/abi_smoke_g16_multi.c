/* abi_smoke_g16_multi.c -- Groth16Prove (groth16.go:122-211) over rank-local Lagrange-form keys through the C ABI, the way a
 * cgo caller uses it: plain C99, no Python.  Makes a key of the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198,
 * witness r1cs.go:67-76) on the device, proves with ps_groth16_prove over the whole key, then
 *   - ps_groth16_prove_multi with two contexts, each holding only its index ranges of lxi / lxi2 / lxi_t / NioLP (the monomial
 *     members of the key NULL);
 *   - ps_groth16_prove_local for ranks 0 and 1 of 2 over the same local keys, the two parts added with ps_points_sum;
 *   - refusals: a device that does not hold its range (PS_ERR_LENGTH, naming it), lxi on one device only and a context used
 *     twice (PS_ERR_ARG).
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_g16_multi.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_g16_multi
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_g16_multi: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

/* points [first, first + cnt) of `src` as an array of its own on `ctx` */
static int local_part(ps_ctx* from, ps_ctx* ctx, const ps_points* src, size_t first, size_t cnt, ps_points** out) {
    const int group = ps_points_group(src);
    const size_t pb = group == PS_G2 ? 192 : 96;
    uint8_t* raw = (uint8_t*)malloc(pb * (cnt ? cnt : 1));
    int rc = ps_points_download(from, src, first, cnt, raw);
    if (rc == PS_OK) rc = ps_points_upload(ctx, group, raw, cnt, PS_FMT_AFFINE, out);
    free(raw);
    return rc;
}

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    ps_ctx* ctxs[2] = {NULL, NULL};
    int rc = ps_ctx_create(0, &ctxs[0]);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);
    CHECK(ps_ctx_create(0, &ctxs[1]) == PS_OK);

    /* the toy R1CS, rows = gates, columns = [const, x, out, u, v, w] (r1cs.go:178-198): n = 4 gates, nbIO = 3 */
    const uint32_t l_ptr[5] = {0, 1, 2, 4, 6}, l_col[6] = {1, 3, 1, 4, 0, 5};
    const int64_t l_val[6] = {1, 1, 1, 1, 5, 1};
    const uint32_t r_ptr[5] = {0, 1, 2, 3, 4}, r_col[4] = {1, 1, 0, 0};
    const int64_t r_val[4] = {1, 1, 1, 1};
    const uint32_t o_ptr[5] = {0, 1, 2, 3, 4}, o_col[4] = {3, 4, 5, 2};
    const int64_t o_val[4] = {1, 1, 1, 1};
    const ps_csr L = {l_ptr, l_col, l_val}, R = {r_ptr, r_col, r_val}, O = {o_ptr, o_col, o_val};
    const int64_t witness[6] = {1, 3, 35, 9, 27, 30}; /* createWitness, r1cs.go:67-76 */
    ps_qap* qap[2] = {NULL, NULL};
    ps_scalars* sol[2] = {NULL, NULL};
    for (int d = 0; d < 2; d++) {
        CHECK(ps_qap_create(ctxs[d], 4, 6, 3, &L, &R, &O, &qap[d]) == PS_OK);
        CHECK(ps_scalars_upload_i64(ctxs[d], witness, 6, &sol[d]) == PS_OK);
    }

    ps_groth16_toxic tw;
    memset(&tw, 0, sizeof tw);
    tw.alpha[31] = 11; tw.beta[31] = 13; tw.delta[31] = 17; tw.x[30] = 1; tw.x[31] = 19; tw.gamma[31] = 23;
    ps_groth16_crs crs;
    CHECK(ps_groth16_setup(ctxs[0], qap[0], &tw, &crs) == PS_OK);
    uint8_t r_be[32] = {0}, s_be[32] = {0};
    r_be[31] = 29; r_be[0] = 1; s_be[31] = 31; s_be[1] = 7;

    ps_groth16_pk whole;
    memset(&whole, 0, sizeof whole); /* the header requires zero-initialised structs */
    memcpy(whole.alpha, crs.alpha, 96); memcpy(whole.beta, crs.beta, 96); memcpy(whole.delta, crs.delta, 96);
    memcpy(whole.beta2, crs.beta2, 192); memcpy(whole.delta2, crs.delta2, 192);
    whole.xi = crs.xi; whole.xi2 = crs.xi2; whole.nio_lp = crs.nio_lp; whole.xi_t = crs.xi_t;
    whole.lxi = crs.lxi; whole.lxi2 = crs.lxi2; whole.lxi_t = crs.lxi_t;
    uint8_t A[96], B[192], C[96], gA[96], gB[192], gC[96];
    CHECK(ps_groth16_prove(ctxs[0], &whole, qap[0], sol[0], r_be, s_be, A, B, C) == PS_OK);

    /* n = 4: lxi, lxi2 -> [0, 2) | [2, 4);  n - 1 = 3 and nbIO = 3: lxi_t, NioLP -> [0, 2) | [2, 3) */
    ps_groth16_device dev[2];
    memset(dev, 0, sizeof dev);
    ps_points* part[2][4];
    for (int d = 0; d < 2; d++) {
        CHECK(local_part(ctxs[0], ctxs[d], crs.lxi, d ? 2 : 0, 2, &part[d][0]) == PS_OK);
        CHECK(local_part(ctxs[0], ctxs[d], crs.lxi2, d ? 2 : 0, 2, &part[d][1]) == PS_OK);
        CHECK(local_part(ctxs[0], ctxs[d], crs.lxi_t, d ? 2 : 0, d ? 1 : 2, &part[d][2]) == PS_OK);
        CHECK(local_part(ctxs[0], ctxs[d], crs.nio_lp, d ? 2 : 0, d ? 1 : 2, &part[d][3]) == PS_OK);
        dev[d].ctx = ctxs[d];
        dev[d].qap = qap[d];
        dev[d].sol = sol[d];
        dev[d].pk = whole;
        dev[d].pk.xi = dev[d].pk.xi2 = dev[d].pk.xi_t = NULL; /* Lagrange-only */
        dev[d].pk.lxi = part[d][0]; dev[d].pk.lxi2 = part[d][1]; dev[d].pk.lxi_t = part[d][2]; dev[d].pk.nio_lp = part[d][3];
    }
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_OK);
    CHECK(!memcmp(A, gA, 96) && !memcmp(B, gB, 192) && !memcmp(C, gC, 96));
    memset(gA, 0, 96);
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_OK); /* again, on warm contexts */
    CHECK(!memcmp(A, gA, 96) && !memcmp(B, gB, 192) && !memcmp(C, gC, 96));

    /* the one-process-per-GPU form over the same local keys: two parts, added element by element */
    uint8_t pa[2 * 96], pb[2 * 192], pc[2 * 96];
    for (int d = 0; d < 2; d++)
        CHECK(ps_groth16_prove_local(ctxs[d], &dev[d].pk, qap[d], sol[d], r_be, s_be, d, 2, pa + 96 * d, pb + 192 * d, pc + 96 * d) == PS_OK);
    CHECK(ps_points_sum(PS_G1, pa, 2, gA) == PS_OK && ps_points_sum(PS_G2, pb, 2, gB) == PS_OK && ps_points_sum(PS_G1, pc, 2, gC) == PS_OK);
    CHECK(!memcmp(A, gA, 96) && !memcmp(B, gB, 192) && !memcmp(C, gC, 96));
    CHECK(ps_groth16_prove_local(ctxs[0], &dev[0].pk, qap[0], sol[0], r_be, s_be, 2, 2, gA, gB, gC) == PS_ERR_ARG);
    CHECK(ps_groth16_prove_local(ctxs[0], &dev[0].pk, qap[0], sol[0], r_be, s_be, 1, 2, gA, gB, gC) == PS_ERR_LENGTH);

    /* refusals of the multi entry */
    dev[1].pk.lxi_t = part[0][2]; /* 2 points where device 1 must hold 1 */
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_ERR_LENGTH);
    CHECK(strstr(ps_last_error(), "device 1") != NULL);
    dev[1].pk.lxi_t = part[1][2];
    dev[1].pk.lxi = NULL; /* the Lagrange form on one device only */
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_ERR_ARG);
    dev[1].pk.lxi = part[1][0];
    dev[1].ctx = ctxs[0]; /* a context used twice */
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_ERR_ARG);
    dev[1].ctx = ctxs[1];
    CHECK(ps_groth16_prove_multi(dev, 2, r_be, s_be, gA, gB, gC) == PS_OK);
    CHECK(!memcmp(A, gA, 96) && !memcmp(B, gB, 192) && !memcmp(C, gC, 96));

    for (int d = 0; d < 2; d++)
        for (int k = 0; k < 4; k++) ps_points_free(part[d][k]);
    ps_points_free(crs.xi); ps_points_free(crs.xi2); ps_points_free(crs.io_lp); ps_points_free(crs.nio_lp); ps_points_free(crs.xi_t);
    ps_points_free(crs.lxi); ps_points_free(crs.lxi2); ps_points_free(crs.lxi_t);
    for (int d = 0; d < 2; d++) {
        ps_scalars_free(sol[d]);
        ps_qap_free(qap[d]);
        ps_ctx_destroy(ctxs[d]);
    }
    printf("abi_smoke_g16_multi ok: the toy Groth16 proof of ps_groth16_prove through ps_groth16_prove_multi (two contexts over "
           "Lagrange-only rank-local keys) and through two ps_groth16_prove_local parts folded; bad ranges, mixed key forms and a "
           "context used twice are refused\n");
    return 0;
}
