/* abi_smoke_kzg_lagrange.c -- a polynomial held as its VALUES on the domain 1..6, committed and opened with no interpolation,
 * through the C ABI the way a cgo caller uses it: plain C99, nothing but include/playsnark_hip.h.  The domain is a ps_qap of six
 * gates whose left matrix is the identity, so its gate values for the solution v = (3, 1, 4, 1, 5, 9) are v itself; the string
 * is held in the clear (tau = 11) and put into Lagrange form by ps_points_monomial_to_lagrange.
 *   - ps_qap_gate_values returns v; ps_qap_interpolate gives the six coefficients the other route needs;
 *   - ps_kzg_commit_lagrange == ps_kzg_commit of the coefficients; ps_poly_eval_lagrange == ps_poly_eval of them;
 *   - ps_kzg_open_lagrange at {2 (a node), 7 (off the domain)} == ps_kzg_open of the coefficients, byte for byte, one point alone
 *     as well; ps_kzg_verify accepts both openings and rejects a changed value;
 *   - ps_poly_div_linear_lagrange gives two rows of six quotient values;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_lagrange_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg_lagrange.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg_lagrange
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "abi_smoke_kzg_lagrange: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                                 \
        }                                                                                             \
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

#define N 6 /* nodes of the domain, values of p */
#define K 2 /* points */
#define TAU 11ull

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(ps_poly_lagrange_tile() >= 512 && ps_poly_lagrange_tile() % 256 == 0);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    /* the domain: six gates, six variables, left = the identity, right = out = the first variable */
    uint32_t row_ptr[N + 1], col_id[N], col_0[N];
    int64_t ones[N];
    for (int i = 0; i < N; i++) { row_ptr[i] = (uint32_t)i; col_id[i] = (uint32_t)i; col_0[i] = 0; ones[i] = 1; }
    row_ptr[N] = N;
    ps_csr L, R;
    L.row_ptr = row_ptr; L.col = col_id; L.val = ones;
    R.row_ptr = row_ptr; R.col = col_0; R.val = ones;
    ps_qap* qap = NULL;
    CHECK(ps_qap_create(ctx, N, N, 1, &L, &R, &R, &qap) == PS_OK);

    /* the string in the clear, and its Lagrange form on the nodes 1..6 */
    uint8_t pw[N * 32];
    unsigned long long t = 1;
    for (int i = 0; i < N; i++, t *= TAU) be32_small(pw + 32 * i, t);
    ps_scalars* pws = NULL;
    ps_points *tau_g1 = NULL, *lag_g1 = NULL, *tau_g2 = NULL;
    CHECK(ps_scalars_upload(ctx, pw, N, &pws) == PS_OK && ps_points_from_scalars(ctx, PS_G1, pws, &tau_g1) == PS_OK);
    ps_scalars* two = NULL;
    CHECK(ps_scalars_slice(pws, 0, 2, &two) == PS_OK && ps_points_from_scalars(ctx, PS_G2, two, &tau_g2) == PS_OK);
    CHECK(ps_points_monomial_to_lagrange(ctx, qap, tau_g1, 0, &lag_g1) == PS_OK && ps_points_len(lag_g1) == N);
    uint8_t t2[2 * 192];
    CHECK(ps_points_download(ctx, tau_g2, 0, 2, t2) == PS_OK);

    const unsigned long long v[N] = {3, 1, 4, 1, 5, 9}, zs[K] = {2, 7};
    uint8_t v_be[N * 32], z_be[K * 32], got[N * 32];
    for (int i = 0; i < N; i++) be32_small(v_be + 32 * i, v[i]);
    for (int j = 0; j < K; j++) be32_small(z_be + 32 * j, zs[j]);
    ps_scalars *sol = NULL, *values = NULL, *coeffs = NULL;
    CHECK(ps_scalars_upload(ctx, v_be, N, &sol) == PS_OK);
    CHECK(ps_qap_gate_values(ctx, qap, sol, 0, &values) == PS_OK && ps_scalars_len(values) == N);
    CHECK(ps_scalars_download(ctx, values, 0, N, got) == PS_OK && memcmp(got, v_be, sizeof got) == 0);
    CHECK(ps_qap_interpolate(ctx, qap, sol, 0, &coeffs) == PS_OK && ps_scalars_len(coeffs) == N);

    /* commitment and values: the bytes of the coefficient route */
    uint8_t commit[96], commit_c[96], y[K * 32], y_c[K * 32], want[32];
    CHECK(ps_kzg_commit_lagrange(ctx, lag_g1, values, commit) == PS_OK && ps_kzg_commit(ctx, tau_g1, coeffs, commit_c) == PS_OK);
    CHECK(memcmp(commit, commit_c, 96) == 0);
    CHECK(ps_poly_eval_lagrange(ctx, qap, values, z_be, K, y) == PS_OK && ps_poly_eval(ctx, coeffs, z_be, K, y_c) == PS_OK);
    CHECK(memcmp(y, y_c, sizeof y) == 0);
    be32_small(want, v[zs[0] - 1]); /* at a node the value is the node's */
    CHECK(memcmp(y, want, 32) == 0);

    /* the openings: on the domain and off it in one call */
    uint8_t y2[K * 32], proofs[K * 96], proofs_c[K * 96], one_y[32], one_pi[96];
    CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, z_be, K, y2, proofs) == PS_OK);
    CHECK(ps_kzg_open(ctx, tau_g1, coeffs, z_be, K, y_c, proofs_c) == PS_OK);
    CHECK(memcmp(y2, y, sizeof y) == 0 && memcmp(proofs, proofs_c, sizeof proofs) == 0);
    for (int j = 0; j < K; j++) {
        int ok = -1;
        CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, z_be + 32 * j, 1, one_y, one_pi) == PS_OK);
        CHECK(memcmp(one_y, y + 32 * j, 32) == 0 && memcmp(one_pi, proofs + 96 * j, 96) == 0);
        CHECK(ps_kzg_verify(t2 + 192, commit, z_be + 32 * j, y + 32 * j, proofs + 96 * j, &ok) == PS_OK && ok == 1);
        memcpy(want, y + 32 * j, 32);
        want[31] ^= 1;
        CHECK(ps_kzg_verify(t2 + 192, commit, z_be + 32 * j, want, proofs + 96 * j, &ok) == PS_OK && ok == 0);
    }

    /* the quotient rows */
    ps_scalars* qv = NULL;
    uint8_t qv_be[K * N * 32];
    CHECK(ps_poly_div_linear_lagrange(ctx, qap, values, z_be, K, &qv, y2) == PS_OK && ps_scalars_len(qv) == K * N);
    CHECK(memcmp(y2, y, sizeof y) == 0 && ps_scalars_download(ctx, qv, 0, K * N, qv_be) == PS_OK);

    /* argument checks: lengths, the group, a point that is not below r, no point at all */
    ps_scalars* fewer = NULL;
    ps_points* shorter = NULL;
    uint8_t big[K * 32], keep[K * 96];
    memset(big, 0xff, sizeof big);
    CHECK(ps_scalars_slice(values, 0, N - 1, &fewer) == PS_OK && ps_points_slice(lag_g1, 0, N - 1, &shorter) == PS_OK);
    CHECK(ps_poly_eval_lagrange(ctx, qap, fewer, z_be, K, y2) == PS_ERR_LENGTH);
    CHECK(ps_kzg_commit_lagrange(ctx, lag_g1, fewer, commit_c) == PS_ERR_LENGTH);
    CHECK(ps_kzg_open_lagrange(ctx, qap, shorter, values, z_be, K, y2, proofs_c) == PS_ERR_LENGTH);
    CHECK(strstr(ps_last_error(), "ps_kzg_open_lagrange") != NULL);
    CHECK(ps_kzg_commit_lagrange(ctx, tau_g2, values, commit_c) == PS_ERR_ARG);
    CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, big, K, y2, proofs_c) == PS_ERR_ENCODING);
    CHECK(ps_kzg_open_lagrange(ctx, NULL, lag_g1, values, z_be, K, y2, proofs_c) == PS_ERR_ARG);
    memcpy(keep, proofs, sizeof keep);
    CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, z_be, 0, y2, proofs) == PS_OK && memcmp(keep, proofs, sizeof keep) == 0);
    CHECK(ps_qap_gate_values(ctx, qap, sol, 3, &fewer) == PS_ERR_ARG);

    print_hex("commit", commit, sizeof commit);
    print_hex("y", y, sizeof y);
    print_hex("proofs", proofs, sizeof proofs);
    print_hex("qv", qv_be, sizeof qv_be);

    ps_scalars_free(fewer);
    ps_points_free(shorter);
    ps_scalars_free(qv);
    ps_scalars_free(coeffs);
    ps_scalars_free(values);
    ps_scalars_free(sol);
    ps_scalars_free(two);
    ps_scalars_free(pws);
    ps_points_free(lag_g1);
    ps_points_free(tau_g1);
    ps_points_free(tau_g2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg_lagrange ok\n");
    return 0;
}
