/* abi_smoke_kzg_set_lagrange.c -- ONE proof for a set of points of a polynomial held as its VALUES on the domain 1..5, through
 * the C ABI the way a cgo caller uses it: plain C99, nothing but include/playsnark_hip.h.  The domain is a ps_qap of five gates
 * whose left matrix is the identity, so its gate values for the solution v = (3, 1, 4, 1, 5) are v itself; the string is held in
 * the clear (tau = 11) and put into Lagrange form by ps_points_monomial_to_lagrange.  The set is {7, 2 (a node), 9}.
 *   - ps_kzg_open_set_lagrange == ps_kzg_open_set of ps_qap_interpolate's coefficients, values and proof, byte for byte;
 *   - ps_kzg_verify_set accepts the opening against ps_kzg_commit_lagrange's commitment and rejects a changed value;
 *   - ps_poly_div_roots_lagrange gives the values and the remainder of ps_poly_div_roots, and five quotient values whose lone sum
 *     over the Lagrange-form string is the proof;
 *   - one point alone opens as ps_kzg_open_lagrange does; five points and more give the identity and a row of zeros;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_set_lagrange_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg_set_lagrange.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg_set_lagrange
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "abi_smoke_kzg_set_lagrange: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
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

#define N 5 /* nodes of the domain, values of p */
#define K 3 /* points of the set */
#define TAU 11ull

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(ps_poly_lagrange_set_group() >= 1);
    ps_ctx* ctx = NULL;
    int rc = ps_ctx_create(0, &ctx);
    if (rc == PS_ERR_NO_DEVICE) { printf("no gfx950 device: %s\n", ps_last_error()); return 77; }
    CHECK(rc == PS_OK);

    /* the domain: five gates, five variables, left = the identity, right = out = the first variable */
    uint32_t row_ptr[N + 1], col_id[N], col_0[N];
    int64_t ones[N];
    for (int i = 0; i < N; i++) { row_ptr[i] = (uint32_t)i; col_id[i] = (uint32_t)i; col_0[i] = 0; ones[i] = 1; }
    row_ptr[N] = N;
    ps_csr L, R;
    L.row_ptr = row_ptr; L.col = col_id; L.val = ones;
    R.row_ptr = row_ptr; R.col = col_0; R.val = ones;
    ps_qap* qap = NULL;
    CHECK(ps_qap_create(ctx, N, N, 1, &L, &R, &R, &qap) == PS_OK);

    /* the string in the clear (N + 1 powers: the verifier reads K + 1 of G2), and its Lagrange form on the nodes 1..5 */
    uint8_t pw[(N + 1) * 32];
    unsigned long long t = 1;
    for (int i = 0; i <= N; i++, t *= TAU) be32_small(pw + 32 * i, t);
    ps_scalars* pws = NULL;
    ps_points *tau_all = NULL, *tau_g1 = NULL, *lag_g1 = NULL, *tau_g2 = NULL;
    CHECK(ps_scalars_upload(ctx, pw, N + 1, &pws) == PS_OK && ps_points_from_scalars(ctx, PS_G1, pws, &tau_all) == PS_OK);
    CHECK(ps_points_from_scalars(ctx, PS_G2, pws, &tau_g2) == PS_OK && ps_points_slice(tau_all, 0, N, &tau_g1) == PS_OK);
    CHECK(ps_points_monomial_to_lagrange(ctx, qap, tau_g1, 0, &lag_g1) == PS_OK && ps_points_len(lag_g1) == N);

    const unsigned long long v[N] = {3, 1, 4, 1, 5}, zs[K] = {7, 2, 9};
    uint8_t v_be[N * 32], z_be[K * 32];
    for (int i = 0; i < N; i++) be32_small(v_be + 32 * i, v[i]);
    for (int j = 0; j < K; j++) be32_small(z_be + 32 * j, zs[j]);
    ps_scalars *values = NULL, *coeffs = NULL;
    CHECK(ps_scalars_upload(ctx, v_be, N, &values) == PS_OK);
    CHECK(ps_qap_interpolate(ctx, qap, values, 0, &coeffs) == PS_OK && ps_scalars_len(coeffs) == N);

    /* the opening: the bytes of the coefficient route */
    uint8_t commit[96], y[K * 32], y_c[K * 32], proof[96], proof_c[96], want[32];
    CHECK(ps_kzg_commit_lagrange(ctx, lag_g1, values, commit) == PS_OK);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, z_be, K, y, proof) == PS_OK);
    CHECK(ps_kzg_open_set(ctx, tau_g1, coeffs, z_be, K, y_c, proof_c) == PS_OK);
    CHECK(memcmp(y, y_c, sizeof y) == 0 && memcmp(proof, proof_c, 96) == 0);
    be32_small(want, v[zs[1] - 1]); /* at a node the value is the node's */
    CHECK(memcmp(y + 32, want, 32) == 0);
    int ok = -1;
    CHECK(ps_kzg_verify_set(ctx, tau_all, tau_g2, commit, z_be, y, K, proof, 1, &ok) == PS_OK && ok == 1);
    memcpy(y_c, y, sizeof y);
    y_c[32 + 31] ^= 1;
    CHECK(ps_kzg_verify_set(ctx, tau_all, tau_g2, commit, z_be, y_c, K, proof, 1, &ok) == PS_OK && ok == 0);

    /* the row of quotient values, the values and the remainder; its lone sum over the Lagrange-form string is the proof */
    ps_scalars *qv = NULL, *q_c = NULL;
    uint8_t qv_be[N * 32], y2[K * 32], rem[K * 32], rem_c[K * 32], sum[96];
    CHECK(ps_poly_div_roots_lagrange(ctx, qap, values, z_be, K, &qv, y2, rem) == PS_OK && ps_scalars_len(qv) == N);
    CHECK(ps_poly_div_roots(ctx, coeffs, z_be, K, &q_c, y_c, rem_c) == PS_OK && ps_scalars_len(q_c) == N - K);
    CHECK(memcmp(y2, y, sizeof y) == 0 && memcmp(y_c, y, sizeof y) == 0 && memcmp(rem, rem_c, sizeof rem) == 0);
    CHECK(ps_scalars_download(ctx, qv, 0, N, qv_be) == PS_OK);
    CHECK(ps_msm(ctx, lag_g1, qv, sum) == PS_OK && memcmp(sum, proof, 96) == 0);
    ps_scalars_free(qv);
    qv = NULL;
    CHECK(ps_poly_div_roots_lagrange(ctx, qap, values, z_be, K, &qv, y2, NULL) == PS_OK && memcmp(y2, y, sizeof y) == 0);

    /* one point alone: the single-point opening; as many points as nodes: the identity and a row of zeros */
    uint8_t one_y[32], one_pi[96], lone_y[32], lone_pi[96];
    for (int j = 0; j < K; j++) {
        CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, z_be + 32 * j, 1, one_y, one_pi) == PS_OK);
        CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, z_be + 32 * j, 1, lone_y, lone_pi) == PS_OK);
        CHECK(memcmp(one_y, lone_y, 32) == 0 && memcmp(one_pi, lone_pi, 96) == 0 && memcmp(one_y, y + 32 * j, 32) == 0);
    }
    uint8_t all_be[N * 32], all_y[N * 32], all_pi[96], all_pi_c[96], zeros[N * 32], all_qv[N * 32];
    for (int i = 0; i < N; i++) be32_small(all_be + 32 * i, (unsigned long long)(i + 1));
    memset(zeros, 0, sizeof zeros);
    ps_scalars* qz = NULL;
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, all_be, N, all_y, all_pi) == PS_OK && memcmp(all_y, v_be, sizeof all_y) == 0);
    CHECK(ps_kzg_open_set(ctx, tau_g1, coeffs, all_be, N, all_y, all_pi_c) == PS_OK && memcmp(all_pi, all_pi_c, 96) == 0);
    CHECK(ps_poly_div_roots_lagrange(ctx, qap, values, all_be, N, &qz, all_y, NULL) == PS_OK && ps_scalars_len(qz) == N);
    CHECK(ps_scalars_download(ctx, qz, 0, N, all_qv) == PS_OK && memcmp(all_qv, zeros, sizeof zeros) == 0);

    /* argument checks: equal points, no point, lengths, the group, a point that is not below r */
    ps_scalars* fewer = NULL;
    ps_points* shorter = NULL;
    uint8_t twice[K * 32], big[K * 32];
    memcpy(twice, z_be, sizeof twice);
    memcpy(twice + 64, z_be, 32);
    memset(big, 0xff, sizeof big);
    CHECK(ps_scalars_slice(values, 0, N - 1, &fewer) == PS_OK && ps_points_slice(lag_g1, 0, N - 1, &shorter) == PS_OK);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, twice, K, y2, sum) == PS_ERR_ARG);
    CHECK(strstr(ps_last_error(), "z[0]") != NULL && strstr(ps_last_error(), "z[2]") != NULL);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, z_be, 0, y2, sum) == PS_ERR_ARG);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, fewer, z_be, K, y2, sum) == PS_ERR_LENGTH);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, shorter, values, z_be, K, y2, sum) == PS_ERR_LENGTH);
    CHECK(strstr(ps_last_error(), "ps_kzg_open_set_lagrange") != NULL);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, tau_g2, values, z_be, K, y2, sum) == PS_ERR_ARG);
    CHECK(ps_kzg_open_set_lagrange(ctx, qap, lag_g1, values, big, K, y2, sum) == PS_ERR_ENCODING);
    CHECK(ps_kzg_open_set_lagrange(ctx, NULL, lag_g1, values, z_be, K, y2, sum) == PS_ERR_ARG);

    print_hex("commit", commit, sizeof commit);
    print_hex("y", y, sizeof y);
    print_hex("proof", proof, sizeof proof);
    print_hex("qv", qv_be, sizeof qv_be);
    print_hex("rem", rem, sizeof rem);

    ps_scalars_free(fewer);
    ps_points_free(shorter);
    ps_scalars_free(qz);
    ps_scalars_free(qv);
    ps_scalars_free(q_c);
    ps_scalars_free(coeffs);
    ps_scalars_free(values);
    ps_scalars_free(pws);
    ps_points_free(lag_g1);
    ps_points_free(tau_g1);
    ps_points_free(tau_all);
    ps_points_free(tau_g2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg_set_lagrange ok\n");
    return 0;
}
