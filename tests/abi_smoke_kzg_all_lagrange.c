/* abi_smoke_kzg_all_lagrange.c -- the KZG proofs of EVERY node of the domain 1..5 for a polynomial held as its VALUES, through
 * the C ABI the way a cgo caller uses it: plain C99, nothing but include/playsnark_hip.h.  The domain is a ps_qap of five gates;
 * the string is held in the clear (tau = 11) and put into Lagrange form by ps_points_monomial_to_lagrange.
 *   - ps_kzg_all_key_lagrange gives five points; ps_kzg_open_all_lagrange gives the same five proofs with the table and with
 *     all_key = NULL, and they are ps_kzg_open_lagrange's proofs at z = 1..5 byte for byte;
 *   - ps_kzg_verify accepts each against ps_kzg_commit_lagrange's commitment and the node's own value, and rejects a changed one;
 *   - the argument rules: lengths, the group, NULL arguments;
 *   - the bytes are printed as `name hex` lines for tests/test_kzg_all_lagrange_c_abi.py, which compares them with the oracle.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_kzg_all_lagrange.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_kzg_all_lagrange
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            fprintf(stderr, "abi_smoke_kzg_all_lagrange: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
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
#define TAU 11ull

int main(void) {
    CHECK(ps_abi_version() == PS_ABI_VERSION);
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

    /* the string in the clear and its Lagrange form on the nodes 1..5; tau G2 for the verifier */
    uint8_t pw[N * 32], tau_g2_1[192];
    unsigned long long t = 1;
    for (int i = 0; i < N; i++, t *= TAU) be32_small(pw + 32 * i, t);
    ps_scalars* pws = NULL;
    ps_points *tau_g1 = NULL, *lag_g1 = NULL, *tau_g2 = NULL;
    CHECK(ps_scalars_upload(ctx, pw, N, &pws) == PS_OK && ps_points_from_scalars(ctx, PS_G1, pws, &tau_g1) == PS_OK);
    CHECK(ps_points_from_scalars(ctx, PS_G2, pws, &tau_g2) == PS_OK && ps_points_download(ctx, tau_g2, 1, 1, tau_g2_1) == PS_OK);
    CHECK(ps_points_monomial_to_lagrange(ctx, qap, tau_g1, 0, &lag_g1) == PS_OK && ps_points_len(lag_g1) == N);

    const unsigned long long v[N] = {3, 1, 4, 1, 5};
    uint8_t v_be[N * 32], nodes_be[N * 32];
    for (int i = 0; i < N; i++) { be32_small(v_be + 32 * i, v[i]); be32_small(nodes_be + 32 * i, (unsigned long long)(i + 1)); }
    ps_scalars* values = NULL;
    CHECK(ps_scalars_upload(ctx, v_be, N, &values) == PS_OK);

    /* the table, the proofs with it and without it, and the single-point openings at the same nodes */
    ps_points *key = NULL, *proofs = NULL, *proofs_nokey = NULL;
    uint8_t commit[96], key_b[N * 96], pi[N * 96], pi_nokey[N * 96], pi_single[N * 96], y[N * 32];
    CHECK(ps_kzg_commit_lagrange(ctx, lag_g1, values, commit) == PS_OK);
    CHECK(ps_kzg_all_key_lagrange(ctx, qap, lag_g1, &key) == PS_OK && ps_points_len(key) == N && ps_points_group(key) == PS_G1);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, key, values, &proofs) == PS_OK && ps_points_len(proofs) == N);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, NULL, values, &proofs_nokey) == PS_OK && ps_points_len(proofs_nokey) == N);
    CHECK(ps_points_download(ctx, key, 0, N, key_b) == PS_OK && ps_points_download(ctx, proofs, 0, N, pi) == PS_OK);
    CHECK(ps_points_download(ctx, proofs_nokey, 0, N, pi_nokey) == PS_OK && memcmp(pi, pi_nokey, sizeof pi) == 0);
    CHECK(ps_kzg_open_lagrange(ctx, qap, lag_g1, values, nodes_be, N, y, pi_single) == PS_OK);
    CHECK(memcmp(y, v_be, sizeof y) == 0 && memcmp(pi, pi_single, sizeof pi) == 0);

    /* every opening verifies against the node's own value, and not against another */
    for (int m = 0; m < N; m++) {
        int ok = -1;
        uint8_t bad[32];
        CHECK(ps_kzg_verify(tau_g2_1, commit, nodes_be + 32 * m, v_be + 32 * m, pi + 96 * m, &ok) == PS_OK && ok == 1);
        memcpy(bad, v_be + 32 * m, 32);
        bad[31] ^= 1;
        CHECK(ps_kzg_verify(tau_g2_1, commit, nodes_be + 32 * m, bad, pi + 96 * m, &ok) == PS_OK && ok == 0);
    }

    /* argument checks: lengths, the group, NULL arguments (all_key alone may be NULL) */
    ps_scalars* fewer = NULL;
    ps_points *shorter = NULL, *short_key = NULL, *out = NULL;
    CHECK(ps_scalars_slice(values, 0, N - 1, &fewer) == PS_OK && ps_points_slice(lag_g1, 0, N - 1, &shorter) == PS_OK);
    CHECK(ps_points_slice(key, 0, N - 1, &short_key) == PS_OK);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, key, fewer, &out) == PS_ERR_LENGTH && out == NULL);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, shorter, key, values, &out) == PS_ERR_LENGTH);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, short_key, values, &out) == PS_ERR_LENGTH);
    CHECK(strstr(ps_last_error(), "ps_kzg_open_all_lagrange") != NULL);
    CHECK(ps_kzg_all_key_lagrange(ctx, qap, shorter, &out) == PS_ERR_LENGTH && strstr(ps_last_error(), "ps_kzg_all_key_lagrange") != NULL);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, tau_g2, key, values, &out) == PS_ERR_ARG);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, tau_g2, values, &out) == PS_ERR_ARG);
    CHECK(ps_kzg_all_key_lagrange(ctx, qap, tau_g2, &out) == PS_ERR_ARG);
    CHECK(ps_kzg_open_all_lagrange(ctx, NULL, lag_g1, key, values, &out) == PS_ERR_ARG);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, key, NULL, &out) == PS_ERR_ARG);
    CHECK(ps_kzg_open_all_lagrange(ctx, qap, lag_g1, key, values, NULL) == PS_ERR_ARG);
    CHECK(ps_kzg_all_key_lagrange(ctx, qap, NULL, &out) == PS_ERR_ARG && ps_kzg_all_key_lagrange(ctx, qap, lag_g1, NULL) == PS_ERR_ARG);

    print_hex("commit", commit, sizeof commit);
    print_hex("key", key_b, sizeof key_b);
    print_hex("proofs", pi, sizeof pi);

    ps_scalars_free(fewer);
    ps_points_free(shorter);
    ps_points_free(short_key);
    ps_points_free(proofs_nokey);
    ps_points_free(proofs);
    ps_points_free(key);
    ps_scalars_free(values);
    ps_scalars_free(pws);
    ps_points_free(lag_g1);
    ps_points_free(tau_g1);
    ps_points_free(tau_g2);
    ps_qap_free(qap);
    ps_ctx_destroy(ctx);
    printf("abi_smoke_kzg_all_lagrange ok\n");
    return 0;
}
