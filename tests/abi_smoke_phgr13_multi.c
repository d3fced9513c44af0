/* abi_smoke_phgr13_multi.c -- PHGR13Prove (pinochio.go:207-254) over index ranges through the C ABI, the way a cgo caller
 * uses it: plain C99, no Python.  Proves the reference's toy circuit x^3 + x + 5 = 35 (r1cs.go:178-198, witness
 * r1cs.go:67-76) against the committed golden fixture tests/golden/phgr13_toy.json (handed over by
 * tests/test_phgr13_multi_abi.py as a flat "name hex" text file):
 *   - ps_phgr13_prove_multi with two contexts, each holding only its index ranges of the evaluation key;
 *   - ps_phgr13_prove_shard for ranks 0 and 1 of 2 over the whole key, the two parts added with ps_points_sum;
 *   - one refusal: a device that does not hold its range is PS_ERR_LENGTH.
 *
 *   gcc -std=c99 -Wall -Iinclude tests/abi_smoke_phgr13_multi.c -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_phgr13_multi
 *   ./abi_smoke_phgr13_multi fixture.txt
 * Exit codes: 0 = all checks passed, 77 = no gfx950 device (the library has no CPU fallback), 1 = failure.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "playsnark_hip.h"

#define MAXF 32
static struct { char name[32]; uint8_t* data; size_t len; } fx[MAXF];
static int nfx = 0;

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

static int load_fixture(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    static char line[1 << 16];
    while (fgets(line, sizeof line, f) && nfx < MAXF) {
        char* sp = strchr(line, ' ');
        if (!sp) continue;
        *sp++ = 0;
        size_t hl = strcspn(sp, "\r\n");
        strncpy(fx[nfx].name, line, sizeof fx[nfx].name - 1);
        fx[nfx].len = hl / 2;
        fx[nfx].data = (uint8_t*)malloc(hl / 2 + 1);
        for (size_t i = 0; i < hl / 2; i++) fx[nfx].data[i] = (uint8_t)(hexval(sp[2 * i]) << 4 | hexval(sp[2 * i + 1]));
        nfx++;
    }
    fclose(f);
    return 0;
}
static const uint8_t* get(const char* name, size_t want_len) {
    for (int i = 0; i < nfx; i++)
        if (!strcmp(fx[i].name, name)) {
            if (fx[i].len != want_len) { fprintf(stderr, "fixture %s: %zu bytes, expected %zu\n", name, fx[i].len, want_len); exit(1); }
            return fx[i].data;
        }
    fprintf(stderr, "fixture %s missing\n", name);
    exit(1);
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "abi_smoke_phgr13_multi: %s:%d: %s failed (last error: %s)\n", __FILE__, __LINE__, #cond, ps_last_error()); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

/* the evaluation-key arrays in the order of ps_phgr13_ek; ws is G2 */
static const char* const EK_NAMES[10] = {"vs", "ws", "ys", "vas", "was", "yas", "gsi", "vbs", "wbs", "ybs"};
static const ps_points** ek_slot(ps_phgr13_ek* ek, int k) {
    const ps_points** s[10] = {&ek->vs, &ek->ws, &ek->ys, &ek->vas, &ek->was, &ek->yas, &ek->gsi, &ek->vbs, &ek->wbs, &ek->ybs};
    return s[k];
}

/* the eight proof elements in the order of ps_phgr13_proof */
static const char* const PROOF_NAMES[8] = {"vss", "vass", "wss", "wass", "yss", "yass", "hs", "gz"};
static uint8_t* proof_slot(ps_phgr13_proof* p, int k) {
    uint8_t* s[8] = {p->vss, p->vass, p->wss, p->wass, p->yss, p->yass, p->hs, p->gz};
    return s[k];
}
static size_t proof_len(int k) { return k == 2 ? 192 : 96; }

static int proof_matches(ps_phgr13_proof* p) {
    for (int k = 0; k < 8; k++)
        if (memcmp(proof_slot(p, k), get(PROOF_NAMES[k], proof_len(k)), proof_len(k))) {
            fprintf(stderr, "proof element %s differs from the fixture\n", PROOF_NAMES[k]);
            return 0;
        }
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2 || load_fixture(argv[1])) { fprintf(stderr, "usage: abi_smoke_phgr13_multi fixture.txt\n"); return 1; }
    CHECK(ps_abi_version() == PS_ABI_VERSION);
    CHECK(sizeof(ps_phgr13_device) == 3 * sizeof(void*) + sizeof(ps_phgr13_ek) && sizeof(ps_phgr13_ek) == 11 * sizeof(void*));
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

    /* every array of the key has 3 points (3 non-IO variables; n-1 = 3 values of h): device 0 holds [0, 2), device 1 [2, 3) */
    ps_phgr13_device dev[2];
    memset(dev, 0, sizeof dev); /* the header requires zero-initialised structs (lgsi absent) */
    ps_points* part[2][10];
    for (int d = 0; d < 2; d++) {
        const size_t first = d ? 2 : 0, cnt = d ? 1 : 2;
        for (int k = 0; k < 10; k++) {
            const int group = k == 1 ? PS_G2 : PS_G1;
            const size_t pb = group == PS_G2 ? 192 : 96;
            CHECK(ps_points_upload(ctxs[d], group, get(EK_NAMES[k], 3 * pb) + first * pb, cnt, PS_FMT_AFFINE, &part[d][k]) == PS_OK);
            *ek_slot(&dev[d].ek, k) = part[d][k];
        }
        dev[d].ctx = ctxs[d];
        dev[d].qap = qap[d];
        dev[d].sol = sol[d];
    }
    ps_phgr13_proof proof;
    CHECK(ps_phgr13_prove_multi(dev, 2, &proof) == PS_OK);
    CHECK(proof_matches(&proof));
    CHECK(ps_phgr13_prove_multi(dev, 2, &proof) == PS_OK && proof_matches(&proof)); /* again, on warm contexts */

    /* a key that is not cut at the index ranges is refused, as BlindEval's length panic (algebra.go:350-352) */
    dev[1].ek.gsi = part[0][6]; /* 2 points where device 1 must hold 1 */
    CHECK(ps_phgr13_prove_multi(dev, 2, &proof) == PS_ERR_LENGTH);
    CHECK(strstr(ps_last_error(), "device 1") != NULL);
    dev[1].ek.gsi = part[1][6];
    CHECK(ps_phgr13_prove_multi(dev, 2, &proof) == PS_OK && proof_matches(&proof));

    /* the one-process-per-GPU form: ranks 0 and 1 of 2 over the whole key, their parts added element by element */
    ps_phgr13_ek whole;
    memset(&whole, 0, sizeof whole);
    ps_points* all[10];
    for (int k = 0; k < 10; k++) {
        const int group = k == 1 ? PS_G2 : PS_G1;
        const size_t pb = group == PS_G2 ? 192 : 96;
        CHECK(ps_points_upload(ctxs[0], group, get(EK_NAMES[k], 3 * pb), 3, PS_FMT_AFFINE, &all[k]) == PS_OK);
        *ek_slot(&whole, k) = all[k];
    }
    ps_phgr13_proof shares[2], folded;
    CHECK(ps_phgr13_prove_shard(ctxs[0], &whole, qap[0], sol[0], 0, 2, &shares[0]) == PS_OK);
    CHECK(ps_phgr13_prove_shard(ctxs[0], &whole, qap[0], sol[0], 1, 2, &shares[1]) == PS_OK);
    for (int k = 0; k < 8; k++) {
        uint8_t two[2 * 192];
        const size_t len = proof_len(k);
        memcpy(two, proof_slot(&shares[0], k), len);
        memcpy(two + len, proof_slot(&shares[1], k), len);
        CHECK(ps_points_sum(k == 2 ? PS_G2 : PS_G1, two, 2, proof_slot(&folded, k)) == PS_OK);
    }
    CHECK(proof_matches(&folded));
    CHECK(ps_phgr13_prove_shard(ctxs[0], &whole, qap[0], sol[0], 2, 2, &shares[0]) == PS_ERR_ARG);

    for (int k = 0; k < 10; k++) {
        ps_points_free(all[k]);
        for (int d = 0; d < 2; d++) ps_points_free(part[d][k]);
    }
    for (int d = 0; d < 2; d++) {
        ps_scalars_free(sol[d]);
        ps_qap_free(qap[d]);
        ps_ctx_destroy(ctxs[d]);
    }
    printf("abi_smoke_phgr13_multi ok: the toy PHGR13 proof equals the golden fixture through ps_phgr13_prove_multi (two contexts over "
           "rank-local keys) and through two ps_phgr13_prove_shard parts folded; a key not cut at the ranges is PS_ERR_LENGTH\n");
    return 0;
}
