// host_poly_scan_set_plan.cpp -- the index arithmetic of the set apply pass (ps_poly_div_roots, ps_kzg_open_set), checked on the
// host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/poly_scan_set_plan.hpp says how k points fall into groups of G, how long the quotient by Z_S is, which
// indices of the recurrence are stored, how large the buffers are, behind which points the accumulators are reduced and when
// a call is too large.  Against literal loops, for k = 1 .. 4G + 3 and 1024 and n in {1, k - 1, k, k + 1, T - 1 + k, T + k,
// T + k + 1, 2T + 1} (T = 2048; n = 0 is left out):
//   * group count, the points of every group (they add up to k, only the last is partial), the last group;
//   * that (blockIdx.y, l) -- as the kernel forms its point -- meets every point exactly once;
//   * the quotient length, the store predicate against a literal "i >= 1 and i - 1 < n - k" for every index of every tile, that
//     a tile the kernel leaves early stores nothing, and -- written through into a real array of the partial rows' size (ASan
//     watches the bounds) -- that every word of every partial row is met exactly once;
//   * the buffer sizes;
//   * the reduction step: never more than 32 points between two reductions;
//   * both limits at their edges, in 128-bit arithmetic.
// Prints "k n groups last nq stored" per shape for tests/test_poly_scan_set_plan_host.py, which derives them again.
#include <cstdio>
#include <vector>

#ifndef POLY_SCAN_SET_PLAN_HEADER
#define POLY_SCAN_SET_PLAN_HEADER "../playsnark_amd/csrc/poly_scan_set_plan.hpp"
#endif
#include POLY_SCAN_SET_PLAN_HEADER

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (failures++ < 20) {                                                   \
                std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                                   \
                std::fprintf(stderr, "\n");                                          \
            }                                                                        \
        }                                                                            \
    } while (0)

typedef unsigned __int128 u128;
typedef unsigned long long ull;
static const uint64_t G = POLY_SCAN_SET_GROUP, T = 2048;

static void check_k(uint64_t k, uint64_t* groups_out, uint64_t* last_out) {
    uint64_t groups = 0, last = 0;
    for (uint64_t start = 0; start < k; start += G) { groups++; last = k - start < G ? k - start : G; }
    CHECK(poly_scan_set_groups(k) == groups, "k=%llu", (ull)k);
    CHECK(poly_scan_set_last_group_len(k) == last, "k=%llu", (ull)k);
    std::vector<unsigned char> met(k, 0);
    uint64_t sum = 0;
    for (uint64_t g = 0; g < groups; g++) {
        const uint64_t len = poly_scan_set_group_len(k, g);
        CHECK(len == (g + 1 < groups ? G : last) && len >= 1, "k=%llu g=%llu", (ull)k, (ull)g);
        sum += len;
        for (uint64_t l = 0; l < len; l++) met.at(g * G + l)++;  // the kernel's j = j0 + l
    }
    CHECK(sum == k, "k=%llu", (ull)k);
    for (uint64_t j = 0; j < k; j++) CHECK(met[j] == 1, "k=%llu j=%llu", (ull)k, (ull)j);
    CHECK(poly_scan_set_weight_elems(k) == k, "k=%llu", (ull)k);
    *groups_out = groups;
    *last_out = last;
}

static void check_shape(uint64_t k, uint64_t n, uint64_t groups, uint64_t last) {
    const uint64_t nq = n > k ? n - k : 0;
    CHECK(poly_scan_set_quotient_len(n, k) == nq, "k=%llu n=%llu", (ull)k, (ull)n);
    CHECK(poly_scan_set_partial_words(n, k) == 8 * groups * nq, "k=%llu n=%llu", (ull)k, (ull)n);
    CHECK(poly_scan_total_elems(n, k) == k * ((n + T - 1) / T), "k=%llu n=%llu", (ull)k, (ull)n);
    const uint64_t tiles = poly_scan_tiles(n);
    // one partial row, written as the kernel writes it
    std::vector<unsigned char> words(8 * nq, 0);
    uint64_t stored = 0;
    for (uint64_t b = 0; b < tiles; b++) {
        bool any = false;
        for (uint64_t i = b * T; i < (b + 1) * T; i++) {
            const bool want = i >= 1 && (u128)i - 1 < (u128)nq && n > k;  // the literal "i - 1 < n - k"
            CHECK(poly_scan_set_stored(i, nq) == want, "k=%llu n=%llu i=%llu", (ull)k, (ull)n, (ull)i);
            if (!want) continue;
            any = true;
            stored++;
            CHECK(i < n, "k=%llu n=%llu i=%llu: a stored index behind the polynomial", (ull)k, (ull)n, (ull)i);
            for (int w = 0; w < 8; w++) words.at(8 * (i - 1) + w)++;
        }
        CHECK(poly_scan_set_tile_stores(b, nq) == any, "k=%llu n=%llu b=%llu", (ull)k, (ull)n, (ull)b);
    }
    CHECK(stored == nq, "k=%llu n=%llu", (ull)k, (ull)n);
    for (unsigned char c : words) CHECK(c == 1, "k=%llu n=%llu", (ull)k, (ull)n);
    // the rows lie one behind the other
    for (uint64_t g = 0; g < groups; g++) {
        CHECK(poly_scan_set_partial_word(g, 0, nq) == 8 * g * nq, "k=%llu n=%llu g=%llu", (ull)k, (ull)n, (ull)g);
        if (nq) CHECK(poly_scan_set_partial_word(g, nq - 1, nq) + 8 == 8 * (g + 1) * nq, "k=%llu n=%llu g=%llu", (ull)k, (ull)n, (ull)g);
    }
    CHECK(poly_scan_set_size_ok(n, k), "k=%llu n=%llu", (ull)k, (ull)n);
    std::printf("%llu %llu %llu %llu %llu %llu\n", (ull)k, (ull)n, (ull)groups, (ull)last, (ull)nq, (ull)stored);
}

int main() {
    CHECK(POLY_SCAN_TILE == (int)T && G >= 1 && POLY_SCAN_SET_REDUCE_EVERY == 32 && PS_KZG_SET_MAX == 1024, "geometry");
    std::vector<uint64_t> ks;
    for (uint64_t k = 1; k <= 4 * G + 3; k++) ks.push_back(k);
    ks.push_back(1024);
    for (uint64_t k : ks) {
        uint64_t groups, last;
        check_k(k, &groups, &last);
        for (uint64_t n : {(uint64_t)1, k - 1, k, k + 1, T - 1 + k, T + k, T + k + 1, 2 * T + 1})
            if (n >= 1) check_shape(k, n, groups, last);
    }
    // the reduction step: runs of points without a reduction, literally
    uint64_t run = 0, reductions = 0;
    for (uint64_t l = 0; l < 200; l++) {
        run++;
        CHECK(run <= (uint64_t)POLY_SCAN_SET_REDUCE_EVERY, "l=%llu", (ull)l);
        CHECK(poly_scan_set_reduce_after(l) == (run == (uint64_t)POLY_SCAN_SET_REDUCE_EVERY), "l=%llu", (ull)l);
        if (poly_scan_set_reduce_after(l)) { run = 0; reductions++; }
    }
    CHECK(reductions == 200 / 32, "reductions=%llu", (ull)reductions);
    // the limits: 1 <= k <= 1024 and k * n < 2^32
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1023, (uint64_t)1024, (uint64_t)1025, (uint64_t)1 << 20, ~(uint64_t)0}) {
        CHECK(poly_scan_set_points_ok(k) == (k >= 1 && k <= 1024), "k=%llu", (ull)k);
        for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)1 << 20, (uint64_t)4194303, (uint64_t)4194304, (uint64_t)4194305, (uint64_t)0xffffffffull,
                           (uint64_t)1 << 32, ~(uint64_t)0}) {
            const bool want = k >= 1 && k <= 1024 && (u128)k * n < ((u128)1 << 32);
            CHECK(poly_scan_set_size_ok(n, k) == want, "k=%llu n=%llu", (ull)k, (ull)n);
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_poly_scan_set_plan ok\n");
    return 0;
}
