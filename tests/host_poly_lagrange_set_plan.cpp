// host_poly_lagrange_set_plan.cpp -- the index arithmetic of the value-form set quotient (ps_poly_div_roots_lagrange,
// ps_kzg_open_set_lagrange), checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/poly_lagrange_set_plan.hpp says how the k points of a set fall into groups of G, which (node, point) the
// item m of thread t of tile b meets as point number l of group g and back, where a thread's LDS slots and the partial rows'
// elements lie, how large the buffers are and when a call is too large.  Against literal loops, for n around 1, T and 2T (each
// +- 1) and k around 1, G and 2G (each +- 1):
//   * group count and group lengths (they add up to k, only the last is partial), point <-> (group, number) round trips;
//   * every (tile, group, thread, item, number) -> (node, point), every pair of 1 .. n x 0 .. k-1 met exactly once, and back;
//   * the partial rows written through into a real array of their size (ASan watches the bounds): every element of every row
//     met exactly once, no row beside the result for one group; the weights and the LDS slots likewise, within the LDS limit;
//   * the limits (1 <= k <= 1024, n >= 1, k * n < 2^32) at their edges, in 128-bit arithmetic; the zero quotient for k >= n.
// Prints "n k groups last rows" per pair for tests/test_poly_lagrange_set_plan_host.py, which derives them again.
#include <cstdio>
#include <vector>

#ifndef POLY_LAGRANGE_SET_PLAN_HEADER
#define POLY_LAGRANGE_SET_PLAN_HEADER "../playsnark_amd/csrc/poly_lagrange_set_plan.hpp"
#endif
#include POLY_LAGRANGE_SET_PLAN_HEADER

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
static const uint64_t I = POLY_LAGR_ITEMS, T = POLY_LAGR_TILE, G = POLY_LAGR_SET_GROUP, TH = POLY_LAGR_THREADS;

static void check_pair(uint64_t n, uint64_t k) {
    CHECK(poly_lagr_set_points_ok(k) && poly_lagr_set_size_ok(n, k), "n=%llu k=%llu", (ull)n, (ull)k);
    uint64_t groups = 0, last = 0;
    for (uint64_t start = 0; start < k; start += G) { groups++; last = k - start < G ? k - start : G; }
    CHECK(poly_lagr_set_groups(k) == groups, "k=%llu", (ull)k);
    uint64_t sum = 0;
    for (uint64_t g = 0; g < groups; g++) {
        const uint64_t len = poly_lagr_set_group_len(k, g);
        CHECK(len == (g + 1 < groups ? G : last) && len >= 1, "k=%llu g=%llu", (ull)k, (ull)g);
        sum += len;
    }
    CHECK(sum == k, "k=%llu", (ull)k);
    for (uint64_t j = 0; j < k; j++) {
        const uint64_t g = poly_lagr_set_point_group(j), l = poly_lagr_set_point_slot(j);
        CHECK(g < groups && l < poly_lagr_set_group_len(k, g) && poly_lagr_set_point(g, l) == j, "k=%llu j=%llu", (ull)k, (ull)j);
    }
    // the buffers: the weights, and the partial rows -- none beside the result for one group
    const uint64_t rows = groups > 1 ? groups : 0;
    CHECK(poly_lagr_set_partial_rows(k) == rows && poly_lagr_set_partial_words(n, k) == 8 * rows * n && poly_lagr_set_weight_elems(k) == k, "n=%llu k=%llu",
          (ull)n, (ull)k);
    // the fold's grid, as the kernel walks it: every (node, point) once; a row written as the kernel writes it (into the result
    // for one group: a buffer of one row)
    const uint64_t tiles = poly_lagr_tiles(n);
    std::vector<unsigned char> met(n * k, 0), part((rows ? rows : 1) * n, 0), weights(poly_lagr_set_weight_elems(k), 0);
    for (uint64_t g = 0; g < groups; g++)
        for (uint64_t b = 0; b < tiles; b++)
            for (uint64_t t = 0; t < TH; t++) {
                const uint64_t first = poly_lagr_set_node(b, t, 0);
                CHECK(first == b * T + t * I + 1, "b=%llu t=%llu", (ull)b, (ull)t);
                for (uint64_t l = 0; l < poly_lagr_set_group_len(k, g); l++) {
                    const uint64_t j = poly_lagr_set_point(g, l);
                    CHECK(j == g * G + l && j < k, "g=%llu l=%llu", (ull)g, (ull)l);
                    if (b == 0 && t == 0) weights.at(j)++;
                    for (uint64_t m = 0; m < I; m++) {
                        const uint64_t node = poly_lagr_set_node(b, t, m);
                        CHECK(node == first + m && poly_lagr_node_tile(node) == b && poly_lagr_node_thread(node) == t && poly_lagr_node_item(node) == m,
                              "node=%llu", (ull)node);
                        if (node <= n) met.at((node - 1) * k + j)++;
                    }
                }
                for (uint64_t m = 0; m < I; m++) {  // the store: row g, the thread's nodes from `first` on
                    if (first + m > n) continue;
                    const uint64_t word = poly_lagr_set_partial_word(g, first, n) + 8 * m;
                    CHECK(word == poly_lagr_set_partial_word(g, first + m, n) && word % 8 == 0, "g=%llu node=%llu", (ull)g, (ull)(first + m));
                    CHECK(rows == 0 || word + 8 <= poly_lagr_set_partial_words(n, k), "g=%llu node=%llu", (ull)g, (ull)(first + m));
                    part.at(word / 8)++;
                }
            }
    for (unsigned char c : met) CHECK(c == 1, "n=%llu k=%llu: a (node, point) pair", (ull)n, (ull)k);
    for (unsigned char c : part) CHECK(c == 1, "n=%llu k=%llu: an element of a partial row", (ull)n, (ull)k);
    for (unsigned char c : weights) CHECK(c == 1, "k=%llu: a weight", (ull)k);
    CHECK(poly_lagr_set_zero(n, k) == (k >= n), "n=%llu k=%llu", (ull)n, (ull)k);
    std::printf("%llu %llu %llu %llu %llu\n", (ull)n, (ull)k, (ull)groups, (ull)last, (ull)rows);
}

int main() {
    CHECK(G >= 1 && G <= 32 && POLY_LAGR_SET_MAX == 1024 && I == 2 * (uint64_t)POLY_LAGR_SET_HALF, "geometry");
    // the LDS of a workgroup: the scan's two arrays double as the H - 1 half products, the slots of the points 1 .. G - 1 of a
    // group lie behind one another, one element per thread, and everything fits the limit
    CHECK(POLY_LAGR_SET_SCRATCH_ARRAYS >= 2 && POLY_LAGR_SET_SCRATCH_ARRAYS >= (uint64_t)POLY_LAGR_SET_HALF - 1, "scratch");
    CHECK(POLY_LAGR_SET_LDS_ELEMS * POLY_LAGR_SET_FR_BYTES <= (uint64_t)POLY_LAGR_SET_LDS_MAX, "LDS");
    {
        std::vector<unsigned char> slot(POLY_LAGR_SET_SLOT_ARRAYS * TH, 0);
        for (uint64_t l = 1; l < G; l++)
            for (uint64_t t = 0; t < TH; t++) slot.at(poly_lagr_set_slot_elem(l, t))++;
        for (size_t i = 0; i < slot.size(); i++) CHECK(slot[i] == (G > 1 ? 1 : 0), "slot %llu", (ull)i);
    }
    for (uint64_t n : {(uint64_t)1, (uint64_t)2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1})
        for (uint64_t k : {(uint64_t)1, (uint64_t)2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1})
            if (k >= 1) check_pair(n, k);
    // the largest set: 1024 points in ceil(1024 / G) groups, blockIdx.y wide enough
    CHECK(poly_lagr_set_groups(POLY_LAGR_SET_MAX) == (1024 + G - 1) / G && poly_lagr_set_groups(POLY_LAGR_SET_MAX) <= 65535, "groups of the largest set");
    // the limits: 1 <= k <= 1024, n >= 1 and k * n < 2^32
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1023, (uint64_t)1024, (uint64_t)1025, (uint64_t)1 << 20, (uint64_t)0xffffffffull,
                       (uint64_t)1 << 32, ~(uint64_t)0}) {
        CHECK(poly_lagr_set_points_ok(k) == (k >= 1 && k <= 1024), "k=%llu", (ull)k);
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1 << 20, (uint64_t)4194303, (uint64_t)4194304, (uint64_t)4194305,
                           (uint64_t)0xffffffffull, (uint64_t)1 << 32, ~(uint64_t)0}) {
            const bool want = k >= 1 && k <= 1024 && n >= 1 && (u128)k * n < ((u128)1 << 32);
            CHECK(poly_lagr_set_size_ok(n, k) == want, "k=%llu n=%llu", (ull)k, (ull)n);
            // what passes the limits has partial rows whose word count fits 64 bits with room to spare
            if (want) CHECK((u128)poly_lagr_set_partial_words(n, k) == (u128)8 * poly_lagr_set_partial_rows(k) * n, "k=%llu n=%llu", (ull)k, (ull)n);
        }
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_poly_lagrange_set_plan ok\n");
    return 0;
}
