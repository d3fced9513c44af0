// host_poly_lagrange_plan.cpp -- the index arithmetic of the value-form evaluation and quotient (ps_poly_eval_lagrange,
// ps_poly_div_linear_lagrange, ps_kzg_open_lagrange), checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/poly_lagrange_plan.hpp says how the nodes 1 .. n fall into tiles of T = 256 I, which node item m of thread t
// of tile b is and back, which point is a node, where a row's elements lie, how the walk cuts the tiles into chunks, how large the
// buffers are and when a call is too large.  Against literal loops, for n around 1, T and 2T (each +- 1) and k in {1, 2, 3}:
//   * tile count and tile lengths (they add up to n, only the last is partial);
//   * every (tile, thread, item) -> node -> (tile, thread, item) round trip, every node of 1 .. n met exactly once, and -- written
//     through into real arrays of the rows' and the partials' size (ASan watches the bounds) -- every element met exactly once;
//   * the node-m lookup (poly_lagr_hit) for every z in 0 .. n + 2, at both edges of every tile, and for values with a high word;
//   * chunks of the walk and the reduction step: never more than 32 additions between two reductions;
//   * the apply pass's blocks; the limits (n >= 1, k * n < 2^32) at their edges, in 128-bit arithmetic.
// Prints "n tiles last chunks" per n for tests/test_poly_lagrange_plan_host.py, which derives them again.
#include <cstdio>
#include <vector>

#ifndef POLY_LAGRANGE_PLAN_HEADER
#define POLY_LAGRANGE_PLAN_HEADER "../playsnark_amd/csrc/poly_lagrange_plan.hpp"
#endif
#include POLY_LAGRANGE_PLAN_HEADER

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
static const uint64_t I = POLY_LAGR_ITEMS, T = POLY_LAGR_TILE;

static void check_n(uint64_t n) {
    uint64_t tiles = 0, last = 0;
    for (uint64_t start = 0; start < n; start += T) { tiles++; last = n - start < T ? n - start : T; }
    CHECK(poly_lagr_tiles(n) == tiles, "n=%llu", (ull)n);
    uint64_t sum = 0;
    for (uint64_t b = 0; b < tiles; b++) {
        const uint64_t len = poly_lagr_tile_len(n, b);
        CHECK(len == (b + 1 < tiles ? T : last) && len >= 1, "n=%llu b=%llu", (ull)n, (ull)b);
        sum += len;
    }
    CHECK(sum == n, "n=%llu", (ull)n);
    // the round trip, as the tile kernel forms its nodes; a row and the partials written as the kernels write them
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)3}) {
        CHECK(poly_lagr_total_ok(n, k), "n=%llu k=%llu", (ull)n, (ull)k);
        CHECK(poly_lagr_row_words(n, k) == 8 * k * n && poly_lagr_value_words(k) == 8 * k && poly_lagr_yq_elems(k) == 2 * k, "n=%llu", (ull)n);
        CHECK(poly_lagr_plane_elems(n, k) == k * tiles && poly_lagr_part_elems(n, k) == 3 * k * tiles, "n=%llu k=%llu", (ull)n, (ull)k);
        std::vector<unsigned char> rows(poly_lagr_row_words(n, k) / 8, 0), parts(poly_lagr_part_elems(n, k), 0);
        for (uint64_t j = 0; j < k; j++) {
            uint64_t met = 0;
            for (uint64_t b = 0; b < tiles; b++) {
                for (uint64_t t = 0; t < (uint64_t)POLY_LAGR_THREADS; t++)
                    for (uint64_t m = 0; m < I; m++) {
                        const uint64_t node = poly_lagr_node(b, t, m);
                        CHECK(node == b * T + t * I + m + 1, "b=%llu t=%llu m=%llu", (ull)b, (ull)t, (ull)m);
                        CHECK(poly_lagr_node_tile(node) == b && poly_lagr_node_thread(node) == t && poly_lagr_node_item(node) == m,
                              "n=%llu node=%llu", (ull)n, (ull)node);
                        if (node > n) continue;  // behind the end: takes no part
                        met++;
                        rows.at(poly_lagr_row_elem(j, node, n))++;
                    }
                for (uint64_t plane = 0; plane < (uint64_t)POLY_LAGR_PARTS; plane++) {
                    // the kernel's plane * (k * tiles) + j * tiles + b
                    CHECK(poly_lagr_part_elem(plane, j, b, n, k) == plane * poly_lagr_plane_elems(n, k) + j * tiles + b, "n=%llu", (ull)n);
                    parts.at(poly_lagr_part_elem(plane, j, b, n, k))++;
                }
            }
            CHECK(met == n, "n=%llu j=%llu met=%llu", (ull)n, (ull)j, (ull)met);
        }
        for (unsigned char c : rows) CHECK(c == 1, "n=%llu k=%llu: a row element", (ull)n, (ull)k);
        for (unsigned char c : parts) CHECK(c == 1, "n=%llu k=%llu: a partial", (ull)n, (ull)k);
    }
    // which point is a node: every small z, and both edges of every tile
    for (uint64_t z = 0; z <= n + 2; z++) {
        uint32_t w[8] = {(uint32_t)z, 0, 0, 0, 0, 0, 0, 0};
        const uint64_t want = z >= 1 && z <= n ? z : 0;
        CHECK(poly_lagr_hit(w, n) == want, "n=%llu z=%llu", (ull)n, (ull)z);
        for (int hi = 1; hi < 8; hi++) {  // the same low word under a high one: far off the domain
            w[hi] = 1;
            CHECK(poly_lagr_hit(w, n) == 0, "n=%llu z=%llu hi=%d", (ull)n, (ull)z, hi);
            w[hi] = 0;
        }
    }
    for (uint64_t b = 0; b < tiles; b++) {
        const uint64_t first = b * T + 1, lastn = b * T + poly_lagr_tile_len(n, b);
        CHECK(poly_lagr_node_tile(first) == b && poly_lagr_node_thread(first) == 0 && poly_lagr_node_item(first) == 0, "n=%llu b=%llu", (ull)n, (ull)b);
        CHECK(poly_lagr_node_tile(lastn) == b && poly_lagr_node(b, poly_lagr_node_thread(lastn), poly_lagr_node_item(lastn)) == lastn, "n=%llu b=%llu",
              (ull)n, (ull)b);
        if (lastn == (b + 1) * T)
            CHECK(poly_lagr_node_thread(lastn) == (uint64_t)POLY_LAGR_THREADS - 1 && poly_lagr_node_item(lastn) == I - 1, "n=%llu b=%llu", (ull)n, (ull)b);
    }
    // the apply pass: one node per thread
    CHECK(poly_lagr_apply_blocks(n) == (n + 255) / 256 && poly_lagr_apply_blocks(n) * 256 >= n && (poly_lagr_apply_blocks(n) - 1) * 256 < n, "n=%llu", (ull)n);
    std::printf("%llu %llu %llu %llu\n", (ull)n, (ull)tiles, (ull)last, (ull)poly_lagr_chunks(tiles));
}

int main() {
    CHECK(T == 256 * I && I >= 2 && POLY_LAGR_CHUNK == 256 && POLY_LAGR_REDUCE_EVERY == 32 && POLY_LAGR_PARTS == 3, "geometry");
    for (uint64_t n : {(uint64_t)1, (uint64_t)2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1}) check_n(n);
    // chunks of the walk, literally, up to the 2^21 tiles and more that k * n < 2^32 allows
    for (uint64_t tiles : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)513, (uint64_t)1 << 21, ((uint64_t)1 << 24) + 1}) {
        uint64_t chunks = 0, sum = 0;
        for (uint64_t start = 0; start < tiles; start += 256) chunks++;
        CHECK(poly_lagr_chunks(tiles) == chunks, "tiles=%llu", (ull)tiles);
        for (uint64_t c = 0; c < chunks && chunks <= 4096; c++) sum += poly_lagr_chunk_len(tiles, c);
        if (chunks <= 4096) CHECK(sum == tiles, "tiles=%llu", (ull)tiles);
        CHECK(poly_lagr_chunk_len(tiles, chunks - 1) == tiles - (chunks - 1) * 256, "tiles=%llu", (ull)tiles);
    }
    // the reduction step: runs of chunks without a reduction, literally
    uint64_t run = 0, reductions = 0;
    for (uint64_t c = 0; c < 200; c++) {
        run++;
        CHECK(run <= (uint64_t)POLY_LAGR_REDUCE_EVERY, "c=%llu", (ull)c);
        CHECK(poly_lagr_reduce_after(c) == (run == (uint64_t)POLY_LAGR_REDUCE_EVERY), "c=%llu", (ull)c);
        if (poly_lagr_reduce_after(c)) { run = 0; reductions++; }
    }
    CHECK(reductions == 200 / 32, "reductions=%llu", (ull)reductions);
    // the limits: n >= 1 and k * n < 2^32
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1023, (uint64_t)1024, (uint64_t)1 << 20, (uint64_t)0xffffffffull, (uint64_t)1 << 32,
                       ~(uint64_t)0})
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)1 << 20, (uint64_t)4194303, (uint64_t)4194304, (uint64_t)4194305,
                           (uint64_t)0xffffffffull, (uint64_t)1 << 32, ~(uint64_t)0}) {
            const bool want = n >= 1 && (u128)k * n < ((u128)1 << 32);
            CHECK(poly_lagr_total_ok(n, k) == want, "k=%llu n=%llu", (ull)k, (ull)n);
        }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_poly_lagrange_plan ok\n");
    return 0;
}
