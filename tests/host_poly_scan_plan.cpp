// host_poly_scan_plan.cpp -- the index arithmetic of the polynomial scan (ps_poly_eval, ps_poly_div_linear), checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/poly_scan_plan.hpp says how n coefficients fall into tiles of T, the tiles into chunks of 256, which power
// of z every carry meets, how large the buffers are and when k * n is too much.  For n = 1 .. 3T + 2, the chunk edges
// 256 T - 1, 256 T, 256 T + 1, 2 * 256 T + 1 and 2^32 - 1, against literal loops:
//   * tile count, the length of every tile (they add up to n), the last tile's length;
//   * chunk count, the length of every chunk (they add up to the tile count);
//   * the exponent of the carry at every coefficient (n <= 3T + 2: all of them; beyond: the edges of every tile), and that the
//     kernels reach it: (I - m) Horner steps inside the thread plus the doubling steps of the (255 - t) threads behind it, each
//     step s multiplying by entry log2(I) + s of {z^(2^k)}; likewise T 2^s = 2^(log2(T) + s) for the tiles of a chunk; no table
//     index reaches POLY_SCAN_POWERS;
//   * buffer sizes for k = 1, 2, 5, 65 535, 65 536, in 128-bit arithmetic;
//   * the k * n bound at k = floor((2^32 - 1) / n) and one more.
// Prints "n tiles last chunks" per n for tests/test_poly_scan_plan_host.py, which derives the three again.
#include <cstdio>
#include <vector>

#ifndef POLY_SCAN_PLAN_HEADER
#define POLY_SCAN_PLAN_HEADER "../playsnark_amd/csrc/poly_scan_plan.hpp"
#endif
#include POLY_SCAN_PLAN_HEADER

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
static const uint64_t T = POLY_SCAN_TILE, I = POLY_SCAN_ITEMS;

// the exponent at coefficient i, literally: steps to the first multiple of T behind i
static uint64_t exponent_literal(uint64_t i) {
    uint64_t e = 0;
    do { i++; e++; } while (i % T != 0);
    return e;
}
// ... and as the kernels compose it
static void check_exponent(uint64_t i) {
    const uint64_t want = exponent_literal(i);
    CHECK(poly_scan_carry_exponent(i) == want, "i=%llu", (unsigned long long)i);
    CHECK(want >= 1 && want <= T, "i=%llu", (unsigned long long)i);
    const uint64_t in_tile = i % T, t = in_tile / I, m = in_tile % I;
    uint64_t reached = I - m;  // Horner steps from the thread's end down to item m
    const uint64_t behind = POLY_SCAN_THREADS - 1 - t;
    for (int s = 0; s < 8; s++)
        if ((behind >> s) & 1) {
            CHECK(poly_scan_thread_power(s) < POLY_SCAN_POWERS, "s=%d", s);
            reached += 1ull << poly_scan_thread_power(s);
        }
    CHECK(reached == want, "i=%llu reached=%llu want=%llu", (unsigned long long)i, (unsigned long long)reached, (unsigned long long)want);
}

static void check_n(uint64_t n, bool every_coefficient) {
    // tiles, literally
    uint64_t tiles = 0, last = 0;
    for (uint64_t start = 0; start < n; start += T) { tiles++; last = n - start < T ? n - start : T; }
    CHECK(poly_scan_tiles(n) == tiles, "n=%llu", (unsigned long long)n);
    CHECK(poly_scan_last_tile_len(n) == last && last >= 1 && last <= T, "n=%llu", (unsigned long long)n);
    uint64_t sum = 0;
    for (uint64_t b = 0; b < tiles; b++) {
        const uint64_t len = poly_scan_tile_len(n, b);
        CHECK(len == (b + 1 < tiles ? T : last), "n=%llu b=%llu", (unsigned long long)n, (unsigned long long)b);
        sum += len;
    }
    CHECK(sum == n, "n=%llu", (unsigned long long)n);
    // chunks of the carry walk
    uint64_t chunks = 0, csum = 0;
    for (uint64_t start = 0; start < tiles; start += POLY_SCAN_CHUNK) chunks++;
    CHECK(poly_scan_chunks(tiles) == chunks, "n=%llu", (unsigned long long)n);
    for (uint64_t c = 0; c < chunks; c++) {
        const uint64_t len = poly_scan_chunk_len(tiles, c);
        CHECK(len >= 1 && len <= (uint64_t)POLY_SCAN_CHUNK && (c + 1 == chunks || len == (uint64_t)POLY_SCAN_CHUNK), "n=%llu c=%llu", (unsigned long long)n,
              (unsigned long long)c);
        csum += len;
    }
    CHECK(csum == tiles, "n=%llu", (unsigned long long)n);
    // exponents
    if (every_coefficient) {
        for (uint64_t i = 0; i < n; i++) check_exponent(i);
    } else {
        for (uint64_t b = 0; b < tiles; b += (tiles > 4096 ? tiles / 1024 : 1)) {
            check_exponent(b * T);
            if (b * T + 1 < n) check_exponent(b * T + 1);
            check_exponent(b * T + poly_scan_tile_len(n, b) - 1);
        }
        check_exponent(n - 1);
    }
    // buffers and the bound
    for (uint64_t k : {1ull, 2ull, 5ull, 65535ull, 65536ull}) {
        if (!poly_scan_total_ok(n, k)) continue;
        CHECK((u128)poly_scan_total_elems(n, k) == (u128)k * tiles, "n=%llu k=%llu", (unsigned long long)n, (unsigned long long)k);
        CHECK((u128)poly_scan_quotient_words(n, k) == (u128)8 * k * (n - 1), "n=%llu k=%llu", (unsigned long long)n, (unsigned long long)k);
        CHECK(poly_scan_value_words(k) == 8 * k, "k=%llu", (unsigned long long)k);
        // the largest word index of the quotient rows fits 64 bits with room to spare, and every row starts 32-byte aligned
        CHECK(poly_scan_quotient_words(n, k) < ((u128)1 << 36) && poly_scan_quotient_words(n, 1) % 8 == 0, "n=%llu", (unsigned long long)n);
    }
    const uint64_t kmax = 0xffffffffull / n;
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, kmax, kmax + 1, ~(uint64_t)0})
        CHECK(poly_scan_total_ok(n, k) == ((u128)n * k < ((u128)1 << 32)), "n=%llu k=%llu", (unsigned long long)n, (unsigned long long)k);
    std::printf("%llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)tiles, (unsigned long long)last, (unsigned long long)chunks);
}

int main() {
    CHECK(T == 256ull * I && (1ull << POLY_SCAN_LOG_TILE) == T && (1ull << POLY_SCAN_LOG_ITEMS) == I, "tile geometry");
    for (int s = 0; s < 8; s++) {
        CHECK((1ull << poly_scan_thread_power(s)) == I << s, "s=%d", s);
        CHECK((1ull << poly_scan_tile_power(s)) == T << s && poly_scan_tile_power(s) < POLY_SCAN_POWERS, "s=%d", s);
    }
    CHECK(!poly_scan_total_ok(1ull << 32, 1) && !poly_scan_total_ok(1, 1ull << 32) && poly_scan_total_ok(0, ~0ull), "bound edges");
    for (uint64_t n = 1; n <= 3 * T + 2; n++) check_n(n, true);
    const uint64_t edge = (uint64_t)POLY_SCAN_CHUNK * T;
    for (uint64_t n : {edge - 1, edge, edge + 1, 2 * edge + 1, (uint64_t)0xffffffffull}) check_n(n, false);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_poly_scan_plan ok\n");
    return 0;
}
