// host_fr_lincomb_plan.cpp -- the index arithmetic of the linear combination of scalar vectors (ps_scalars_lincomb), checked on
// the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/fr_lincomb_plan.hpp says how t rows fall into groups of R, the groups into launches of 65 535, N indices
// into workgroups of 256, where entry (l, j) of the coefficient table and element (j, i) of the output lie, behind which inputs
// the accumulators are reduced and when a call is too large.  Against literal loops:
//   * for t = 1 .. 4R + 3 and the launch edges 65 535 R - 1 .. 65 535 R + 1, 2 * 65 535 R + 1, 2^20: group count, the rows of every
//     group (they add up to t, only the last is partial), launch count and the groups of every launch (they add up to the groups,
//     none above 65 535), and that (launch, blockIdx.y, r) -- as the kernel forms its row -- meets every row exactly once;
//   * for N = 1 .. 3 * 256 + 2 and 2^32 - 1: the workgroup count, and that it covers N with less than one workgroup to spare;
//   * table and output layout on a small shape, written through into real arrays (ASan watches the bounds): every entry and
//     every element is met exactly once, rows start 32-byte aligned;
//   * the reduction step: never more than 32 inputs between two reductions, for m up to 200;
//   * the size limits at their edges, in 128-bit arithmetic.
// Prints "t groups last launches" per t for tests/test_fr_lincomb_plan_host.py, which derives the three again.
#include <cstdio>
#include <vector>

#ifndef FR_LINCOMB_PLAN_HEADER
#define FR_LINCOMB_PLAN_HEADER "../playsnark_amd/csrc/fr_lincomb_plan.hpp"
#endif
#include FR_LINCOMB_PLAN_HEADER

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
static const uint64_t R = FR_LINCOMB_ROWS, Y = FR_LINCOMB_MAX_GROUPS_PER_LAUNCH;

static void check_t(uint64_t t, bool every_row) {
    uint64_t groups = 0, last = 0;
    for (uint64_t start = 0; start < t; start += R) { groups++; last = t - start < R ? t - start : R; }
    CHECK(fr_lincomb_groups(t) == groups, "t=%llu", (ull)t);
    uint64_t sum = 0;
    for (uint64_t g = 0; g < groups; g += (every_row ? 1 : 1 + groups / 4096)) {
        const uint64_t rows = fr_lincomb_group_rows(t, g);
        CHECK(rows == (g + 1 < groups ? R : last) && rows >= 1, "t=%llu g=%llu", (ull)t, (ull)g);
        sum += rows;
    }
    CHECK(fr_lincomb_group_rows(t, groups - 1) == last, "t=%llu", (ull)t);
    if (every_row) CHECK(sum == t, "t=%llu", (ull)t);
    uint64_t launches = 0, gsum = 0;
    for (uint64_t start = 0; start < groups; start += Y) launches++;
    CHECK(fr_lincomb_launches(groups) == launches, "t=%llu", (ull)t);
    std::vector<unsigned char> met(every_row ? t : 0, 0);
    for (uint64_t k = 0; k < launches; k++) {
        const uint64_t len = fr_lincomb_launch_groups(groups, k);
        CHECK(len >= 1 && len <= Y && (k + 1 == launches || len == Y), "t=%llu k=%llu", (ull)t, (ull)k);
        gsum += len;
        if (!every_row) continue;
        const uint64_t g0 = k * Y;  // the kernel's argument
        for (uint64_t y = 0; y < len; y++)
            for (uint64_t r = 0; r < R; r++) {
                const uint64_t j = (g0 + y) * R + r;  // as the kernel forms it, in 32 bits
                CHECK(j <= 0xffffffffull, "t=%llu", (ull)t);
                if (j < t) met[j]++;
            }
    }
    CHECK(gsum == groups, "t=%llu", (ull)t);
    for (uint64_t j = 0; j < met.size(); j++) CHECK(met[j] == 1, "t=%llu j=%llu met %d times", (ull)t, (ull)j, (int)met[j]);
    std::printf("%llu %llu %llu %llu\n", (ull)t, (ull)groups, (ull)last, (ull)launches);
}

static void check_layout(uint64_t m, uint64_t t, uint64_t N) {
    std::vector<unsigned char> table(m * t, 0);
    for (uint64_t l = 0; l < m; l++)
        for (uint64_t j = 0; j < t; j++) table[fr_lincomb_coef_index(l, j, t)]++;
    for (unsigned char c : table) CHECK(c == 1, "m=%llu t=%llu", (ull)m, (ull)t);
    std::vector<unsigned char> words(8 * t * N, 0);
    for (uint64_t j = 0; j < t; j++)
        for (uint64_t i = 0; i < N; i++) {
            const uint64_t w = fr_lincomb_out_word(j, i, N);
            CHECK(w % 8 == 0, "j=%llu i=%llu", (ull)j, (ull)i);
            for (int k = 0; k < 8; k++) words[w + k]++;
        }
    for (unsigned char c : words) CHECK(c == 1, "t=%llu N=%llu", (ull)t, (ull)N);
}

int main() {
    CHECK(FR_LINCOMB_THREADS == 256 && R >= 1 && FR_LINCOMB_REDUCE_EVERY == 32, "geometry");
    for (uint64_t t = 1; t <= 4 * R + 3; t++) check_t(t, true);
    for (uint64_t t : {Y * R - 1, Y * R, Y * R + 1, 2 * Y * R + 1}) check_t(t, true);
    check_t(1ull << 20, false);
    for (uint64_t N = 1; N <= 3 * 256 + 2; N++) {
        uint64_t blocks = 0;
        for (uint64_t s = 0; s < N; s += 256) blocks++;
        CHECK(fr_lincomb_blocks(N) == blocks, "N=%llu", (ull)N);
    }
    for (uint64_t N : {(uint64_t)0xffffffffull, (uint64_t)1 << 31, ((uint64_t)1 << 31) + 1}) {
        const uint64_t b = fr_lincomb_blocks(N);
        CHECK((u128)b * 256 >= N && (u128)(b - 1) * 256 < N && b < (1ull << 31), "N=%llu", (ull)N);
    }
    for (uint64_t m : {1, 2, 3})
        for (uint64_t t : {(uint64_t)1, R, R + 1})
            for (uint64_t N : {1, 5, 257}) check_layout(m, t, N);
    // the reduction step: runs of inputs without a reduction, literally
    uint64_t run = 0, reductions = 0;
    for (uint64_t l = 0; l < 200; l++) {
        run++;
        CHECK(run <= (uint64_t)FR_LINCOMB_REDUCE_EVERY, "l=%llu", (ull)l);
        CHECK(fr_lincomb_reduce_after(l) == (run == (uint64_t)FR_LINCOMB_REDUCE_EVERY), "l=%llu", (ull)l);
        if (fr_lincomb_reduce_after(l)) { run = 0; reductions++; }
    }
    CHECK(reductions == 200 / 32, "reductions=%llu", (ull)reductions);
    // the limits
    for (uint64_t N : {(uint64_t)1, (uint64_t)2, (uint64_t)257, (uint64_t)1 << 20, (uint64_t)0xffffffffull, (uint64_t)1 << 32, ~(uint64_t)0})
        for (uint64_t t : {(uint64_t)1, (uint64_t)2, (uint64_t)5, (uint64_t)4095, (uint64_t)4096, (uint64_t)1 << 20, ((uint64_t)1 << 20) + 1, ~(uint64_t)0})
            for (uint64_t m : {(uint64_t)1, (uint64_t)2, (uint64_t)256, (uint64_t)257, (uint64_t)1 << 20, ((uint64_t)1 << 20) + 1, ~(uint64_t)0}) {
                const bool want = (u128)t * N < ((u128)1 << 32) && (u128)m * t <= ((u128)1 << 20);
                CHECK(fr_lincomb_size_ok(m, t, N) == want, "m=%llu t=%llu N=%llu", (ull)m, (ull)t, (ull)N);
                if (want) CHECK(fr_lincomb_out_word(t - 1, N - 1, N) + 8 == (u128)8 * t * N, "t=%llu N=%llu", (ull)t, (ull)N);
            }
    CHECK(fr_lincomb_size_ok(0, 5, 5) && fr_lincomb_size_ok(5, 0, 5), "empty shapes");
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_fr_lincomb_plan ok\n");
    return 0;
}
