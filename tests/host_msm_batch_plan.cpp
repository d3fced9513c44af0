// host_msm_batch_plan.cpp -- the pass arithmetic of ps_msm_batch, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/msm_batch_plan.hpp says how many of the K members of a batch (K scalar vectors of n scalars each, W
// windows of NB = 2^(c-1) buckets) run as one pass.  On a grid of n in 1..2^26, K in 1..2^16, c in 4..16, full-width and
// 64-bit scalars, both groups' point sizes and chunk limits 0, 1, 2, 7:
//   * every pass respects all five limits (buckets, entries, bytes, sets, chunk), evaluated here from the pass's own count;
//   * one more member in the largest pass would break one of them (the passes are as large as allowed);
//   * the passes partition 0..K in order;
//   * K = 0 gives no pass and success; a member too large for any pass (n * W >= 2^31, or W * NB over the sort's buckets) is
//     reported as such, with no pass.
// Prints "n W NB point_bytes min_slice chunk kc" per shape for tests/test_msm_batch_plan_host.py, which derives kc again.
#include <cstdio>
#include <vector>

#ifndef MSM_BATCH_PLAN_HEADER
#define MSM_BATCH_PLAN_HEADER "../playsnark_amd/csrc/msm_batch_plan.hpp"
#endif
#include MSM_BATCH_PLAN_HEADER

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

// the five limits, written out independently of the header's own arithmetic (128-bit: no product may wrap)
typedef unsigned __int128 u128;
static bool pass_ok(const BatchShape& s, const BatchLimits& l, uint64_t kc) {
    const u128 k = kc;
    if (k * s.W * s.NB > l.max_buckets) return false;
    if (k * s.n * s.W >= l.max_entries) return false;
    if (k * s.W > l.max_sets) return false;
    const u128 slices_per_member = ((u128)s.n * s.W + s.min_slice - 1) / s.min_slice;
    if ((k * s.W * s.NB + 2 * k * slices_per_member) * s.point_bytes > l.max_bytes) return false;
    if (l.chunk && kc > l.chunk) return false;
    return true;
}

int main() {
    const uint64_t ns[] = {1, 2, 3, 63, 64, 65, 1000, 4096, 65536, 70000, 1u << 20, (1u << 22) + 5, 1u << 24, (1u << 25) - 1, 1u << 26};
    const uint64_t Ks[] = {1, 2, 3, 5, 17, 64, 255, 256, 1000, 4096, 65535, 65536};
    const uint64_t chunks[] = {0, 1, 2, 7};
    const uint64_t pbs[] = {224, 448};
    const int bitss[] = {255, 64};
    std::vector<BatchPass> passes;
    long shapes = 0, unfit = 0;
    for (uint64_t n : ns)
        for (int c = 4; c <= 16; c++)
            for (int bits : bitss)
                for (uint64_t pb : pbs)
                    for (uint64_t chunk : chunks) {
                        const BatchShape s{n, (uint64_t)(bits / c + 1), 1ull << (c - 1), pb, 2};
                        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, chunk};
                        const uint64_t kc = batch_pass_members(s, l);
                        std::printf("%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)s.n, (unsigned long long)s.W,
                                    (unsigned long long)s.NB, (unsigned long long)pb, (unsigned long long)s.min_slice,
                                    (unsigned long long)chunk, (unsigned long long)kc);
                        shapes++;
                        if (kc) {
                            CHECK(pass_ok(s, l, kc), "n %llu c %d: the largest pass breaks a limit", (unsigned long long)n, c);
                            CHECK(!pass_ok(s, l, kc + 1), "n %llu c %d: a larger pass would have fitted", (unsigned long long)n, c);
                        } else {
                            unfit++;
                            CHECK(!pass_ok(s, l, 1), "n %llu c %d: one member fits, none was allowed", (unsigned long long)n, c);
                        }
                        for (uint64_t K : Ks) {
                            const bool ok = batch_passes(K, s, l, &passes);
                            CHECK(ok == (kc != 0), "n %llu c %d K %llu: fit reported wrongly", (unsigned long long)n, c, (unsigned long long)K);
                            if (!ok) { CHECK(passes.empty(), "passes listed for a batch that does not fit"); continue; }
                            uint64_t next = 0;
                            for (const BatchPass& p : passes) {
                                CHECK(p.first == next && p.count > 0, "n %llu c %d K %llu: passes out of order or empty", (unsigned long long)n, c, (unsigned long long)K);
                                CHECK(pass_ok(s, l, p.count), "n %llu c %d K %llu: a pass of %llu breaks a limit", (unsigned long long)n, c,
                                      (unsigned long long)K, (unsigned long long)p.count);
                                next = p.first + p.count;
                            }
                            CHECK(next == K, "n %llu c %d K %llu: the passes cover %llu members", (unsigned long long)n, c, (unsigned long long)K, (unsigned long long)next);
                            CHECK(passes.size() == (K + kc - 1) / kc, "full passes first");
                        }
                    }
    CHECK(unfit > 0 && unfit < shapes, "the grid should hold shapes of both kinds (%ld of %ld do not fit)", unfit, shapes);
    {   // K = 0: success and nothing to do, whatever the shape
        const BatchShape s{1000, 16, 1u << 15, 224, 2};
        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, 0};
        CHECK(batch_passes(0, s, l, &passes) && passes.empty(), "K = 0");
        const BatchShape huge{1ull << 26, 64, 8, 224, 2};  // n * W = 2^32 digits: no pass holds one member
        CHECK(!batch_passes(0 + 1, huge, l, &passes) && passes.empty(), "a member of 2^32 digits");
        CHECK(batch_passes(0, huge, l, &passes) && passes.empty(), "K = 0 of a shape that does not fit");
        const BatchShape wide{1000, 13, 1u << 19, 224, 2};  // a forced 20-bit window: 13 * 2^19 buckets per member
        CHECK(!batch_passes(3, wide, l, &passes) && passes.empty(), "a member of more buckets than the sort takes");
        // set_chunk(2), K = 5: passes of 2, 2 and 1
        const BatchLimits l2{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, 2};
        const BatchShape small{65, 32, 128, 224, 2};
        CHECK(batch_passes(5, small, l2, &passes) && passes.size() == 3 && passes[0].count == 2 && passes[1].count == 2 && passes[2].count == 1 &&
                  passes[2].first == 4, "chunk 2, K = 5");
        // degenerate shapes do not divide by zero
        const BatchShape zero{0, 16, 8, 224, 2};
        CHECK(batch_pass_members(zero, l) == 0, "n = 0");
    }
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("host_msm_batch_plan ok\n");
    return 0;
}
