// host_msm_batch_multi_plan.cpp -- the pass arithmetic of ps_msm_batch_multi, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/msm_batch_multi_plan.hpp adds two conditions to the passes of ps_msm_batch (msm_batch_plan.hpp): the
// point size of the largest group present, and the member stride, which bounds the 32-bit scalar index of
// k_sort_count_batch.  On a grid of n in 1..2^26, c in 4..16, full-width and 64-bit scalars, the three group mixes, chunk
// limits 0 and 7, and strides n, n + 9, 4 n + 3, 2^20, 2^31 + 7 and 2^33 (where at least n):
//   * every pass respects the five limits of ps_msm_batch, evaluated with the mixed point size, and the stride limit
//     (count - 1) * stride + n - 1 < 2^32, all written out here in 128-bit arithmetic;
//   * one more member in the largest pass would break one of them;
//   * the passes partition 0..K in order, full passes first;
//   * a packed batch (stride == n) gets exactly the passes of batch_passes: ps_msm_batch loses nothing to the stride limit;
//   * a stride below n, K = 0 and a member too large for any pass are reported as ps_msm_batch_multi expects them.
// Prints "n W NB point_bytes chunk stride kc" per shape for tests/test_msm_batch_multi_plan_host.py, which derives kc again.
#include <cstdio>
#include <vector>

#ifndef MSM_BATCH_MULTI_PLAN_HEADER
#define MSM_BATCH_MULTI_PLAN_HEADER "../playsnark_amd/csrc/msm_batch_multi_plan.hpp"
#endif
#include MSM_BATCH_MULTI_PLAN_HEADER

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
// the limits, written out independently of the headers' own arithmetic (128-bit: no product may wrap)
static bool pass_ok(const BatchShape& s, const BatchLimits& l, uint64_t stride, uint64_t kc) {
    const u128 k = kc;
    if (kc == 0) return false;
    if (k * s.W * s.NB > l.max_buckets) return false;
    if (k * s.n * s.W >= l.max_entries) return false;
    if (k * s.W > l.max_sets) return false;
    const u128 slices_per_member = ((u128)s.n * s.W + s.min_slice - 1) / s.min_slice;
    if ((k * s.W * s.NB + 2 * k * slices_per_member) * s.point_bytes > l.max_bytes) return false;
    if (l.chunk && kc > l.chunk) return false;
    if ((k - 1) * stride + s.n - 1 >= ((u128)1 << 32)) return false;  // the last scalar index of the pass
    return true;
}

int main() {
    const uint64_t ns[] = {1, 2, 3, 63, 64, 65, 1000, 4096, 65536, 70000, 1u << 20, (1u << 22) + 5, 1u << 24, (1u << 25) - 1, 1u << 26};
    const uint64_t Ks[] = {1, 2, 3, 5, 17, 64, 255, 256, 1000, 4096, 65535, 65536};
    const uint64_t chunks[] = {0, 7};
    const bool mixes[][2] = {{true, false}, {false, true}, {true, true}};
    const int bitss[] = {255, 64};
    std::vector<BatchPass> passes, packed;
    long shapes = 0, unfit = 0, stride_bound = 0;
    CHECK(batch_multi_point_bytes(true, false, 224, 448) == 224 && batch_multi_point_bytes(false, true, 224, 448) == 448 &&
              batch_multi_point_bytes(true, true, 224, 448) == 448 && batch_multi_point_bytes(false, false, 224, 448) == 0,
          "point size of a mix");
    for (uint64_t n : ns)
        for (int c = 4; c <= 16; c++)
            for (int bits : bitss)
                for (auto& mix : mixes)
                    for (uint64_t chunk : chunks) {
                        const uint64_t pb = batch_multi_point_bytes(mix[0], mix[1], 224, 448);
                        const BatchShape s{n, (uint64_t)(bits / c + 1), 1ull << (c - 1), pb, 2};
                        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, chunk};
                        const uint64_t strides[] = {n, n + 9, 4 * n + 3, 1ull << 20, (1ull << 31) + 7, 1ull << 33};
                        for (uint64_t stride : strides) {
                            if (stride < n) continue;
                            const uint64_t kc = batch_multi_members(s, l, stride);
                            std::printf("%llu %llu %llu %llu %llu %llu %llu\n", (ull)s.n, (ull)s.W, (ull)s.NB, (ull)pb, (ull)chunk, (ull)stride, (ull)kc);
                            shapes++;
                            if (kc) {
                                CHECK(pass_ok(s, l, stride, kc), "n %llu c %d stride %llu: the largest pass breaks a limit", (ull)n, c, (ull)stride);
                                CHECK(!pass_ok(s, l, stride, kc + 1), "n %llu c %d stride %llu: a larger pass would have fitted", (ull)n, c, (ull)stride);
                                if (kc < batch_pass_members(s, l)) stride_bound++;
                            } else {
                                unfit++;
                                CHECK(!pass_ok(s, l, stride, 1), "n %llu c %d stride %llu: one member fits, none was allowed", (ull)n, c, (ull)stride);
                            }
                            if (stride == n) CHECK(kc == batch_pass_members(s, l), "n %llu c %d: the stride limit shortens a packed pass", (ull)n, c);
                            for (uint64_t K : Ks) {
                                const bool ok = batch_multi_passes(K, s, l, stride, &passes);
                                CHECK(ok == (kc != 0), "n %llu c %d K %llu: fit reported wrongly", (ull)n, c, (ull)K);
                                if (!ok) { CHECK(passes.empty(), "passes listed for a batch that does not fit"); continue; }
                                uint64_t next = 0;
                                for (const BatchPass& p : passes) {
                                    CHECK(p.first == next && p.count > 0, "n %llu c %d K %llu: passes out of order or empty", (ull)n, c, (ull)K);
                                    CHECK(pass_ok(s, l, stride, p.count), "n %llu c %d K %llu: a pass of %llu breaks a limit", (ull)n, c, (ull)K, (ull)p.count);
                                    next = p.first + p.count;
                                }
                                CHECK(next == K, "n %llu c %d K %llu: the passes cover %llu members", (ull)n, c, (ull)K, (ull)next);
                                CHECK(passes.size() == (K + kc - 1) / kc, "full passes first");
                                if (stride == n) {
                                    CHECK(batch_passes(K, s, l, &packed) && packed.size() == passes.size(), "packed: as batch_passes");
                                    for (size_t i = 0; i < passes.size() && i < packed.size(); i++)
                                        CHECK(packed[i].first == passes[i].first && packed[i].count == passes[i].count, "packed: as batch_passes");
                                }
                            }
                        }
                    }
    CHECK(unfit > 0 && unfit < shapes, "the grid should hold shapes of both kinds (%ld of %ld do not fit)", unfit, shapes);
    CHECK(stride_bound > 0, "the grid should hold passes that the stride alone shortens");
    {
        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, 0};
        const BatchShape s{1000, 16, 1u << 15, 448, 2};
        CHECK(batch_multi_passes(0, s, l, 1000, &passes) && passes.empty(), "K = 0");
        CHECK(batch_multi_members(s, l, 999) == 0, "a stride below n holds no member");
        CHECK(!batch_multi_passes(3, s, l, 999, &passes) && passes.empty(), "a stride below n");
        CHECK(batch_multi_members(s, l, 1ull << 40) == 1, "a huge stride: one member per pass, its own scalars start at index 0");
        CHECK(batch_multi_passes(3, s, l, 1ull << 40, &passes) && passes.size() == 3, "a huge stride, K = 3");
        const BatchShape huge{1ull << 26, 64, 8, 224, 2};  // n * W = 2^32 digits: no pass holds one member
        CHECK(!batch_multi_passes(1, huge, l, 1ull << 26, &passes) && passes.empty(), "a member of 2^32 digits");
        const BatchShape wide{1000, 15, 1u << 17, 224, 2};  // a forced 18-bit window: 15 * 2^17 buckets per member
        CHECK(!batch_multi_passes(3, wide, l, 1000, &passes) && passes.empty(), "a member of more buckets than the sort takes");
        // a PHGR13 batch: m = 2^16 + 3 variables, the seven arrays over the last 2^16 of them, G2 present
        const BatchShape ph{1u << 16, 16, 1u << 15, 448, 2};
        CHECK(batch_multi_members(ph, l, (1u << 16) + 3) == batch_pass_members(ph, l), "a witness stride does not shorten the passes");
        const BatchShape zero{0, 16, 8, 224, 2};
        CHECK(batch_multi_members(zero, l, 5) == 0, "n = 0");
    }
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("host_msm_batch_multi_plan ok\n");
    return 0;
}
