// host_msm_batch_table_plan.cpp -- the pass arithmetic of the tabled batch pass, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// Over a window table a member of a batch has n * W entries but ONE bucket set of NB = 2^(c-1) buckets
// (playsnark_amd/csrc/msm_batch_plan.hpp, BatchShape::table; msm_batch_multi_plan.hpp adds the stride limit).  On a grid of
// n in 1..2^26 - 1, K in 1..2^16, the table windows c in {8, 9, 10, 13, 16, 20}, full-width and 64-bit scalars, both groups'
// point sizes and chunk limits 0, 1, 2, 7:
//   * every pass respects the five tabled limits (buckets Kc NB, entries Kc n W, bytes Kc (NB + 2 slices) point_bytes, sets
//     Kc, chunk), evaluated here from the pass's own count in 128-bit integers;
//   * one more member in the largest pass would break one of them;
//   * the passes partition 0..K in order, full passes first, also under a stride (batch_multi_passes);
//   * the five-value initialiser BatchShape{n, W, NB, point_bytes, min_slice} is still the plain shape: it yields the pass
//     sizes of the plain limits (buckets Kc W NB, sets Kc W), written out here as they stood before the field was added.
// Prints "n W NB point_bytes min_slice chunk kc_tabled kc_plain" per shape for tests/test_msm_batch_table_plan_host.py, which
// derives both counts again.
#include <cstdio>
#include <vector>

#include "../playsnark_amd/csrc/msm_batch_multi_plan.hpp"

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
// the limits written out independently of the header's own arithmetic; `tabled` chooses the products, not the shape's field
static bool pass_ok(const BatchShape& s, const BatchLimits& l, uint64_t kc, bool tabled) {
    const u128 k = kc;
    const u128 member_buckets = tabled ? (u128)s.NB : (u128)s.W * s.NB;
    const u128 member_sets = tabled ? (u128)1 : (u128)s.W;
    if (k * member_buckets > l.max_buckets) return false;
    if (k * s.n * s.W >= l.max_entries) return false;
    if (k * member_sets > l.max_sets) return false;
    const u128 slices_per_member = ((u128)s.n * s.W + s.min_slice - 1) / s.min_slice;
    if ((k * member_buckets + 2 * k * slices_per_member) * s.point_bytes > l.max_bytes) return false;
    if (l.chunk && kc > l.chunk) return false;
    return true;
}

static void check_passes(const char* what, bool ok, uint64_t kc, uint64_t K, const BatchShape& s, const BatchLimits& l, bool tabled,
                         const std::vector<BatchPass>& passes) {
    CHECK(ok == (kc != 0), "%s n %llu NB %llu K %llu: fit reported wrongly", what, (unsigned long long)s.n, (unsigned long long)s.NB, (unsigned long long)K);
    if (!ok) { CHECK(passes.empty(), "%s: passes listed for a batch that does not fit", what); return; }
    uint64_t next = 0;
    for (const BatchPass& p : passes) {
        CHECK(p.first == next && p.count > 0, "%s n %llu K %llu: passes out of order or empty", what, (unsigned long long)s.n, (unsigned long long)K);
        CHECK(pass_ok(s, l, p.count, tabled), "%s n %llu NB %llu K %llu: a pass of %llu breaks a limit", what, (unsigned long long)s.n,
              (unsigned long long)s.NB, (unsigned long long)K, (unsigned long long)p.count);
        next = p.first + p.count;
    }
    CHECK(next == K, "%s n %llu K %llu: the passes cover %llu members", what, (unsigned long long)s.n, (unsigned long long)K, (unsigned long long)next);
    CHECK(passes.size() == (K + kc - 1) / kc, "%s: full passes first", what);
}

int main() {
    const uint64_t ns[] = {1, 2, 3, 63, 64, 65, 512, 1023, 1026, 4096, 65536, 70000, 1u << 20, (1u << 22) + 5, 1u << 24, (1u << 26) - 1};
    const uint64_t Ks[] = {1, 2, 3, 5, 17, 33, 64, 255, 256, 1000, 4096, 65535, 65536};
    const uint64_t chunks[] = {0, 1, 2, 7};
    const uint64_t pbs[] = {224, 448};
    const int bitss[] = {255, 64};
    const int cs[] = {8, 9, 10, 13, 16, 20};
    std::vector<BatchPass> passes;
    long shapes = 0, unfit = 0, wider = 0;
    for (uint64_t n : ns)
        for (int c : cs)
            for (int bits : bitss)
                for (uint64_t pb : pbs)
                    for (uint64_t chunk : chunks) {
                        const BatchShape tab{n, (uint64_t)(bits / c + 1), 1ull << (c - 1), pb, 2, 1};
                        const BatchShape plain{n, (uint64_t)(bits / c + 1), 1ull << (c - 1), pb, 2};  // as every caller wrote it before
                        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, chunk};
                        CHECK(plain.table == 0, "the five-value initialiser leaves the shape plain");
                        const uint64_t kc = batch_pass_members(tab, l), kp = batch_pass_members(plain, l);
                        std::printf("%llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)tab.W,
                                    (unsigned long long)tab.NB, (unsigned long long)pb, (unsigned long long)tab.min_slice,
                                    (unsigned long long)chunk, (unsigned long long)kc, (unsigned long long)kp);
                        shapes++;
                        if (kc) {
                            CHECK(pass_ok(tab, l, kc, true), "n %llu c %d: the largest tabled pass breaks a limit", (unsigned long long)n, c);
                            CHECK(!pass_ok(tab, l, kc + 1, true), "n %llu c %d: a larger tabled pass would have fitted", (unsigned long long)n, c);
                        } else {
                            unfit++;
                            CHECK(!pass_ok(tab, l, 1, true), "n %llu c %d: one tabled member fits, none was allowed", (unsigned long long)n, c);
                        }
                        if (kp) {
                            CHECK(pass_ok(plain, l, kp, false), "n %llu c %d: the largest plain pass breaks a limit", (unsigned long long)n, c);
                            CHECK(!pass_ok(plain, l, kp + 1, false), "n %llu c %d: a larger plain pass would have fitted", (unsigned long long)n, c);
                        } else {
                            CHECK(!pass_ok(plain, l, 1, false), "n %llu c %d: one plain member fits, none was allowed", (unsigned long long)n, c);
                        }
                        CHECK(kc >= kp, "n %llu c %d: a tabled member is never larger than a plain one", (unsigned long long)n, c);
                        wider += kc > kp;
                        for (uint64_t K : Ks) {
                            check_passes("tabled", batch_passes(K, tab, l, &passes), kc, K, tab, l, true, passes);
                            check_passes("plain", batch_passes(K, plain, l, &passes), kp, K, plain, l, false, passes);
                            // under a stride (ps_msm_batch_multi): (Kc - 1) * stride + n - 1 < 2^32 on top of the five limits
                            const uint64_t stride = n + 9;
                            const bool ok = batch_multi_passes(K, tab, l, stride, &passes);
                            const uint64_t km = batch_multi_members(tab, l, stride);
                            CHECK(km <= kc, "the stride limit only shortens a pass");
                            check_passes("strided", ok, km, K, tab, l, true, passes);
                            for (const BatchPass& p : passes)
                                CHECK((u128)(p.count - 1) * stride + n - 1 < ((u128)1 << 32), "n %llu: a strided pass of %llu reads past 2^32 scalars",
                                      (unsigned long long)n, (unsigned long long)p.count);
                        }
                    }
    CHECK(unfit > 0 && unfit < shapes, "the grid should hold shapes of both kinds (%ld of %ld do not fit)", unfit, shapes);
    CHECK(wider > 0, "some tabled pass should hold more members than the plain one");
    {
        const BatchLimits l{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, 0};
        // a 16-bit table, n = 64, K = 33: 32 members of 2^15 buckets fill the sort's bucket keys, then one more pass of 1
        const BatchShape t16{64, 16, 1u << 15, 224, 2, 1};
        CHECK(batch_passes(33, t16, l, &passes) && passes.size() == 2 && passes[0].count == 32 && passes[1].first == 32 && passes[1].count == 1,
              "16-bit table, K = 33");
        // a 20-bit table, K = 3: passes of 2 and 1; the same window as a plain shape (13 * 2^19 buckets per member) fits no pass
        const BatchShape t20{64, 13, 1u << 19, 224, 2, 1};
        CHECK(batch_passes(3, t20, l, &passes) && passes.size() == 2 && passes[0].count == 2 && passes[1].count == 1, "20-bit table, K = 3");
        const BatchShape p20{64, 13, 1u << 19, 224, 2};
        CHECK(!batch_passes(3, p20, l, &passes) && passes.empty(), "a plain member of 13 * 2^19 buckets");
        // a 22-bit table: 2^21 buckets, not even one member fits -- the caller falls back to the plain route
        const BatchShape t22{64, 12, 1u << 21, 224, 2, 1};
        CHECK(batch_pass_members(t22, l) == 0 && !batch_passes(1, t22, l, &passes), "a 22-bit table fits no pass");
        // set_chunk(2), K = 5: passes of 2, 2 and 1
        const BatchLimits l2{1ull << 20, 1ull << 31, 4ull << 30, 1ull << 16, 2};
        const BatchShape small{65, 20, 1u << 12, 224, 2, 1};
        CHECK(batch_passes(5, small, l2, &passes) && passes.size() == 3 && passes[0].count == 2 && passes[1].count == 2 && passes[2].count == 1 &&
                  passes[2].first == 4, "chunk 2, K = 5");
        CHECK(batch_passes(0, t22, l, &passes) && passes.empty(), "K = 0 of a shape that does not fit");
        const BatchShape zero{0, 16, 8, 224, 2, 1};
        CHECK(batch_pass_members(zero, l) == 0, "n = 0");
    }
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("host_msm_batch_table_plan ok\n");
    return 0;
}
