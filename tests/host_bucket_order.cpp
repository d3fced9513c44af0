// host_bucket_order.cpp -- the buckets of a sum in order of size, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// The whole-bucket point pass (msm.hpp section 4b) gives bucket perm[t] to logical thread t, so it is correct only if perm[] is
// a permutation of 0 .. G-1 (every bucket has exactly one writer), and it is fast only if the sizes do not increase along it.
// This file compiles the index arithmetic the three ordering kernels are built from (playsnark_amd/csrc/bucket_order.hpp:
// bo_class, bo_scan_desc, bo_verdict) and runs it, in the roles of k_bo_count / k_bo_scan / k_bo_place -- tiles of
// BO_PLACE_TILE buckets, one cursor reservation per (tile, class) -- over generated offs[] arrays.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../playsnark_amd/csrc/bucket_order.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) {                                                  \
                std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                                  \
                std::fprintf(stderr, "\n");                                         \
            }                                                                       \
        }                                                                           \
    } while (0)

static unsigned long long rng_state = 0x6275636b65746f72ull;
static unsigned long long rnd() {  // splitmix64
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static std::vector<u32> offs_of(const std::vector<u32>& sizes) {
    std::vector<u32> offs(sizes.size() + 1, 0);
    for (size_t g = 0; g < sizes.size(); g++) offs[g + 1] = offs[g] + sizes[g];
    return offs;
}

static long cases_run = 0, seen_even = 0, seen_uneven = 0, seen_capped = 0;

// tile_order: the order in which the place kernel's workgroups reach their cursor reservations (any order must do)
static void run_case(const char* what, const std::vector<u32>& offs, int tile_order) {
    const u32 G = (u32)offs.size() - 1, E = offs[G];
    cases_run++;
    // k_bo_count: per-tile histograms added into the global one
    std::vector<u32> hist(BO_CLASSES, 0);
    const u32 tiles = (G + BO_PLACE_TILE - 1) / BO_PLACE_TILE;
    for (u32 b = 0; b < tiles; b++) {
        u32 lh[BO_CLASSES] = {0};
        for (u32 g = b * BO_PLACE_TILE; g < std::min(G, (b + 1) * BO_PLACE_TILE); g++) lh[bo_class(offs[g], offs[g + 1])]++;
        for (u32 k = 0; k < BO_CLASSES; k++) hist[k] += lh[k];
    }
    // k_bo_scan
    std::vector<u32> cursors(BO_CLASSES, 0);
    const u32 maxc = bo_scan_desc(hist.data(), cursors.data());
    const u32 nonempty = G - hist[0];
    const u32 verdict = bo_verdict(maxc, nonempty, E);
    const std::vector<u32> start = cursors;
    // k_bo_place
    std::vector<u32> perm(G, 0xffffffffu);
    std::vector<u32> order(tiles);
    for (u32 b = 0; b < tiles; b++) order[b] = tile_order == 0 ? b : tile_order == 1 ? tiles - 1 - b : b;
    if (tile_order == 2)
        for (u32 b = tiles; b > 1; b--) std::swap(order[b - 1], order[rnd() % b]);
    for (u32 b : order) {
        u32 lh[BO_CLASSES] = {0}, base[BO_CLASSES];
        const u32 g0 = b * BO_PLACE_TILE, g1 = std::min(G, g0 + BO_PLACE_TILE);
        for (u32 g = g0; g < g1; g++) lh[bo_class(offs[g], offs[g + 1])]++;
        for (u32 k = 0; k < BO_CLASSES; k++) { base[k] = cursors[k]; cursors[k] += lh[k]; }
        for (u32 g = g1; g-- > g0;) {  // ranks inside the run in no particular order: here, backwards
            const u32 k = bo_class(offs[g], offs[g + 1]);
            const u32 pos = base[k]++;
            CHECK(pos < G, "%s: position %u outside perm[%u]", what, pos, G);
            if (pos < G) {
                CHECK(perm[pos] == 0xffffffffu, "%s: position %u written twice", what, pos);
                perm[pos] = g;
            }
        }
    }

    // perm is a permutation of 0 .. G-1
    std::vector<int> seen(G, 0);
    for (u32 t = 0; t < G; t++) {
        CHECK(perm[t] < G, "%s: perm[%u] = %u", what, t, perm[t]);
        if (perm[t] < G) seen[perm[t]]++;
    }
    for (u32 g = 0; g < G; g++) CHECK(seen[g] == 1, "%s: bucket %u appears %d times", what, g, seen[g]);
    // size classes do not increase along it; sizes of BO_CLASSES - 1 and more all sit in the first class
    u32 big = 0;
    for (u32 g = 0; g < G; g++) big += offs[g + 1] - offs[g] >= BO_CLASSES - 1;
    for (u32 t = 0; t < G; t++) {
        if (perm[t] >= G) continue;
        const u32 g = perm[t], k = bo_class(offs[g], offs[g + 1]);
        if (t + 1 < G && perm[t + 1] < G) {
            const u32 gn = perm[t + 1];
            CHECK(k >= bo_class(offs[gn], offs[gn + 1]), "%s: class grows at position %u", what, t);
        }
        CHECK((offs[g + 1] - offs[g] >= BO_CLASSES - 1) == (t < big), "%s: bucket %u of %u entries at position %u, %u big buckets", what, g,
              offs[g + 1] - offs[g], t, big);
        CHECK(start[k] <= t && t < start[k] + hist[k], "%s: position %u outside the run of class %u", what, t, k);
    }
    if (big) seen_capped++;

    // the verdict against a direct computation
    u32 dmax = 0, dnon = 0;
    for (u32 g = 0; g < G; g++) {
        const u32 s = offs[g + 1] - offs[g];
        dmax = std::max(dmax, s);
        dnon += s != 0;
    }
    CHECK(nonempty == dnon, "%s: %u non-empty buckets, %u counted", what, dnon, nonempty);
    CHECK(maxc == std::min(dmax, BO_CLASSES - 1), "%s: largest class %u, largest bucket %u", what, maxc, dmax);
    const bool even = dnon > 0 && dmax < BO_CLASSES - 1 && (double)dmax <= (double)BO_EVEN_MULT * E / dnon + BO_EVEN_ADD;
    CHECK(verdict == (even ? (u32)ACC_BUCKETS : (u32)ACC_SLICES), "%s: verdict %u, largest %u of %u entries in %u buckets", what, verdict, dmax, E, dnon);
    (even ? seen_even : seen_uneven)++;
}

static void run_all(const char* what, const std::vector<u32>& sizes) {
    const std::vector<u32> offs = offs_of(sizes);
    for (int order = 0; order < 3; order++) run_case(what, offs, order);
}

int main() {
    // G around the tile and the workgroup sizes, and not a multiple of either
    for (u32 G : {1u, 2u, 63u, 255u, 256u, 257u, BO_PLACE_TILE - 1, BO_PLACE_TILE, BO_PLACE_TILE + 1, 3 * BO_PLACE_TILE + 77, 5000u}) {
        run_all("all empty", std::vector<u32>(G, 0));
        run_all("all of size 1", std::vector<u32>(G, 1));
        for (u32 at : {0u, G / 2, G - 1}) {
            std::vector<u32> one(G, 0);
            one[at] = 1;
            run_all("one entry in all", one);
            one[at] = 100000;
            run_all("one bucket holds everything", one);
            std::vector<u32> skew(G, 3);
            skew[at] = 254;  // the largest size with a class of its own: uneven by the bound, not by the cap
            run_all("one large bucket among small ones", skew);
        }
        {
            std::vector<u32> mixed(G);
            for (u32 g = 0; g < G; g++) mixed[g] = (u32)(rnd() % 301);  // 0 .. 300: both sides of the cap
            run_all("sizes 0..300", mixed);
        }
        {
            std::vector<u32> poisson(G);  // an evenly filled sum: sizes near 26
            for (u32 g = 0; g < G; g++) {
                u32 s = 0;
                for (int j = 0; j < 52; j++) s += (u32)(rnd() & 1);
                poisson[g] = s;
            }
            run_all("even fill", poisson);
            poisson[G / 3] = 26 * 4 + 32 + 40;  // beyond 4 x mean + 32 whatever the draw
            run_all("even fill with one outlier", poisson);
        }
        {
            std::vector<u32> edge(G, 10);  // the bound itself: mean 10 + a little, largest 72 / 73
            edge[0] = 72;
            run_all("at the bound", edge);
            edge[0] = 73 + 4 * 73 / G;
            run_all("past the bound", edge);
        }
    }
    CHECK(seen_even > 0 && seen_uneven > 0 && seen_capped > 0, "verdicts even %ld, uneven %ld, capped cases %ld", seen_even, seen_uneven, seen_capped);
    std::printf("%ld cases, verdict even %ld / uneven %ld, %ld with buckets in the capped class\n", cases_run, seen_even, seen_uneven, seen_capped);
    if (failures) {
        std::printf("host_bucket_order: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("host_bucket_order ok\n");
    return 0;
}
