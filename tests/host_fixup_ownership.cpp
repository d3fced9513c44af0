// host_fixup_ownership.cpp -- who writes a bucket and who reads a partial slot, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// The bucket array of a sum is never cleared and the partial slots of the accumulation are never initialised, so the
// fix-up is correct only if
//   * every bucket is written by exactly one of: the accumulation's flush (a bucket inside one slice), the classification
//     (an empty bucket), the pair kernel (a bucket cut once), the chain kernel (chain_list), the heavy kernels (heavy_list);
//   * every partial slot the accumulation writes is read exactly once, and no slot is read that was not written.
// This file compiles the predicates the kernels are built from (playsnark_amd/csrc/fixup_class.hpp: eff_slice,
// bucket_class, part_slot, pair_boundary_bucket) and runs them, in the roles of those kernels, over generated offs[] arrays
// and slice lengths.  The accumulation's side is modelled after k_accumulate / flush_run (msm.hpp section 4).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../playsnark_amd/csrc/fixup_class.hpp"

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

static unsigned long long rng_state = 0x66697875706f776eull;
static unsigned long long rnd() {  // splitmix64
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static std::set<int> seen_M, seen_span;
static long seen_class[5] = {0, 0, 0, 0, 0};
static long cases_run = 0;

// offs[0..G] from bucket sizes
static std::vector<u32> offs_of(const std::vector<u32>& sizes) {
    std::vector<u32> offs(sizes.size() + 1, 0);
    for (size_t g = 0; g < sizes.size(); g++) offs[g + 1] = offs[g] + sizes[g];
    return offs;
}

// One sum: offs[], the planned slice length and the planned number of slices T (>= E / Mplan, as the plan's W * n digits
// are >= the non-zero ones).
static void run_case(const char* what, const std::vector<u32>& offs, int Mplan, u32 T) {
    const u32 G = (u32)offs.size() - 1, E = offs[G];
    const u32 M = (u32)eff_slice(E, T, Mplan);
    CHECK((u64)T * M >= E, "%s: %u slices of %u do not cover %u entries", what, T, M, E);
    cases_run++;
    seen_M.insert((int)M);
    std::vector<int> bucket_writes(G, 0), slot_writes(2 * (size_t)T, 0), slot_reads(2 * (size_t)T, 0);

    // the accumulation: thread t walks [t M, min(E, t M + M)) and flushes a run whenever the bucket changes
    for (u32 t = 0; t < T; t++) {
        const u64 start64 = (u64)t * M;
        if (start64 >= E) continue;
        const u32 start = (u32)start64, end = (E - start < M) ? E : start + M;
        u32 lo = 0, hi = G;
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (offs[mid] <= start) lo = mid; else hi = mid;
        }
        u32 g = lo, rs = start;
        while (rs < end) {
            while (offs[g + 1] <= rs) g++;  // next non-empty bucket
            const u32 re = offs[g + 1] < end ? offs[g + 1] : end;
            const bool whole = rs == offs[g] && re == offs[g + 1];
            if (whole) bucket_writes[g]++;
            else if (rs == start) slot_writes[2 * (size_t)t]++;
            else slot_writes[2 * (size_t)t + 1]++;
            rs = re;
        }
    }

    // the classification: one thread per bucket
    std::vector<u32> chain_list, heavy_list;
    for (u32 g = 0; g < G; g++) {
        const int cls = bucket_class(offs[g], offs[g + 1], M, HEAVY_SPAN);
        seen_class[cls]++;
        if (cls != BUCKET_EMPTY) seen_span.insert((int)((offs[g + 1] - 1) / M - offs[g] / M) + 1);
        if (cls == BUCKET_EMPTY) bucket_writes[g]++;
        else if (cls == BUCKET_CHAIN) chain_list.push_back(g);
        else if (cls == BUCKET_HEAVY) heavy_list.push_back(g);
    }
    // a bucket on chain_list holds at least one whole slice that no other bucket shares: the host sizes the list by that
    CHECK(chain_list.size() <= (size_t)T / 2 + 2, "%s: %zu chain buckets for %u slices", what, chain_list.size(), T);

    // the pair kernel: one thread per slice boundary
    for (u32 t = 1; t < T; t++) {
        u32 g = 0;
        if (!pair_boundary_bucket(offs.data(), G, E, t, M, HEAVY_SPAN, g)) continue;
        const size_t left = part_slot(offs[g], t - 1, M), right = part_slot(offs[g], t, M);
        CHECK(right == 2 * (size_t)t, "%s: the right half of a cut bucket is not a head slot", what);
        slot_reads[left]++;
        slot_reads[right]++;
        bucket_writes[g]++;
    }
    // the chain kernel and the heavy kernels: every slice the bucket touches
    for (int pass = 0; pass < 2; pass++)
        for (u32 g : pass == 0 ? chain_list : heavy_list) {
            const u32 t0 = offs[g] / M, t1 = (offs[g + 1] - 1) / M;
            CHECK(pass == 0 ? (t1 - t0 >= 2 && t1 - t0 < HEAVY_SPAN) : t1 - t0 >= HEAVY_SPAN, "%s: bucket %u on the wrong list", what, g);
            for (u32 t = t0; t <= t1; t++) slot_reads[part_slot(offs[g], t, M)]++;
            bucket_writes[g]++;
        }

    for (u32 g = 0; g < G; g++)
        CHECK(bucket_writes[g] == 1, "%s (M %u, T %u): bucket %u [%u, %u) written %d times", what, M, T, g, offs[g], offs[g + 1], bucket_writes[g]);
    for (size_t s = 0; s < 2 * (size_t)T; s++) {
        CHECK(slot_writes[s] <= 1, "%s (M %u, T %u): slot %zu written %d times", what, M, T, s, slot_writes[s]);
        CHECK(slot_reads[s] == slot_writes[s], "%s (M %u, T %u): slot %zu written %d times, read %d times", what, M, T, s, slot_writes[s], slot_reads[s]);
    }
}

// every planned M and slice count that leads to an effective slice length of 4 .. 64 for this list
static void run_all_M(const char* what, const std::vector<u32>& offs) {
    const u32 E = offs.back();
    for (int Mplan : {4, 8, 16, 32, 64}) {
        const u32 T0 = (E + Mplan - 1) / Mplan;
        // T0: the list is as long as planned; more slices planned than used: eff_slice shortens them (down to 4)
        for (u32 T : {T0, T0 + 1, 2 * T0 + 1, 4 * T0, 5 * T0 + 3, 7 * T0 + 1, 9 * T0, 16 * T0 + 5, 40 * T0})
            run_case(what, offs, Mplan, T ? T : 1u);
    }
}

int main() {
    const u32 shapes[] = {4, 5, 8, 13, 16, 32, 33, 64};
    for (u32 M : shapes) {
        // uniform fills and all-empty
        for (u32 fill : {0u, 1u, M / 2, M - 1, M, M + 1, 2 * M, 2 * M + 1, 3 * M - 1, 9 * M + 1})
            run_all_M("uniform", offs_of(std::vector<u32>(37, fill)));
        // one bucket holding everything: first, in the middle, last
        for (u32 at : {0u, 11u, 22u}) {
            for (u32 n : {1u, M - 1, M, M + 1, 8 * M, 8 * M + 1, 100 * M + 7}) {
                std::vector<u32> sizes(23, 0);
                sizes[at] = n;
                run_all_M("one bucket", offs_of(sizes));
            }
        }
        // buckets ending exactly on slice boundaries, between buckets that do not
        {
            std::vector<u32> sizes;
            for (u32 k = 1; k <= 10; k++) { sizes.push_back(k * M); sizes.push_back(0); }
            for (u32 k = 1; k <= 10; k++) { sizes.push_back(3); sizes.push_back(k * M - 3); sizes.push_back(k * M); }
            run_all_M("on boundaries", offs_of(sizes));
        }
        // spans of 2, 3, 7, 8 and 9 slices (and 10, 11: heavy), starting one entry before a boundary, on it and after it
        for (u32 lead : {M - 1, 0u, 1u}) {
            std::vector<u32> sizes;
            for (u32 span : {2u, 3u, 7u, 8u, 9u, 10u, 11u}) {
                sizes.push_back(lead ? lead : M);      // a small bucket first: the long ones start at every phase of a slice
                sizes.push_back((span - 2) * M + 2);   // started one entry before a boundary this touches exactly `span` slices
                sizes.push_back(0);
                sizes.push_back(span * M);             // `span` slices when aligned, one more when not
                sizes.push_back(2 * M - (lead + 2) % M);  // filler that moves the phase for the next round
            }
            run_all_M("spans", offs_of(sizes));
        }
        // E not a multiple of M; E < M
        for (u32 E : {1u, 2u, M - 1, M + 1, 3 * M + M / 2, 17 * M - 1}) {
            std::vector<u32> sizes;
            u32 left = E;
            while (left) {
                const u32 s = (u32)(rnd() % (left + 1));
                sizes.push_back(s);
                left -= s;
                if (rnd() & 1) sizes.push_back(0);
            }
            sizes.push_back(0);
            run_all_M("ragged end", offs_of(sizes));
        }
        // random mixes: mostly small buckets and empties, a few long ones
        for (int rep = 0; rep < 40; rep++) {
            std::vector<u32> sizes(1 + rnd() % 200);
            for (u32& s : sizes) {
                const unsigned r = (unsigned)(rnd() % 16);
                s = r < 5 ? 0u : r < 12 ? (u32)(rnd() % (2 * M)) : r < 15 ? (u32)(rnd() % (9 * M)) : (u32)(rnd() % (40 * M));
            }
            run_all_M("random", offs_of(sizes));
        }
    }
    // the cases must have reached every class, the spans around the list thresholds and the slice lengths 4 .. 64
    for (int cls = 0; cls < 5; cls++) CHECK(seen_class[cls] > 0, "class %d never occurred", cls);
    for (int span : {1, 2, 3, 7, 8, 9, 10}) CHECK(seen_span.count(span), "no bucket spanned %d slices", span);
    for (int M : {4, 5, 7, 8, 16, 32, 33, 64}) CHECK(seen_M.count(M), "no case ran with an effective slice of %d", M);
    CHECK(*seen_M.begin() >= 4 && *seen_M.rbegin() <= 64, "effective slices %d .. %d", *seen_M.begin(), *seen_M.rbegin());
    std::printf("%ld cases, %zu slice lengths, classes empty/whole/pair/chain/heavy %ld/%ld/%ld/%ld/%ld\n", cases_run, seen_M.size(),
                seen_class[0], seen_class[1], seen_class[2], seen_class[3], seen_class[4]);
    if (failures) {
        std::printf("host_fixup_ownership: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("host_fixup_ownership ok\n");
    return 0;
}
