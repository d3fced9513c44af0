// host_phgr13_locate_index.cpp -- the index arithmetic of the locating PHGR13 batch verifier's trees, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/locate_phgr13_dev.hpp says which trees a root mask needs and where a node of them lies; the host side
// (verify_phgr13_locate.inc) sizes its buffers and builds its gather indices with the functions compiled here:
//   * element_equations / element_slots: for every root mask the elements with a tree are exactly those the table of the
//     five equations reads (E0: hs, yss; E1: vass, vss; E2: wass; E3: yass, yss; E4: gz, vss, yss), in ascending slots;
//     wss has a tree exactly for E2 and E4;
//   * segment_node: written into real arrays of segs x nodes slots (ASan watches the bounds), the nodes of all segments of
//     all levels tile the array without gap or overlap, level by level, and a parent's children lie in its own segment;
//   * f_level_base / f_tree_values: level 0, the key's loops, the upper levels and the batch's product tile the F buffer;
//   * host_loops: two, two, two, two and three;
//   * locate_bisect of locate_descent.hpp, the descent as it ships (children tested on the parent's mask alone, carried nodes
//     inherit), its `check` an oracle that knows the marked leaves, reports exactly the marked leaves with exactly their
//     masks, within checks <= 1 + 2 b ceil(log2 n) and products <= 5 + 2 ceil(log2 n) sum popcount(mask); cut into passes of
//     1 or 3 sets it reports the same and hands no pass more; a `check` that returns a code ends it with that code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#define PS_LOCATE_INDEX_ONLY 1
#include "../playsnark_amd/csrc/locate_phgr13_dev.hpp"

using namespace ps;
using namespace ps::phgr13_locate;

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
#include "host_locate_descent.hpp"  // locate_bisect and its oracle harness, which reports through CHECK

static unsigned long long rng_state = 0x7068677231336cull;
static unsigned long long rnd() {  // splitmix64
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int ceil_log2(u64 n) {
    int k = 0;
    while (((u64)1 << k) < n) k++;
    return k;
}
static int popcount(u32 m) {
    int k = 0;
    for (; m; m &= m - 1) k++;
    return k;
}

static void check_masks() {
    // the table of the issue: equation -> elements
    const bool reads[EQUATIONS][G1_ELEMENTS] = {
        /* E0 */ {false, false, false, true, false, true, false},   // yss, hs
        /* E1 */ {true, true, false, false, false, false, false},   // vss, vass
        /* E2 */ {false, false, true, false, false, false, false},  // wass
        /* E3 */ {false, false, false, true, true, false, false},   // yss, yass
        /* E4 */ {true, false, false, true, false, false, true},    // vss, yss, gz
    };
    const bool reads_wss[EQUATIONS] = {false, false, true, false, true};
    CHECK(VSS == 0 && VASS == 1 && WASS == 2 && YSS == 3 && YASS == 4 && HS == 5 && GZ == 6 && G1_ELEMENTS == 7, "element order");
    for (u32 mask = 0; mask <= ALL_EQUATIONS; mask++) {
        int slot[G1_ELEMENTS];
        const int n = element_slots(mask, slot);
        int expect = 0;
        for (int e = 0; e < G1_ELEMENTS; e++) {
            bool need = false;
            for (int c = 0; c < EQUATIONS; c++) need = need || (((mask >> c) & 1u) && reads[c][e]);
            CHECK((slot[e] >= 0) == need, "mask %u element %d", mask, e);
            if (need) CHECK(slot[e] == expect++, "mask %u element %d slot %d", mask, e, slot[e]);
        }
        CHECK(n == expect && n <= G1_ELEMENTS, "mask %u: %d trees", mask, n);
        bool w = false;
        for (int c = 0; c < EQUATIONS; c++) w = w || (((mask >> c) & 1u) && reads_wss[c]);
        CHECK(((mask & WSS_EQUATIONS) != 0) == w, "mask %u wss", mask);
    }
    CHECK(element_equations(G1_ELEMENTS) == 0 && element_equations(-1) == 0, "no such element");
    int total = 0;
    for (int c = 0; c < EQUATIONS; c++) total += host_loops(c);
    CHECK(total == 11 && host_loops(4) == 3 && host_loops(0) == 2, "host loops");
}

static void check_layout(u64 n, u64 segs, u64 diff) {
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    const int nl = locate::tree_levels(n, size, off);
    // G1 trees, level-major: every (level, segment, node) owns one slot of a real array
    std::vector<int> owner(segs * off[nl], -1);
    u64 next = 0;
    for (int l = 0; l < nl; l++)
        for (u64 s = 0; s < segs; s++) {
            const u64 base = segment_node(size, off, l, segs, s);
            CHECK(base == next, "n = %llu segs = %llu: level %d segment %llu starts at %llu, not %llu", (unsigned long long)n, (unsigned long long)segs, l,
                  (unsigned long long)s, (unsigned long long)base, (unsigned long long)next);
            for (u64 i = 0; i < size[l]; i++) {
                CHECK(owner.at(base + i) == -1, "slot written twice");
                owner.at(base + i) = (int)s;
            }
            next = base + size[l];
        }
    CHECK(next == owner.size(), "n = %llu segs = %llu: %llu of %zu slots", (unsigned long long)n, (unsigned long long)segs, (unsigned long long)next, owner.size());
    // one level of k_g1_pair_sums as the host launches it: in + seg * size[l], out + seg * size[l + 1]
    for (int l = 0; l + 1 < nl; l++)
        for (u64 s = 0; s < segs; s++)
            for (u64 i = 0; i < size[l + 1]; i++) {
                const u64 out = segs * off[l + 1] + s * size[l + 1] + i, in = segs * off[l] + s * size[l] + 2 * i;
                CHECK(out == segment_node(size, off, l + 1, segs, s) + i && in == segment_node(size, off, l, segs, s) + 2 * i, "launch strides");
                CHECK(owner.at(out) == (int)s && owner.at(in) == (int)s, "a parent and its child in different trees");
                if (locate::node_has_two_children(i, size[l])) CHECK(owner.at(in + 1) == (int)s, "right child in another tree");
            }
    // F buffer
    std::vector<char> f(f_tree_values(off, nl, diff), 0);
    auto take = [&](u64 at, u64 count) {
        for (u64 i = 0; i < count; i++) {
            CHECK(f.at(at + i) == 0, "F value owned twice");
            f.at(at + i) = 1;
        }
    };
    for (int l = 0; l < nl; l++) take(f_level_base(off, l, diff), size[l]);
    take(n, diff);                             // the key's loops behind level 0
    take(f_product_at(off, nl, diff), 1);      // the batch's product
    u64 at = f_key_levels_at(off, nl, diff);   // the levels of the tree over the key's loops, as phgr13_miller_levels lays them
    for (u64 m = diff; m > 1; m = (m + 1) / 2) {
        take(at, (m + 1) / 2);
        at += (m + 1) / 2;
    }
    CHECK(at <= f.size() && f.size() - at <= (u64)locate::MAX_LEVELS + 1, "n = %llu diff = %llu: %llu of %zu values", (unsigned long long)n,
          (unsigned long long)diff, (unsigned long long)at, f.size());
    for (u64 i = 0; i < at; i++) CHECK(f[i] == 1, "n = %llu diff = %llu: a hole in the F buffer", (unsigned long long)n, (unsigned long long)diff);
}

// the descent of verify_phgr13_locate.inc as it ships with an oracle that knows the marked leaves and their masks
static Descent check_descent(u64 n, const std::map<u64, u32>& bad) {
    const Descent d = descend_every_way(n, [&](int l, u64 i) {
        u64 lo, hi;
        locate::node_range(l, i, n, &lo, &hi);
        u32 m = 0;
        for (auto it = bad.lower_bound(lo); it != bad.end() && it->first < hi; ++it) m |= it->second;
        return m;
    });
    std::map<u64, u32> found;
    u64 bits = 0;
    for (size_t k = 0; k < d.leaves.size(); k++) found[d.leaves[k]] = d.masks[k];
    for (const auto& b : bad) bits += (u64)popcount(b.second);
    CHECK(found == bad && d.leaves.size() == bad.size(), "n = %llu, %zu marked: found %zu", (unsigned long long)n, bad.size(), d.leaves.size());
    // with the batch's own check and its five products
    CHECK(1 + (u64)d.checks <= 1 + 2 * bad.size() * (u64)ceil_log2(n) && d.levels == (u32)ceil_log2(n), "n = %llu, %zu marked: %u checks, %u levels",
          (unsigned long long)n, bad.size(), 1 + d.checks, d.levels);
    CHECK(EQUATIONS + d.products <= EQUATIONS + 2 * (u64)ceil_log2(n) * bits, "n = %llu, %zu marked: %llu products", (unsigned long long)n, bad.size(),
          (unsigned long long)(EQUATIONS + d.products));
    return d;
}

int main() {
    check_masks();
    for (u64 n = 1; n <= 70; n++)
        for (u64 segs : {(u64)1, (u64)2, (u64)7, (u64)13, (u64)70})
            check_layout(n, segs, segs % 3 == 0 ? 0 : segs - 1);
    for (u64 n : {(u64)127, (u64)130, (u64)300, (u64)1000, (u64)4097}) check_layout(n, 9, 6);
    check_layout(1, 1, 0);
    check_layout(3, 70, 63);
    for (u64 n : {(u64)1, (u64)2, (u64)3, (u64)5, (u64)7, (u64)64, (u64)65, (u64)127, (u64)130, (u64)300, (u64)1000}) {
        for (u32 m = 1; m <= ALL_EQUATIONS; m += 6) {
            check_descent(n, {{0, m}});
            check_descent(n, {{n - 1, m}});
            check_descent(n, {{n / 2, m}});
        }
        std::map<u64, u32> all, alt;
        for (u64 i = 0; i < n; i++) {
            all[i] = 1 + (u32)(rnd() % ALL_EQUATIONS);
            if (i % 2 == 0) alt[i] = 1 + (u32)(rnd() % ALL_EQUATIONS);
        }
        check_descent(n, all);
        check_descent(n, alt);
        for (int rep = 0; rep < 50; rep++) {
            std::map<u64, u32> some;
            const u64 b = 1 + rnd() % (n < 9 ? n : 9);
            while (some.size() < b) some[rnd() % n] = 1 + (u32)(rnd() % ALL_EQUATIONS);
            check_descent(n, some);
        }
    }
    check_descent(7, {{1, 0b00010u}, {5, 0b01000u}});  // different equations in different halves
    check_descent(65, {{32, 0b10011u}, {33, 0b00100u}});
    // levels of 7, 4, 2, 1 nodes, leaf 6 marked on three equations: the root's two children, the two children of node 1 of 2,
    // and node 3 of 4 has the single child 6 -- 2 + 2 + 0 tested nodes, each on the three equations
    const Descent seven = check_descent(7, {{6, 0b10011u}});
    CHECK(seven.checks == 4 && seven.levels == 3 && seven.products == 12, "n = 7, leaf 6: %u checks, %u levels, %llu products", seven.checks, seven.levels,
          (unsigned long long)seven.products);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_phgr13_locate_index ok\n");
    return 0;
}
