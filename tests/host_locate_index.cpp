// host_locate_index.cpp -- the index arithmetic of the locating batch verifier's trees, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/locate_dev.hpp keeps every level of three trees one behind the other; the descent of
// verify_locate.inc, locate_bisect of locate_descent.hpp, finds a node's children and its carried nodes with the functions
// compiled here, and is itself compiled here and run as it ships:
//   * tree_levels: the sizes halve (rounded up) down to one, the offsets are their running sum, the total is below 2 n + 32;
//   * node_range: the nodes of a level cover [0, n) without gap or overlap, and a node covers what its children cover;
//   * node_has_two_children: false exactly for the odd one out, whose range is its single child's;
//   * locate_bisect from the root, its `check` an oracle that knows a set of marked leaves, reports exactly the marked leaves
//     in ascending order, with at most 2 b ceil(log2 n) tested nodes and ceil(log2 n) levels; cut into passes of 1 or 3 sets
//     it reports the same and hands no pass more; a `check` that returns a code ends it with that code;
//   * words8_add_mod_r against 128-bit arithmetic on the edges 0, 1, r - 1 and pairs that sum to exactly r.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../playsnark_amd/csrc/locate_dev.hpp"

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
#include "host_locate_descent.hpp"  // locate_bisect and its oracle harness, which reports through CHECK

static unsigned long long rng_state = 0x6c6f63617465ull;
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

static void check_tree(u64 n) {
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    const int nl = locate::tree_levels(n, size, off);
    CHECK(nl >= 1 && nl <= locate::MAX_LEVELS && nl == ceil_log2(n) + 1, "n = %llu: %d levels", (unsigned long long)n, nl);
    CHECK(size[0] == n && off[0] == 0 && size[nl - 1] == 1, "n = %llu: ends", (unsigned long long)n);
    for (int l = 0; l + 1 < nl; l++) {
        CHECK(size[l + 1] == (size[l] + 1) / 2 && off[l + 1] == off[l] + size[l], "n = %llu level %d", (unsigned long long)n, l);
    }
    CHECK(off[nl] == off[nl - 1] + 1 && off[nl] < 2 * n + 32, "n = %llu: %llu nodes", (unsigned long long)n, (unsigned long long)off[nl]);
    if (n > 4096) return;  // the ranges node by node for the small trees
    for (int l = 0; l < nl; l++) {
        u64 expect = 0;
        for (u64 i = 0; i < size[l]; i++) {
            u64 lo, hi;
            locate::node_range(l, i, n, &lo, &hi);
            CHECK(lo == expect && hi > lo && hi <= n, "n = %llu node (%d, %llu): [%llu, %llu)", (unsigned long long)n, l, (unsigned long long)i,
                  (unsigned long long)lo, (unsigned long long)hi);
            expect = hi;
            if (l > 0) {
                u64 a, b, c2, d;
                locate::node_range(l - 1, 2 * i, n, &a, &b);
                if (locate::node_has_two_children(i, size[l - 1])) {
                    locate::node_range(l - 1, 2 * i + 1, n, &c2, &d);
                    CHECK(a == lo && b == c2 && d == hi, "n = %llu node (%d, %llu): children", (unsigned long long)n, l, (unsigned long long)i);
                } else {
                    CHECK(i == size[l] - 1 && size[l - 1] % 2 == 1 && a == lo && b == hi, "n = %llu node (%d, %llu): carried", (unsigned long long)n, l,
                          (unsigned long long)i);
                }
            }
        }
        CHECK(expect == n, "n = %llu level %d covers %llu", (unsigned long long)n, l, (unsigned long long)expect);
    }
}

// the descent of verify_locate.inc as it ships (one equation: mask 1) with an oracle that knows the marked leaves
static Descent check_descent(u64 n, const std::set<u64>& bad) {
    const Descent d = descend_every_way(n, [&](int l, u64 i) {
        u64 lo, hi;
        locate::node_range(l, i, n, &lo, &hi);
        auto it = bad.lower_bound(lo);
        return it != bad.end() && *it < hi ? 1u : 0u;
    });
    CHECK(std::set<u64>(d.leaves.begin(), d.leaves.end()) == bad && d.leaves.size() == bad.size() && d.masks == std::vector<uint8_t>(bad.size(), 1),
          "n = %llu, %zu marked: found %zu", (unsigned long long)n, bad.size(), d.leaves.size());
    CHECK(1 + (u64)d.checks <= 1 + 2 * bad.size() * (u64)ceil_log2(n) && d.levels == (u32)ceil_log2(n), "n = %llu, %zu marked: %u checks, %u levels",
          (unsigned long long)n, bad.size(), 1 + d.checks, d.levels);  // with the batch's own check
    return d;
}

typedef unsigned __int128 u128;
static void check_add(const u32* a, const u32* b) {
    u32 acc[8], want[8];
    std::memcpy(acc, a, 32);
    locate::words8_add_mod_r(acc, b);
    // reference: 256-bit sum in two 128-bit halves, then one conditional subtraction of r
    u32 sum[9];
    u64 carry = 0;
    for (int i = 0; i < 8; i++) {
        const u64 s = (u64)a[i] + b[i] + carry;
        sum[i] = (u32)s;
        carry = s >> 32;
    }
    sum[8] = (u32)carry;
    bool ge = sum[8] != 0;
    if (!ge) {
        ge = true;
        for (int i = 7; i >= 0; i--)
            if (sum[i] != FrParams::mod(i)) { ge = sum[i] > FrParams::mod(i); break; }
    }
    if (ge) {
        long long borrow = 0;
        for (int i = 0; i < 8; i++) {
            long long d = (long long)sum[i] - (long long)FrParams::mod(i) - borrow;
            borrow = d < 0;
            want[i] = (u32)(d + (borrow ? (1ll << 32) : 0));
        }
    } else {
        std::memcpy(want, sum, 32);
    }
    CHECK(!std::memcmp(acc, want, 32), "words8_add_mod_r");
    bool below = false;
    for (int i = 7; i >= 0; i--)
        if (acc[i] != FrParams::mod(i)) { below = acc[i] < FrParams::mod(i); break; }
    CHECK(below, "words8_add_mod_r: result not below r");
}

int main() {
    for (u64 n = 1; n <= 1100; n++) check_tree(n);
    for (u64 n : {(u64)4095, (u64)4096, (u64)65537, (u64)1 << 20, ((u64)1 << 20) + 1, (u64)1 << 24, ((u64)1 << 32) - 1}) check_tree(n);
    for (u64 n : {(u64)1, (u64)2, (u64)3, (u64)5, (u64)7, (u64)64, (u64)65, (u64)127, (u64)130, (u64)300, (u64)1000}) {
        check_descent(n, {0});
        check_descent(n, {n - 1});
        check_descent(n, {n / 2});
        std::set<u64> all, alt;
        for (u64 i = 0; i < n; i++) { all.insert(i); if (i % 2 == 0) alt.insert(i); }
        check_descent(n, all);
        check_descent(n, alt);
        for (int rep = 0; rep < 50; rep++) {
            std::set<u64> some;
            const u64 b = 1 + rnd() % (n < 9 ? n : 9);
            while (some.size() < b) some.insert(rnd() % n);
            check_descent(n, some);
        }
    }
    check_descent(300, {296, 299});
    check_descent(300, {0, 1});
    check_descent(300, {0, 299});
    // levels of 7, 4, 2, 1 nodes, leaf 6 marked: the root's two children, the two children of node 1 of 2 (nodes 2 and 3 of
    // 4), and node 3 of 4 has the single child 6 -- 2 + 2 + 0 tested nodes
    const Descent seven = check_descent(7, {6});
    CHECK(seven.checks == 4 && seven.levels == 3 && seven.calls == 2, "n = 7, leaf 6: %u checks, %u levels, %zu calls", seven.checks, seven.levels, seven.calls);
    u32 r[8], zero[8] = {0}, one[8] = {1}, rm1[8];
    for (int i = 0; i < 8; i++) r[i] = FrParams::mod(i);
    std::memcpy(rm1, r, 32);
    rm1[0] -= 1;
    const u32* edges[4] = {zero, one, rm1, nullptr};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) check_add(edges[i], edges[j]);
    for (int rep = 0; rep < 2000; rep++) {
        u32 a[8], b[8];
        do {
            for (int i = 0; i < 8; i++) a[i] = (u32)rnd();
            a[7] &= 0x7fffffffu;
        } while (a[7] >= r[7]);
        // b = r - a: the pair sums to exactly r
        long long borrow = 0;
        for (int i = 0; i < 8; i++) {
            long long d = (long long)r[i] - (long long)a[i] - borrow;
            borrow = d < 0;
            b[i] = (u32)(d + (borrow ? (1ll << 32) : 0));
        }
        check_add(a, b);
        u32 s[8];
        std::memcpy(s, a, 32);
        locate::words8_add_mod_r(s, b);
        CHECK(!std::memcmp(s, zero, 32), "a + (r - a) != 0");
        check_add(a, a);
        check_add(a, rm1);
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_locate_index ok\n");
    return 0;
}
