// host_kzg_all_plan.cpp -- the index arithmetic of the openings at every node of the domain (ps_kzg_all_key_lagrange,
// ps_kzg_open_all_lagrange), checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/kzg_all_plan.hpp says which transform size S = 2^p an n takes, where kappa(d) = 1 / d sits in the wrapped
// multiplier, where a node's input and result sit, how large the buffers are and when a call is too large.  Against literal
// loops:
//   * p and S on both sides of every power of two, n = 2^k and 2^k + 1 for k = 0 .. 20 (and 2^k - 1): S is the smallest power of
//     two >= 2n - 1, recomputed here without the header;
//   * every offset d = -(n-1) .. n-1 written through its index into a real array of S entries (ASan watches the bounds): every
//     index within [0, S), no two offsets colliding, index 0 left to kappa(0) = 0, and the way back (index -> offset) agreeing --
//     for every n up to 300 and the n around the powers of two up to 2^12; the two ends d = +-(n-1) alone up to 2^20;
//   * the cyclic convolution through these indices equals the literal Toeplitz sum, in integers modulo a small prime, and the
//     multiplier written at the NEGATED indices gives the negated sum (kappa is antisymmetric);
//   * the buffers: the normalisation of n results fits the S points; sizes in 128-bit arithmetic at the limit;
//   * the n limit: 1 <= n <= 2^30, S <= 2^31 fits the 32-bit indices of the transform over points.
// Prints "n p S" per swept n for tests/test_kzg_all_plan_host.py, which derives them again.
#include <algorithm>
#include <cstdio>
#include <vector>

#ifndef KZG_ALL_PLAN_HEADER
#define KZG_ALL_PLAN_HEADER "../playsnark_amd/csrc/kzg_all_plan.hpp"
#endif
#include KZG_ALL_PLAN_HEADER

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

static void check_size(uint64_t n) {
    int p = 0;
    uint64_t S = 1;
    while (S < 2 * n - 1) { S *= 2; p++; }
    CHECK(kzg_all_size_ok(n), "n=%llu", (ull)n);
    CHECK(kzg_all_log(n) == p && kzg_all_size(n) == S, "n=%llu: p=%d S=%llu", (ull)n, kzg_all_log(n), (ull)kzg_all_size(n));
    CHECK(S >= 2 * n - 1 && (p == 0 || S / 2 < 2 * n - 1) && p <= KZG_ALL_MAX_LOG, "n=%llu", (ull)n);
    // the two ends of the offsets: inside [0, S), apart from each other and from index 0
    if (n >= 2) {
        const uint64_t hi = kzg_all_kappa_index((int64_t)(n - 1), p), lo = kzg_all_kappa_index(-(int64_t)(n - 1), p);
        CHECK(hi == n - 1 && lo == S - (n - 1) && hi < lo && lo < S, "n=%llu", (ull)n);
        CHECK(kzg_all_kappa_offset(hi, n, p) == (int64_t)(n - 1) && kzg_all_kappa_offset(lo, n, p) == -(int64_t)(n - 1), "n=%llu", (ull)n);
        CHECK(kzg_all_kappa_offset(n, n, p) == 0 || n == S - (n - 1), "n=%llu: the first index past the positive offsets", (ull)n);
    }
    CHECK(kzg_all_kappa_offset(0, n, p) == 0, "n=%llu", (ull)n);
    CHECK(kzg_all_node_index(1) == 0 && kzg_all_node_index(n) == n - 1 && kzg_all_node_index(n) < S, "n=%llu", (ull)n);
    // buffers
    CHECK(kzg_all_point_elems(n) == S && kzg_all_kappa_elems(n) == S && kzg_all_scalar_elems(n) == 2 * S && kzg_all_value_elems(n) == n, "n=%llu", (ull)n);
    if (n >= 2) CHECK(kzg_all_normalise_fits(n) && (u128)n * (224 + 56) <= (u128)S * 224, "n=%llu", (ull)n);
    std::printf("%llu %d %llu\n", (ull)n, p, (ull)S);
}

// every offset through its index into a real array; the convolution against the literal sum, modulo a small prime
static void check_placement(uint64_t n) {
    const int p = kzg_all_log(n);
    const uint64_t S = kzg_all_size(n), Q = 1000003;
    std::vector<int64_t> held(S, 0);
    std::vector<unsigned char> met(S, 0);
    std::vector<uint64_t> kap(S, 0), rev(S, 0), inv(n + 1, 0);
    for (uint64_t d = 1; d < n; d++) {  // 1 / d mod Q by Fermat
        uint64_t r = 1, b = d % Q, e = Q - 2;
        for (; e; e >>= 1, b = b * b % Q)
            if (e & 1) r = r * b % Q;
        inv[d] = r;
    }
    for (int64_t d = -(int64_t)(n - 1); d <= (int64_t)(n - 1); d++) {
        const uint64_t t = kzg_all_kappa_index(d, p), tr = kzg_all_kappa_index(-d, p);
        CHECK(t < S, "n=%llu d=%lld", (ull)n, (long long)d);
        met.at(t)++;
        held.at(t) = d;
        const uint64_t a = (uint64_t)(d < 0 ? -d : d);
        kap.at(t) = d == 0 ? 0 : d > 0 ? inv[a] : (Q - inv[a]) % Q;
        rev.at(tr) = kap.at(t);
    }
    for (uint64_t t = 0; t < S; t++) {
        CHECK(met[t] <= 1, "n=%llu: two offsets at index %llu", (ull)n, (ull)t);
        CHECK(kzg_all_kappa_offset(t, n, p) == (met[t] ? held[t] : 0), "n=%llu t=%llu", (ull)n, (ull)t);
    }
    if (n > 64) return;
    std::vector<uint64_t> x(S, 0);
    for (uint64_t i = 1; i <= n; i++) x.at(kzg_all_node_index(i)) = (i * i * 7919 + 13) % Q;
    for (uint64_t m = 1; m <= n; m++) {
        uint64_t want = 0, got = 0, got_rev = 0;
        for (uint64_t i = 1; i <= n; i++)
            if (i != m) want = (want + (m > i ? inv[m - i] : Q - inv[i - m]) % Q * x[i - 1]) % Q;
        const uint64_t a = kzg_all_node_index(m);
        for (uint64_t j = 0; j < S; j++) {
            got = (got + kap[(a + S - j) % S] * x[j]) % Q;
            got_rev = (got_rev + rev[(a + S - j) % S] * x[j]) % Q;
        }
        CHECK(got == want, "n=%llu m=%llu", (ull)n, (ull)m);
        CHECK(got_rev == (Q - want) % Q, "n=%llu m=%llu: the reversed multiplier", (ull)n, (ull)m);
    }
}

int main() {
    CHECK(KZG_ALL_MAX_N == (uint64_t)1 << 30 && KZG_ALL_MAX_LOG == 31 && KZG_ALL_SCALAR_BATCH == 2, "constants");
    {
        std::vector<uint64_t> ns;
        for (int k = 0; k <= 20; k++)
            for (uint64_t n : {((uint64_t)1 << k) - 1, (uint64_t)1 << k, ((uint64_t)1 << k) + 1})
                if (n >= 1) ns.push_back(n);
        std::sort(ns.begin(), ns.end());
        ns.erase(std::unique(ns.begin(), ns.end()), ns.end());
        for (uint64_t n : ns) check_size(n);
    }
    for (uint64_t n = 1; n <= 300; n++) check_placement(n);
    for (int k = 9; k <= 12; k++)
        for (uint64_t n : {((uint64_t)1 << k) - 1, (uint64_t)1 << k, ((uint64_t)1 << k) + 1}) check_placement(n);
    // the limit: 1 <= n <= 2^30; at the limit S = 2^31 and every size fits 64 bits with room to spare
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << 30) - 1, (uint64_t)1 << 30, ((uint64_t)1 << 30) + 1, (uint64_t)1 << 31, (uint64_t)1 << 32,
                       ~(uint64_t)0})
        CHECK(kzg_all_size_ok(n) == (n >= 1 && n <= ((uint64_t)1 << 30)), "n=%llu", (ull)n);
    CHECK(kzg_all_log(KZG_ALL_MAX_N) == 31 && kzg_all_size(KZG_ALL_MAX_N) == (uint64_t)1 << 31, "the largest transform");
    CHECK(kzg_all_size(KZG_ALL_MAX_N) <= 0xffffffffull, "S fits the 32-bit indices of the transform over points");
    CHECK(kzg_all_log(KZG_ALL_MAX_N - 1) == 31 && kzg_all_log((KZG_ALL_MAX_N >> 1) + 1) == 31 && kzg_all_log(KZG_ALL_MAX_N >> 1) == 30, "below the limit");
    CHECK((u128)kzg_all_point_elems(KZG_ALL_MAX_N) * KZG_ALL_XYZZ_BYTES < ((u128)1 << 63), "bytes of the point buffer at the limit");
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_kzg_all_plan ok\n");
    return 0;
}
