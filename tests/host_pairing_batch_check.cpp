// host_pairing_batch_check.cpp -- the PS_HD helpers of playsnark_amd/csrc/pairing_dev.hpp that are NOT literally
// pairing_dev::miller / f12_mul, compiled for the host with
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
// and driven with the lanes emulated by a loop:
//   * f12_mul_mem (the product tree's coefficient-by-coefficient product) == f12_mul, mod p, on random operands and on
//     the worst-case lazy-limb operands of host_limb_check.cpp (every limb at the edge of its class, |value| <= 16 p);
//   * a 1 000-factor product tree of worst-case operands, level by level through f12_tree_node as k_f12_product runs
//     it, equals the serial product (computed in the host field) and every stored coefficient stays at limb class <= 2;
//   * the conversion of a device value into the host field (what the verifier does with the downloaded product);
//   * spread_index: every element is taken by exactly one lane of the launch;
//   * fr_weighted_column against a plain sum of products, chunked as the kernel chunks it.
// Exit code 0 = all checks passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <vector>

#include "../playsnark_amd/csrc/curve.hpp"

using namespace ps;

template <class F> static bool affine_is_identity(const Affine<F>& p) { return fp_all_zero(p.x) && fp_all_zero(p.y); }
namespace ps {
#include "../playsnark_amd/csrc/hostfield.inc"
}
#define PS_HOSTFIELD 1
#include "../playsnark_amd/csrc/pairing_math.inc"
#include "../playsnark_amd/csrc/pairing_dev.hpp"

static unsigned long long rng_state = 0x7061697262617463ull;
static unsigned long long rnd() {  // splitmix64
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            failures++;                                                          \
            std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                   \
            std::fprintf(stderr, "\n");                                          \
        }                                                                        \
    } while (0)

static int limb_class(const Fp& a) {
    long long m = 0;
    for (int i = 0; i < FP_L; i++) { long long v = a.l[i] < 0 ? -(long long)a.l[i] : a.l[i]; if (v > m) m = v; }
    return (int)(m >> 28) + 1;
}
// as in host_limb_check.cpp: limbs at the edge of the class, the top limb at the edge of |value| <= 16 p
static const long long TOP_SPAN = 15ll * fp_mod28(FP_L - 1);
static Fp worst(int cls, int pattern) {
    Fp r;
    for (int i = 0; i < FP_L; i++) {
        i32 v = i == FP_L - 1 ? (i32)TOP_SPAN : (i32)(((long long)cls << 28) - 1);
        bool neg = pattern == 1 || (pattern == 2 && (i & 1)) || (pattern == 3 && (rnd() & 1));
        r.l[i] = neg ? -v : v;
    }
    return r;
}
static Fp random_canon() {
    u32 w[12];
    for (int i = 0; i < 12; i++) w[i] = (u32)rnd();
    w[11] &= 0x0fffffffu;  // below p
    return fp_to_mont(fp_from_words12(w));
}
typedef pairing_dev::Fp12 D12;
static Fp* limb(D12& a, int k) {
    Fp2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    return (k & 1) ? &c[k >> 1]->c1 : &c[k >> 1]->c0;
}
static D12 worst12(int cls, int seed) {
    D12 a;
    for (int k = 0; k < 12; k++) *limb(a, k) = worst(cls, (seed + k) & 3);
    return a;
}
static D12 random12() {
    D12 a;
    for (int k = 0; k < 12; k++) *limb(a, k) = random_canon();
    return a;
}
static pairing::Fp12 host12(const D12& a) { return f12_to_host(a); }  // the conversion the verifier runs
static int class12(D12& a) {
    int c = 0;
    for (int k = 0; k < 12; k++) c = std::max(c, limb_class(*limb(a, k)));
    return c;
}

static void check_mul_mem() {
    int n = 0;
    for (int it = 0; it < 200; it++) {
        D12 a, b;
        if (it < 64) { a = worst12(2, it); b = worst12(2, it >> 2); }        // class 2 x class 2
        else if (it < 96) { a = worst12(4, it); b = worst12(1, it >> 2); }   // class 4 x class 1
        else { a = random12(); b = random12(); }
        D12 m;
        pairing_dev::f12_mul_mem(m, a, b);
        D12 want = pairing_dev::f12_mul(a, b);
        CHECK(pairing::f12_eq(host12(m), host12(want)), "f12_mul_mem != f12_mul (case %d)", it);
        // ... and both equal the product formed in the host field from the converted operands
        CHECK(pairing::f12_eq(host12(m), pairing::f12_mul(host12(a), host12(b))), "f12_mul_mem != host product (case %d)", it);
        CHECK(class12(m) <= 2, "f12_mul_mem left limb class %d", class12(m));
        n++;
    }
    std::printf("f12_mul_mem == f12_mul on %d worst-case and random operand pairs\n", n);
}

static void check_tree() {
    const u32 N = 1000;
    std::vector<D12> lvl(N), nxt((N + 1) / 2);
    for (u32 i = 0; i < N; i++) lvl[i] = worst12(2, (int)i);
    pairing::Fp12 serial = pairing::f12_one();
    for (u32 i = 0; i < N; i++) serial = pairing::f12_mul(serial, host12(lvl[i]));
    u32 n = N;
    int worst_cls = 0, levels = 0;
    while (n > 1) {
        const u32 h = (n + 1) / 2, lpw = 3;  // waves of three active lanes, as a small batch is spread
        std::vector<int> taken(h, 0);
        for (u32 tid = 0; tid < ((h + lpw - 1) / lpw) * 64; tid++) {
            u32 i;
            if (!pairing_dev::spread_index(tid, lpw, h, i)) continue;
            taken[i]++;
            pairing_dev::f12_tree_node(nxt.data(), lvl.data(), n, i);
        }
        for (u32 i = 0; i < h; i++) CHECK(taken[i] == 1, "element %u taken %d times", i, taken[i]);
        for (u32 i = 0; i < h; i++) { lvl[i] = nxt[i]; if (2 * i + 1 < n) worst_cls = std::max(worst_cls, class12(lvl[i])); }
        n = h;
        levels++;
    }
    CHECK(pairing::f12_eq(host12(lvl[0]), serial), "tree product != serial product");
    CHECK(worst_cls <= 2, "tree values reached limb class %d", worst_cls);
    std::printf("product tree of %u worst-case factors == serial product (%d levels, limb class <= %d)\n", N, levels, worst_cls);
}

static void check_spread() {
    const u32 simds = 1024;
    for (u32 n : {1u, 2u, 63u, 64u, 65u, 1000u, 1024u, 1025u, 4096u, 4097u, 65536u, 70001u}) {
        const u32 lpw = pairing_dev::spread_lanes(n, simds);
        CHECK(lpw >= 1 && lpw <= 64, "lanes per wave %u", lpw);
        const u32 waves = (n + lpw - 1) / lpw;
        CHECK(n > 64 * simds || waves <= simds || lpw == 64, "n = %u: %u waves of %u lanes", n, waves, lpw);
        std::vector<unsigned char> taken(n, 0);
        for (u32 tid = 0; tid < waves * 64; tid++) {
            u32 i = ~0u;
            if (pairing_dev::spread_index(tid, lpw, n, i)) { CHECK(i < n, "index %u of %u", i, n); if (i < n) taken[i]++; }
        }
        for (u32 i = 0; i < n; i++) CHECK(taken[i] == 1, "n = %u: element %u taken %d times", n, i, (int)taken[i]);
    }
    std::printf("spread_index covers every element exactly once\n");
}

static void check_columns() {
    const u32 rows = 203, cols = 5;
    std::vector<Fr> w(rows);
    std::vector<u32> m((size_t)rows * cols * 8);
    for (u32 i = 0; i < rows; i++) {
        u32 x[8];
        for (int k = 0; k < 8; k++) x[k] = i % 7 == 0 ? FrParams::mod(k) - (k == 0) : (u32)rnd();  // r - 1 among them
        if (i % 7) x[7] &= 0x3fffffffu;
        w[i] = fr_to_mont(fr_from_words8(x));
        for (u32 j = 0; j < cols; j++)
            for (int k = 0; k < 8; k++) m[((size_t)i * cols + j) * 8 + k] = (i + j) % 5 == 0 ? FrParams::mod(k) - (k == 0) : ((u32)rnd() & (k == 7 ? 0x3fffffffu : ~0u));
    }
    for (u32 j = 0; j < cols; j++) {
        Fr want = fr_zero();
        for (u32 i = 0; i < rows; i++) want = fr_canon(fr_reduce(fr_add(want, fr_mul(w[i], fr_from_words8(&m[((size_t)i * cols + j) * 8])))));
        // two passes, as the host runs the kernel: chunks of 64 rows, then the chunks' sums with weight one
        const u32 per = 64, chunks = (rows + per - 1) / per;
        std::vector<u32> part((size_t)chunks * 8);
        for (u32 c = 0; c < chunks; c++) fr_to_words8(&part[c * 8], fr_weighted_column(w.data(), m.data(), cols, j, c * per, std::min(rows, (c + 1) * per)));
        Fr got = fr_weighted_column(nullptr, part.data(), 1, 0, 0, chunks);
        bool same = true;
        for (int k = 0; k < FR_L; k++) same = same && got.l[k] == want.l[k];
        CHECK(same, "column %u", j);
    }
    std::printf("weighted column sums ok\n");
}

int main() {
    check_mul_mem();
    check_tree();
    check_spread();
    check_columns();
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("host_pairing_batch_check ok\n");
    return 0;
}
