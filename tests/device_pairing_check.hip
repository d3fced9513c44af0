// device_pairing_check.hip -- a test-only program (never linked into the product) that runs the batch verifier's device
// side ON THE GPU, as the product compiles it, and the same functions compiled for the host next to it:
//   * the shipped kernels of playsnark_amd/csrc/pairing_dev.hpp -- ps::k_miller_batch, ps::k_f12_product,
//     ps::k_fr_weighted_columns -- launched directly, with the grid and the lanes per wave chosen by the caller;
//   * the tower of pairing_body.inc over the device representation (namespace pairing_dev), one element per thread.
// Built by tests/test_device_pairing.py with the product's flags; the headers are included unmodified.
//
//     device_pairing_check OP N IN OUT
//
// IN and OUT are raw int32 words.  For every operation OUT holds what the device computed and then what the SAME
// pairing_dev:: / ps:: function gives compiled for the host (every Fp product in its C++ form).  OP "host:<op>" computes
// the host part alone and makes no HIP call.  Layouts (W12 = 168 words: an Fp12 as the struct lies in memory):
//   tower ops     IN  N x (the operands' raw limbs)                OUT N x result (device), N x result (host)
//   miller        IN  lpw, N x (x, y of P: 24 canonical words; x.c0, x.c1, y.c0, y.c1 of Q: 48); all zero = identity
//                 OUT (N + PAD) x W12 (device, buffer poisoned beforehand), N x W12 (host)
//   tree          IN  nlpw, lpw[nlpw], N x W12 raw limbs
//                 OUT per lpw, per level (n -> h = ceil(n / 2) until 1): (h + PAD) x W12 (device, poisoned beforehand);
//                     then per level h x W12 (host)
//   columns       IN  cols, nrpc, rows_per_chunk[nrpc], N x 8 weight words (canonical), N x cols x 8 entry words
//                 OUT for weights / nullptr, per rows_per_chunk: (chunks + 1) x cols x 8 (device pass one, poisoned),
//                     2 x cols x 8 (device pass two over the chunk sums, poisoned), chunks x cols x 8, cols x 8 (host)
// Exit status 0 = every HIP call succeeded; the checking is the test's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <vector>

#include "../playsnark_amd/csrc/curve.hpp"

using namespace ps;

template <class F>
PS_HD static inline bool affine_is_identity(const Affine<F>& p) { return fp_all_zero(p.x) && fp_all_zero(p.y); }
namespace ps {
#include "../playsnark_amd/csrc/hostfield.inc"
}
#define PS_HOSTFIELD 1
#include "../playsnark_amd/csrc/pairing_math.inc"
#include "../playsnark_amd/csrc/pairing_dev.hpp"

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(3);                                                                           \
        }                                                                                           \
    } while (0)

typedef pairing_dev::Fp6 D6;
typedef pairing_dev::Fp12 D12;
constexpr int W1 = FP_L, W2 = 2 * FP_L, W6 = 6 * FP_L, W12 = 12 * FP_L;
constexpr int PAD = 8;               // elements past the end of an output buffer, which must keep the poison
constexpr int POISON_BYTE = 0xA5;    // every word 0xA5A5A5A5: no limb of a result
static_assert(sizeof(Fp2) == 4 * W2 && sizeof(D6) == 4 * W6 && sizeof(D12) == 4 * W12, "the tower is plain limbs");

// a value of the tower <-> its limbs in memory order (c0 before c1 at every level)
template <class T>
PS_HD static inline T ld(const i32* p) {
    T r;
    i32* d = reinterpret_cast<i32*>(&r);
    for (unsigned i = 0; i < sizeof(T) / 4; i++) d[i] = p[i];
    return r;
}
template <class T>
PS_HD static inline void st(i32* o, const T& a) {
    const i32* s = reinterpret_cast<const i32*>(&a);
    for (unsigned i = 0; i < sizeof(T) / 4; i++) o[i] = s[i];
}

// ---- the tower operations: IN words per case, OUT words per case; run() compiles for both sides ----
#define OP(NAME, IN_, OUT_, ...)                                      \
    struct NAME {                                                     \
        static constexpr int IN = IN_, OUT = OUT_;                    \
        PS_HD static void run(const i32* in, i32* o) { __VA_ARGS__; } \
    };
OP(OpMulXi, W2, W2, st(o, pairing_dev::mul_xi(ld<Fp2>(in))))
OP(OpF2Scale, W2 + W1, W2, st(o, pairing_dev::f2_scale(ld<Fp2>(in), ld<Fp>(in + W2))))
OP(OpF2Reduce, W2, W2, st(o, pairing_dev::f2_reduce(ld<Fp2>(in))))
OP(OpF6Mul, 2 * W6, W6, st(o, pairing_dev::f6_mul(ld<D6>(in), ld<D6>(in + W6))))
OP(OpF6Mul01, W6 + 2 * W2, W6, st(o, pairing_dev::f6_mul_01(ld<D6>(in), ld<Fp2>(in + W6), ld<Fp2>(in + W6 + W2))))
OP(OpF6Mul1, W6 + W2, W6, st(o, pairing_dev::f6_mul_1(ld<D6>(in), ld<Fp2>(in + W6))))
OP(OpF12Mul, 2 * W12, W12, st(o, pairing_dev::f12_mul(ld<D12>(in), ld<D12>(in + W12))))
OP(OpF12Sqr, W12, W12, st(o, pairing_dev::f12_sqr(ld<D12>(in))))
OP(OpF12MulLine, W12 + 3 * W2, W12,
   st(o, pairing_dev::f12_mul_line(ld<D12>(in), ld<Fp2>(in + W12), ld<Fp2>(in + W12 + W2), ld<Fp2>(in + W12 + 2 * W2))))
OP(OpF12MulMem, 2 * W12, W12, {
    const D12 a = ld<D12>(in), b = ld<D12>(in + W12);
    D12 m;
    pairing_dev::f12_mul_mem(m, a, b);
    st(o, m);
})

template <class Op>
__global__ void __launch_bounds__(64) k_case(const i32* __restrict__ in, i32* __restrict__ out, int n) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    i32 res[Op::OUT];
    Op::run(in + (size_t)c * Op::IN, res);
    for (int i = 0; i < Op::OUT; i++) out[(size_t)c * Op::OUT + i] = res[i];
}

typedef std::vector<i32> Words;
struct Dev {  // a device buffer of words, poisoned, freed at the end of the operation
    i32* p = nullptr;
    size_t n;
    explicit Dev(size_t words) : n(words) {
        HIP_OK(hipMalloc(&p, (n ? n : 1) * sizeof(i32)));
        HIP_OK(hipMemset(p, POISON_BYTE, (n ? n : 1) * sizeof(i32)));
    }
    Dev(const Dev&) = delete;
    ~Dev() { (void)hipFree(p); }
    void up(const void* src, size_t words) { HIP_OK(hipMemcpy(p, src, words * sizeof(i32), hipMemcpyHostToDevice)); }
    void down(Words& out) const {
        const size_t at = out.size();
        out.resize(at + n);
        if (n) HIP_OK(hipMemcpy(out.data() + at, p, n * sizeof(i32), hipMemcpyDeviceToHost));
    }
};
static void done_launch() {
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
}
[[noreturn]] static void bad_input(const char* what) {
    std::fprintf(stderr, "bad input: %s\n", what);
    std::exit(2);
}

template <class Op>
static void run_tower(long n, const Words& in, Words& out, bool device) {
    if (in.size() != (size_t)n * Op::IN) bad_input("tower op: wrong number of input words");
    if (device) {
        Dev d_in(in.size()), d_out((size_t)n * Op::OUT);
        d_in.up(in.data(), in.size());
        k_case<Op><<<(unsigned)((n + 63) / 64), 64>>>(d_in.p, d_out.p, (int)n);
        done_launch();
        d_out.down(out);
    }
    const size_t at = out.size();
    out.resize(at + (size_t)n * Op::OUT);
    for (long c = 0; c < n; c++) Op::run(in.data() + (size_t)c * Op::IN, out.data() + at + (size_t)c * Op::OUT);
}

static Fp fp_of_words(const i32* w) { return fp_to_mont(fp_from_words12(reinterpret_cast<const u32*>(w))); }

static void run_miller(long n, const Words& in, Words& out, bool device) {
    if (in.size() != 1 + (size_t)n * 72) bad_input("miller: wrong number of input words");
    const u32 lpw = (u32)in[0];
    if (lpw < 1 || lpw > 64) bad_input("miller: lanes per wave outside 1 .. 64");
    std::vector<Affine<Fp>> g1(n);
    std::vector<Affine<Fp2>> g2(n);
    for (long i = 0; i < n; i++) {
        const i32* w = in.data() + 1 + (size_t)i * 72;
        g1[i] = Affine<Fp>{fp_of_words(w), fp_of_words(w + 12)};
        g2[i] = Affine<Fp2>{Fp2{fp_of_words(w + 24), fp_of_words(w + 36)}, Fp2{fp_of_words(w + 48), fp_of_words(w + 60)}};
    }
    if (device) {
        Dev d1(g1.size() * 2 * W1), d2(g2.size() * 2 * W2), d_out((size_t)(n + PAD) * W12);
        d1.up(g1.data(), d1.n);
        d2.up(g2.data(), d2.n);
        ps::k_miller_batch<<<(unsigned)((n + lpw - 1) / lpw), 64>>>((const Affine<Fp>*)d1.p, (const Affine<Fp2>*)d2.p, (u32)n, lpw, (D12*)d_out.p);
        done_launch();
        d_out.down(out);
    }
    std::vector<D12> host(n);
    std::vector<std::future<void>> jobs;
    const long T = 8;
    for (long t = 0; t < T; t++)
        jobs.push_back(std::async(std::launch::async, [&, t] {
            for (long i = t; i < n; i += T) host[i] = pairing_dev::miller(g1[i], g2[i]);
        }));
    for (auto& j : jobs) j.get();
    const size_t at = out.size();
    out.resize(at + (size_t)n * W12);
    std::memcpy(out.data() + at, host.data(), (size_t)n * W12 * sizeof(i32));
}

static void run_tree(long n, const Words& in, Words& out, bool device) {
    if (in.size() < 1 || in[0] < 0 || in[0] > 8 || in.size() != 1 + (size_t)in[0] + (size_t)n * W12) bad_input("tree: wrong number of input words");
    const int nlpw = in[0];
    const i32* fac = in.data() + 1 + nlpw;
    for (int k = 0; k < nlpw && device; k++) {
        const u32 lpw = (u32)in[1 + k];
        if (lpw < 1 || lpw > 64) bad_input("tree: lanes per wave outside 1 .. 64");
        Dev first((size_t)n * W12);
        first.up(fac, first.n);
        std::vector<Dev*> levels;
        const i32* src = first.p;
        for (u32 m = (u32)n; m > 1;) {  // as miller_product_launch runs it, every level into a buffer of its own
            const u32 h = (m + 1) / 2;
            Dev* dst = new Dev((size_t)(h + PAD) * W12);
            ps::k_f12_product<<<(h + lpw - 1) / lpw, 64>>>((const D12*)src, m, lpw, (D12*)dst->p);
            levels.push_back(dst);
            src = dst->p;
            m = h;
        }
        done_launch();
        for (Dev* d : levels) { d->down(out); delete d; }
    }
    std::vector<D12> lvl(n);
    std::memcpy(lvl.data(), fac, (size_t)n * W12 * sizeof(i32));
    for (u32 m = (u32)n; m > 1;) {
        const u32 h = (m + 1) / 2;
        std::vector<D12> nxt(h);
        for (u32 i = 0; i < h; i++) pairing_dev::f12_tree_node(nxt.data(), lvl.data(), m, i);
        const size_t at = out.size();
        out.resize(at + (size_t)h * W12);
        std::memcpy(out.data() + at, nxt.data(), (size_t)h * W12 * sizeof(i32));
        lvl.swap(nxt);
        m = h;
    }
}

static void run_columns(long rows, const Words& in, Words& out, bool device) {
    if (in.size() < 2 || in[0] < 1 || in[1] < 1 || in[1] > 8) bad_input("columns: header");
    const u32 cols = (u32)in[0];
    const int nrpc = in[1];
    const size_t hdr = 2 + (size_t)nrpc;
    if (in.size() != hdr + (size_t)rows * 8 + (size_t)rows * cols * 8) bad_input("columns: wrong number of input words");
    const u32* wwords = reinterpret_cast<const u32*>(in.data() + hdr);
    const u32* m = wwords + (size_t)rows * 8;
    std::vector<Fr> w(rows);
    for (long i = 0; i < rows; i++) w[i] = fr_to_mont(fr_from_words8(wwords + (size_t)i * 8));
    for (int weighted = 1; weighted >= 0; weighted--)
        for (int k = 0; k < nrpc; k++) {
            if (in[2 + k] < 1) bad_input("columns: rows per chunk");
            const u32 per = (u32)in[2 + k], chunks = ((u32)rows + per - 1) / per;
            if (device) {
                Dev d_w(w.size() * FR_L), d_m((size_t)rows * cols * 8), one((size_t)(chunks + 1) * cols * 8), two((size_t)2 * cols * 8);
                d_w.up(w.data(), d_w.n);
                d_m.up(m, d_m.n);
                const dim3 block(256);
                ps::k_fr_weighted_columns<<<dim3((cols + 255) / 256, chunks), block>>>(weighted ? (const Fr*)d_w.p : nullptr, (const u32*)d_m.p, (u32)rows,
                                                                                     cols, per, (u32*)one.p);
                ps::k_fr_weighted_columns<<<dim3((cols + 255) / 256, 1), block>>>(nullptr, (const u32*)one.p, chunks, cols, chunks, (u32*)two.p);
                done_launch();
                one.down(out);
                two.down(out);
            }
            std::vector<u32> part((size_t)chunks * cols * 8), full((size_t)cols * 8);
            for (u32 c = 0; c < chunks; c++)
                for (u32 j = 0; j < cols; j++) {
                    const u32 row0 = c * per, row1 = (u32)rows - row0 < per ? (u32)rows : row0 + per;
                    fr_to_words8(&part[((size_t)c * cols + j) * 8], fr_weighted_column(weighted ? w.data() : nullptr, m, cols, j, row0, row1));
                }
            for (u32 j = 0; j < cols; j++) fr_to_words8(&full[(size_t)j * 8], fr_weighted_column(nullptr, part.data(), cols, j, 0, chunks));
            const size_t at = out.size();
            out.resize(at + part.size() + full.size());
            std::memcpy(out.data() + at, part.data(), part.size() * 4);
            std::memcpy(out.data() + at + part.size(), full.data(), full.size() * 4);
        }
}

struct Entry {
    const char* name;
    void (*run)(long, const Words&, Words&, bool);
};
static const Entry kEntries[] = {
    {"mul_xi", run_tower<OpMulXi>}, {"f2_scale", run_tower<OpF2Scale>}, {"f2_reduce", run_tower<OpF2Reduce>},
    {"f6_mul", run_tower<OpF6Mul>}, {"f6_mul_01", run_tower<OpF6Mul01>}, {"f6_mul_1", run_tower<OpF6Mul1>},
    {"f12_mul", run_tower<OpF12Mul>}, {"f12_sqr", run_tower<OpF12Sqr>}, {"f12_mul_line", run_tower<OpF12MulLine>},
    {"f12_mul_mem", run_tower<OpF12MulMem>}, {"miller", run_miller}, {"tree", run_tree}, {"columns", run_columns},
};

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        for (const Entry& e : kEntries) std::printf("%s\n", e.name);
        return 0;
    }
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s [host:]OP N IN OUT | --list\n", argv[0]);
        return 2;
    }
    const bool device = std::strncmp(argv[1], "host:", 5) != 0;
    const char* op = device ? argv[1] : argv[1] + 5;
    const Entry* ent = nullptr;
    for (const Entry& e : kEntries)
        if (!std::strcmp(e.name, op)) ent = &e;
    const long n = std::atol(argv[2]);
    if (!ent || n <= 0 || n > (1 << 20)) bad_input("operation or case count");
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) bad_input("cannot open the input file");
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    Words in((size_t)bytes / 4), out;
    if (bytes % 4 || std::fread(in.data(), 4, in.size(), f) != in.size()) bad_input("cannot read the input file");
    std::fclose(f);
    ent->run(n, in, out, device);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f)) {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    return 0;
}
