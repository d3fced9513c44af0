// device_locate_check.hip -- a test-only program (never linked into the product) that launches the two tree kernels of the
// locating batch verifier ON THE GPU as the product compiles them: ps::k_g1_pair_sums and ps::k_fr_row_pair_sums of
// playsnark_amd/csrc/locate_dev.hpp, level by level as verify_locate.inc runs them, every level into a poisoned buffer of
// its own.  Built by tests/test_device_locate.py with the product's flags; the headers are included unmodified.
//
//     device_locate_check OP N IN OUT
//
// IN and OUT are raw 32-bit words.
//   rows    IN  cols, N x cols x 8 words (plain canonical scalars, row-major)
//           OUT per level (n -> h = ceil(n / 2) until 1; one level 1 -> 1 for N = 1): (h + PAD) x cols x 8 as the device left them
//   points  IN  segs, then segs x N x 24 words (x, y canonical plain words; all zero = the identity): segs segments of N points
//           OUT per level: segs x h x 24 words (the nodes normalised on the host: affine, canonical, plain; zero = identity),
//               then ONE word: the slots of the level's buffer no node owns that no longer hold the poison.
//               segs = 1 runs with strides 0 as the C tree does, segs > 1 with the segment stride N as the X_S sums do.
// Exit status 0 = every HIP call succeeded; the checking is the test's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <vector>

#include "../playsnark_amd/csrc/msm.hpp"

using namespace ps;

namespace ps {
#include "../playsnark_amd/csrc/hostfield.inc"
}
#define PS_HOSTFIELD 1
#include "../playsnark_amd/csrc/pairing_math.inc"
#include "../playsnark_amd/csrc/pairing_dev.hpp"
#include "../playsnark_amd/csrc/locate_dev.hpp"

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(3);                                                                           \
        }                                                                                           \
    } while (0)

constexpr int PAD = 8;             // elements past the end of an output buffer, which must keep the poison
constexpr int POISON_BYTE = 0xA5;  // every word 0xA5A5A5A5
constexpr u32 POISON = 0xA5A5A5A5u;
constexpr size_t WX = sizeof(Xyzz<Fp>) / 4;

typedef std::vector<u32> Words;
struct Dev {  // a device buffer of words, poisoned, freed at the end of the operation
    u32* p = nullptr;
    size_t n;
    explicit Dev(size_t words) : n(words) {
        HIP_OK(hipMalloc(&p, (n ? n : 1) * 4));
        HIP_OK(hipMemset(p, POISON_BYTE, (n ? n : 1) * 4));
    }
    Dev(const Dev&) = delete;
    ~Dev() { (void)hipFree(p); }
    void up(const void* src, size_t words) { HIP_OK(hipMemcpy(p, src, words * 4, hipMemcpyHostToDevice)); }
    Words down() const {
        Words out(n);
        if (n) HIP_OK(hipMemcpy(out.data(), p, n * 4, hipMemcpyDeviceToHost));
        return out;
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

static void run_rows(long n, const Words& in, Words& out) {
    if (in.size() < 1 || in[0] < 1 || in.size() != 1 + (size_t)n * in[0] * 8) bad_input("rows: wrong number of input words");
    const u32 cols = in[0];
    Dev first((size_t)n * cols * 8);
    first.up(in.data() + 1, first.n);
    std::vector<Dev*> levels;
    const u32* src = first.p;
    for (u32 m = (u32)n;;) {
        const u32 h = (m + 1) / 2;
        Dev* dst = new Dev((size_t)(h + PAD) * cols * 8);
        const size_t threads = (size_t)h * cols;
        ps::k_fr_row_pair_sums<<<(unsigned)((threads + 255) / 256), 256>>>(src, m, cols, dst->p);
        levels.push_back(dst);
        src = dst->p;
        m = h;
        if (m <= 1) break;
    }
    done_launch();
    for (Dev* d : levels) {
        const Words w = d->down();
        out.insert(out.end(), w.begin(), w.end());
        delete d;
    }
}

static void run_points(long n, const Words& in, Words& out) {
    if (in.size() < 1 || in[0] < 1 || in.size() != 1 + (size_t)in[0] * n * 24) bad_input("points: wrong number of input words");
    const u32 segs = in[0], stride = segs > 1 ? (u32)n : 0u;
    std::vector<Xyzz<Fp>> pts((size_t)segs * n);
    for (size_t i = 0; i < pts.size(); i++) {
        const u32* w = in.data() + 1 + i * 24;
        bool zero = true;
        for (int k = 0; k < 24; k++) zero = zero && w[k] == 0;
        pts[i] = zero ? xyzz_identity<Fp>() : xyzz_from_affine<Fp>(fp_to_mont(fp_from_words12(w)), fp_to_mont(fp_from_words12(w + 12)));
    }
    Dev first(pts.size() * WX);
    first.up(pts.data(), first.n);
    struct Level { Dev* d; u32 h; };
    std::vector<Level> levels;
    const Xyzz<Fp>* src = (const Xyzz<Fp>*)first.p;
    for (u32 m = (u32)n;;) {
        const u32 h = (m + 1) / 2;
        // the buffer of a level: segment s at s * stride (one segment: h nodes), PAD slots behind
        const size_t slots = (segs > 1 ? (size_t)segs * stride : h) + PAD;
        Dev* dst = new Dev(slots * WX);
        ps::k_g1_pair_sums<<<(unsigned)(((size_t)segs * h + 255) / 256), 256>>>(src, m, segs, stride, (Xyzz<Fp>*)dst->p, stride);
        levels.push_back({dst, h});
        src = (const Xyzz<Fp>*)dst->p;
        m = h;
        if (m <= 1) break;
    }
    done_launch();
    for (const Level& lv : levels) {
        const Words w = lv.d->down();
        const size_t slots = w.size() / WX;
        std::vector<char> owned(slots, 0);
        for (u32 s = 0; s < segs; s++)
            for (u32 i = 0; i < lv.h; i++) {
                const size_t slot = (size_t)s * stride + i;
                owned[slot] = 1;
                Xyzz<Fp> p;
                std::memcpy(&p, w.data() + slot * WX, sizeof(p));
                u32 xy[24];
                std::memset(xy, 0, sizeof(xy));
                Fp x, y;
                if (xyzz_to_affine<Fp>(p, x, y)) {
                    fp_to_words12(xy, fp_from_mont(x));
                    fp_to_words12(xy + 12, fp_from_mont(y));
                }
                out.insert(out.end(), xy, xy + 24);
            }
        u32 touched = 0;
        for (size_t slot = 0; slot < slots; slot++) {
            if (owned[slot]) continue;
            bool clean = true;
            for (size_t k = 0; k < WX; k++) clean = clean && w[slot * WX + k] == POISON;
            touched += clean ? 0 : 1;
        }
        out.push_back(touched);
        delete lv.d;
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        std::printf("rows\npoints\n");
        return 0;
    }
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s OP N IN OUT | --list\n", argv[0]);
        return 2;
    }
    const long n = std::atol(argv[2]);
    if (n <= 0 || n > (1 << 20)) bad_input("node count");
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) bad_input("cannot open the input file");
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    Words in((size_t)bytes / 4), out;
    if (bytes % 4 || std::fread(in.data(), 4, in.size(), f) != in.size()) bad_input("cannot read the input file");
    std::fclose(f);
    if (!std::strcmp(argv[1], "rows")) run_rows(n, in, out);
    else if (!std::strcmp(argv[1], "points")) run_points(n, in, out);
    else bad_input("operation");
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f)) {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    return 0;
}
