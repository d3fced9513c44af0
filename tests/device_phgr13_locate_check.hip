// device_phgr13_locate_check.hip -- a test-only program (never linked into the product) that launches the two kernels of the
// locating PHGR13 batch verifier ON THE GPU as the product compiles them: ps::k_g2_pair_sums and ps::k_f12_segment_products of
// playsnark_amd/csrc/locate_phgr13_dev.hpp, every output into a poisoned, padded buffer of its own.  Built by
// tests/test_device_phgr13_locate.py with the product's flags; the headers are included unmodified.
//
//     device_phgr13_locate_check OP N IN OUT
//
// IN and OUT are raw 32-bit words.
//   g2points  IN  segs, then segs x N x 48 words (x.c0, x.c1, y.c0, y.c1 canonical plain words; all zero = the identity)
//             OUT per level (n -> h = ceil(n / 2) until 1; one level 1 -> 1 for N = 1): segs x h x 48 words (the nodes
//                 normalised on the host: affine, canonical, plain; zero = identity), then ONE word: the slots of the level's
//                 buffer no node owns that no longer hold the poison.
//                 segs = 1 runs with strides 0 as the wss tree does, segs > 1 with the segment stride N.
//   segprod   N = segs.  IN len, has_first, lpw, then (has_first ? N x 168 : 0) and N x len x 168 raw limbs
//             OUT (N + PAD) x 168 words as the device left them (buffer poisoned beforehand)
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
#include "../playsnark_amd/csrc/locate_phgr13_dev.hpp"

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
constexpr size_t WX2 = sizeof(Xyzz<Fp2>) / 4, W12 = sizeof(pairing_dev::Fp12) / 4;
static_assert(W12 == 12 * FP_L, "an Fp12 is plain limbs");

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

static Fp2 fp2_of_words(const u32* w) { return Fp2{fp_to_mont(fp_from_words12(w)), fp_to_mont(fp_from_words12(w + 12))}; }

static void run_g2points(long n, const Words& in, Words& out) {
    if (in.size() < 1 || in[0] < 1 || in.size() != 1 + (size_t)in[0] * n * 48) bad_input("g2points: wrong number of input words");
    const u32 segs = in[0], stride = segs > 1 ? (u32)n : 0u;
    std::vector<Xyzz<Fp2>> pts((size_t)segs * n);
    for (size_t i = 0; i < pts.size(); i++) {
        const u32* w = in.data() + 1 + i * 48;
        bool zero = true;
        for (int k = 0; k < 48; k++) zero = zero && w[k] == 0;
        pts[i] = zero ? xyzz_identity<Fp2>() : xyzz_from_affine<Fp2>(fp2_of_words(w), fp2_of_words(w + 24));
    }
    Dev first(pts.size() * WX2);
    first.up(pts.data(), first.n);
    struct Level { Dev* d; u32 h; };
    std::vector<Level> levels;
    const Xyzz<Fp2>* src = (const Xyzz<Fp2>*)first.p;
    for (u32 m = (u32)n;;) {
        const u32 h = (m + 1) / 2;
        // the buffer of a level: segment s at s * stride (one segment: h nodes), PAD slots behind
        const size_t slots = (segs > 1 ? (size_t)segs * stride : h) + PAD;
        Dev* dst = new Dev(slots * WX2);
        ps::k_g2_pair_sums<<<(unsigned)((2 * (size_t)segs * h + 255) / 256), 256>>>(src, m, segs, stride, (Xyzz<Fp2>*)dst->p, stride);
        levels.push_back({dst, h});
        src = (const Xyzz<Fp2>*)dst->p;
        m = h;
        if (m <= 1) break;
    }
    done_launch();
    for (const Level& lv : levels) {
        const Words w = lv.d->down();
        const size_t slots = w.size() / WX2;
        std::vector<char> owned(slots, 0);
        for (u32 s = 0; s < segs; s++)
            for (u32 i = 0; i < lv.h; i++) {
                const size_t slot = (size_t)s * stride + i;
                owned[slot] = 1;
                Xyzz<Fp2> p;
                std::memcpy(&p, w.data() + slot * WX2, sizeof(p));
                u32 xy[48];
                std::memset(xy, 0, sizeof(xy));
                Fp2 x, y;
                if (xyzz_to_affine<Fp2>(p, x, y)) {
                    fp_to_words12(xy, fp_from_mont(x.c0));
                    fp_to_words12(xy + 12, fp_from_mont(x.c1));
                    fp_to_words12(xy + 24, fp_from_mont(y.c0));
                    fp_to_words12(xy + 36, fp_from_mont(y.c1));
                }
                out.insert(out.end(), xy, xy + 48);
            }
        u32 touched = 0;
        for (size_t slot = 0; slot < slots; slot++) {
            if (owned[slot]) continue;
            bool clean = true;
            for (size_t k = 0; k < WX2; k++) clean = clean && w[slot * WX2 + k] == POISON;
            touched += clean ? 0 : 1;
        }
        out.push_back(touched);
        delete lv.d;
    }
}

static void run_segprod(long segs, const Words& in, Words& out) {
    if (in.size() < 3) bad_input("segprod: no header");
    const u32 len = in[0], has_first = in[1], lpw = in[2];
    if (has_first > 1 || lpw < 1 || lpw > 64 || len > 4096) bad_input("segprod: header");
    const size_t nf = has_first ? (size_t)segs * W12 : 0, ni = (size_t)segs * len * W12;
    if (in.size() != 3 + nf + ni) bad_input("segprod: wrong number of input words");
    Dev first(nf), fac(ni), res(((size_t)segs + PAD) * W12);
    if (nf) first.up(in.data() + 3, nf);
    if (ni) fac.up(in.data() + 3 + nf, ni);
    ps::k_f12_segment_products<<<(unsigned)((segs + lpw - 1) / lpw), 64>>>(has_first ? (const pairing_dev::Fp12*)first.p : nullptr, (const pairing_dev::Fp12*)fac.p,
                                                                          (u32)segs, len, lpw, (pairing_dev::Fp12*)res.p);
    done_launch();
    out = res.down();
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        std::printf("g2points\nsegprod\n");
        return 0;
    }
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s OP N IN OUT | --list\n", argv[0]);
        return 2;
    }
    const long n = std::atol(argv[2]);
    if (n <= 0 || n > (1 << 16)) bad_input("node count");
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) bad_input("cannot open the input file");
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    Words in((size_t)bytes / 4), out;
    if (bytes % 4 || std::fread(in.data(), 4, in.size(), f) != in.size()) bad_input("cannot read the input file");
    std::fclose(f);
    if (!std::strcmp(argv[1], "g2points")) run_g2points(n, in, out);
    else if (!std::strcmp(argv[1], "segprod")) run_segprod(n, in, out);
    else bad_input("operation");
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size() || std::fclose(f)) {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    return 0;
}
