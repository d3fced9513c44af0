// device_tail_check.hip -- a test-only program (never linked into the product) that runs the tail of a sum ON THE GPU, value by
// value: the lane-quad group law q_add and the tree q_block_tree of playsnark_amd/csrc/qtail.hpp behind thin wrapper kernels
// (q_load, the call, q_store), and the shipped tail kernels k_qreduce_rowcol, k_qreduce_bits, k_qfixup, k_qfixup_chain,
// k_heavy_jobs, k_qfixup_heavy_part and k_qfixup_heavy as they stand, launched with the host's launch expressions (capi.hip,
// msm_launch_impl).  Built by tests/test_device_tail.py with the product's flags; every operation exists for Fp (G1, a quad of
// four lanes per point) and for Fp2s (G2, eight lanes).
//
//     device_tail_check OP N IN OUT
//
// IN and OUT are int32 words.  A point is an Xyzz as it lies in memory: x, y, zz, zzz, each 14 limbs (G1: PT = 56 words) or
// c0 then c1 (G2: PT = 112 words).  Every output buffer of points is poisoned (every word 0xA5A5A5A5) and PAD points longer
// than what the kernels may write; the poison comes back with the results.
//   qadd_*          IN  N x (A, B)                                        OUT (N + PAD) x PT: A + B, a quad per pair
//   qtree_*         IN  grp, N x point                                    OUT (ceil(N / grp) + PAD) x PT: the sum of every group
//                       of grp consecutive points (a short last group: the points there are)
//   rowcol_bits_*   IN  cb, s, sets, np, extra, (sets << cb) x point, and as many again if extra
//                   OUT (sets (cb + 1) + PAD) x PT, then the entry count word that rides along (poison if extra); N = sets
//   qfixup_*        IN  G, M, T, LPB, offs[G + 1], 2 T x point            N = G
//                   OUT (G + PAD) x PT buckets after k_qfixup, heavy_count, heavy_list[G + PAD]
//   qfixup_heavy_*  the same IN; OUT as qfixup_*, then (G + PAD) x PT buckets after the three heavy kernels, job_base[G + 1 + PAD]
//   qfixup_chain_*  IN  G, M, T, nchain, max_chain, offs[G + 1], chain_list[nchain], 2 T x point     N = G
//                   OUT (G + PAD) x PT
// Exit status 0 = every HIP call succeeded; the checking is the test's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../playsnark_amd/csrc/msm.hpp"
#include "../playsnark_amd/csrc/qtail.hpp"

using namespace ps;

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(3);                                                                           \
        }                                                                                           \
    } while (0)
#define NEED(c)                                                              \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::fprintf(stderr, "bad arguments: %s does not hold\n", #c);  \
            std::exit(2);                                                    \
        }                                                                    \
    } while (0)

constexpr int PAD = 4;             // elements past the end of an output buffer, which must keep the poison
constexpr int POISON_BYTE = 0xA5;  // every word 0xA5A5A5A5: no limb of a result, no index of a list

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
    void up(const i32* src, size_t words) {
        NEED(words <= n);
        if (words) HIP_OK(hipMemcpy(p, src, words * sizeof(i32), hipMemcpyHostToDevice));
    }
    void down(Words& out) const {
        const size_t at = out.size();
        out.resize(at + n);
        if (n) HIP_OK(hipMemcpy(out.data() + at, p, n * sizeof(i32), hipMemcpyDeviceToHost));
    }
};
static void sync() {
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
}
static unsigned nblocks(size_t threads) { return (unsigned)((threads + 255) / 256); }

// ---- the wrapper kernels: q_load, the call, q_store ----
// Quads past the last case work on the last case, so that every lane a DPP move or a ballot reads is live; only their stores
// are masked.
template <class KF>
__global__ void __launch_bounds__(256) k_qadd(const Xyzz<typename FieldTraits<KF>::Store>* __restrict__ in,
                                              Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out, u32 n) {
    constexpr u32 GL = QTraits<KF>::GL;
    const u32 pt = blockIdx.x * (256 / GL) + threadIdx.x / GL;
    const u32 c = pt < n ? pt : n - 1;
    KF a = q_load<KF>(&in[2 * (size_t)c]);
    const KF b = q_load<KF>(&in[2 * (size_t)c + 1]);
    q_add<KF>(a, b);
    if (pt < n) q_store<KF>(&out[pt], a);
}
// points past the end are the identity
template <class KF>
__global__ void __launch_bounds__(256) k_qtree(const Xyzz<typename FieldTraits<KF>::Store>* __restrict__ in,
                                               Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out, u32 n, u32 grp) {
    constexpr u32 GL = QTraits<KF>::GL;
    __shared__ Fp sm[256];
    const u32 lp = threadIdx.x / GL;
    const u32 pt = blockIdx.x * (256 / GL) + lp;
    KF mine = f_zero((const KF*)0);
    if (pt < n) mine = q_load<KF>(&in[pt]);
    q_block_tree<KF>(sm, mine, lp, grp);
    if (pt < n && (pt & (grp - 1)) == 0) q_store<KF>(&out[pt / grp], mine);
}

template <class KF>
struct G {
    typedef typename FieldTraits<KF>::Store St;
    typedef Xyzz<St> Pt;
    static constexpr u32 GL = QTraits<KF>::GL, NPB = 256 / GL;
    static constexpr size_t PT = sizeof(Pt) / sizeof(i32);
    static_assert(sizeof(Pt) == 4 * sizeof(St) && sizeof(St) == FieldTraits<KF>::LANES * FP_L * sizeof(i32), "a point is plain limbs");

    static Words qadd(const Words& in, long n) {
        NEED(in.size() == (size_t)n * 2 * PT);
        Dev din(in.size()), dout((size_t)(n + PAD) * PT);
        din.up(in.data(), in.size());
        k_qadd<KF><<<nblocks((size_t)n * GL), 256>>>((const Pt*)din.p, (Pt*)dout.p, (u32)n);
        sync();
        Words out;
        dout.down(out);
        return out;
    }

    static Words qtree(const Words& in, long n) {
        NEED(in.size() == 1 + (size_t)n * PT);
        const u32 grp = (u32)in[0];
        NEED(grp >= 1 && grp <= NPB && (grp & (grp - 1)) == 0);
        const size_t groups = ((size_t)n + grp - 1) / grp;
        Dev din((size_t)n * PT), dout((groups + PAD) * PT);
        din.up(in.data() + 1, (size_t)n * PT);
        k_qtree<KF><<<nblocks((size_t)n * GL), 256>>>((const Pt*)din.p, (Pt*)dout.p, (u32)n, grp);
        sync();
        Words out;
        dout.down(out);
        return out;
    }

    // capi.hip, msm_launch_impl: the reduction of pl.qtail plans (extra = 0) and of the long sums' hybrid tail (extra = 1),
    // with the block size in quads (np) handed in: the host picks a power of two from 64 / GL to 512 / GL (256 / GL: hybrid)
    static Words rowcol_bits(const Words& in, long sets) {
        NEED(in.size() >= 5);
        const int cb = in[0], s = in[1];
        const u32 np = (u32)in[3];
        const bool extra = in[4] != 0;
        NEED(in[2] == sets && sets >= 1 && sets <= 64 && cb >= 1 && cb <= 16 && s >= 0 && s <= cb);
        NEED(np >= 64 / GL && np <= (extra ? 256u : 512u) / GL && (np & (np - 1)) == 0);
        NEED(!extra || s > 0);
        const size_t nb = (size_t)sets << cb;
        NEED(in.size() == 5 + nb * PT * (extra ? 2 : 1));
        const u32 rows = 1u << (cb - s), cols = 1u << s;
        const u32 nres = (u32)sets * (u32)(cb + 1);
        Dev buckets(nb * PT), second(extra ? nb * PT : 0), R((size_t)sets * rows * PT), C((size_t)sets * cols * PT),
            R2(extra ? (size_t)sets * rows * PT : 0), wins((size_t)(nres + PAD) * PT), esrc(1), edst(1);
        buckets.up(in.data() + 5, nb * PT);
        if (extra) second.up(in.data() + 5 + nb * PT, nb * PT);
        const i32 entries = 0x1234567;
        esrc.up(&entries, 1);
        if (s > 0)
            hipLaunchKernelGGL(k_qreduce_rowcol<KF>, dim3(((extra ? 2 : 1) * rows + cols) * (u32)sets), dim3(np * GL), np * GL * sizeof(Fp), 0,
                               (const Pt*)buckets.p, cb, s, (Pt*)R.p, (Pt*)C.p, extra ? (const Pt*)second.p : (const Pt*)nullptr,
                               extra ? (Pt*)R2.p : (Pt*)nullptr);
        hipLaunchKernelGGL(k_qreduce_bits<KF>, dim3(nres), dim3(np * GL), np * GL * sizeof(Fp), 0,
                           s > 0 ? (const Pt*)R.p : (const Pt*)buckets.p, (const Pt*)C.p, cb, s, (Pt*)wins.p,
                           extra ? (const u32*)nullptr : (const u32*)esrc.p, extra ? (u32*)nullptr : (u32*)edst.p,
                           extra ? (const Pt*)R2.p : (const Pt*)nullptr);
        sync();
        Words out;
        wins.down(out);
        edst.down(out);
        return out;
    }

    // the offsets of a fix-up case, checked before any kernel reads through them
    static void check_offs(const i32* offs, u32 Gn, int M, u32 T) {
        NEED(offs[0] == 0 && M >= 1 && T >= 1);
        for (u32 g = 0; g < Gn; g++) NEED(offs[g] <= offs[g + 1]);
        const u32 E = (u32)offs[Gn];
        NEED(E >= 1 && (E + (u32)M - 1) / (u32)M <= T);  // every slice of the list has its two slots
        NEED(eff_slice(E, T, M) == M);                    // the slice length the kernels derive is the one handed in
    }

    static Words qfixup(const Words& in, long Gl, bool heavy) {
        NEED(in.size() >= 4);
        const u32 Gn = (u32)Gl, T = (u32)in[2], LPB = (u32)in[3];
        const int M = in[1];
        NEED(in[0] == Gl && Gn >= 1 && Gn <= (1u << 16) && T <= (1u << 20));
        NEED(LPB >= 1 && LPB <= NPB && (LPB & (LPB - 1)) == 0);
        NEED(in.size() == 4 + (size_t)Gn + 1 + 2 * (size_t)T * PT);
        const i32* offs = in.data() + 4;
        check_offs(offs, Gn, M, T);
        Dev doffs(Gn + 1), parts(2 * (size_t)T * PT), buckets((size_t)(Gn + PAD) * PT), hcount(1), hlist(Gn + PAD), job_base(Gn + 1 + PAD),
            hparts(((size_t)T + Gn + 1) * PT);
        doffs.up(offs, Gn + 1);
        parts.up(offs + Gn + 1, 2 * (size_t)T * PT);
        HIP_OK(hipMemset(hcount.p, 0, sizeof(i32)));
        hipLaunchKernelGGL(k_qfixup<KF>, dim3(nblocks((size_t)Gn * LPB * GL)), dim3(256), 0, 0, (const u32*)doffs.p, Gn, M, T, LPB,
                           (const Pt*)parts.p, (Pt*)buckets.p, (u32*)hcount.p, (u32*)hlist.p, (const u32*)nullptr);
        sync();
        Words out;
        buckets.down(out);
        hcount.down(out);
        hlist.down(out);
        if (!heavy) return out;
        hipLaunchKernelGGL(k_heavy_jobs, dim3(1), dim3(256), 0, 0, (const u32*)doffs.p, Gn, M, T, (const u32*)hcount.p, (const u32*)hlist.p,
                           (u32*)job_base.p, NPB, (const u32*)nullptr);
        hipLaunchKernelGGL(k_qfixup_heavy_part<KF>, dim3(1024), dim3(256), 0, 0, (const u32*)doffs.p, Gn, M, T, (const Pt*)parts.p,
                           (const u32*)hcount.p, (const u32*)hlist.p, (const u32*)job_base.p, (Pt*)hparts.p, (const u32*)nullptr);
        hipLaunchKernelGGL(k_qfixup_heavy<KF>, dim3(256), dim3(256), 0, 0, (const Pt*)hparts.p, (Pt*)buckets.p, (const u32*)hcount.p,
                           (const u32*)hlist.p, (const u32*)job_base.p, (const u32*)nullptr);
        sync();
        buckets.down(out);
        job_base.down(out);
        return out;
    }
    static Words qfixup_plain(const Words& in, long n) { return qfixup(in, n, false); }
    static Words qfixup_heavy(const Words& in, long n) { return qfixup(in, n, true); }

    static Words qfixup_chain(const Words& in, long Gl) {
        NEED(in.size() >= 5);
        const u32 Gn = (u32)Gl, T = (u32)in[2], nchain = (u32)in[3], max_chain = (u32)in[4];
        const int M = in[1];
        NEED(in[0] == Gl && Gn >= 1 && Gn <= (1u << 16) && T <= (1u << 20) && nchain <= Gn && max_chain >= 1);
        NEED(in.size() == 5 + (size_t)Gn + 1 + nchain + 2 * (size_t)T * PT);
        const i32* offs = in.data() + 5;
        check_offs(offs, Gn, M, T);
        const i32* list = offs + Gn + 1;
        for (u32 h = 0; h < nchain; h++) NEED(list[h] >= 0 && (u32)list[h] < Gn && offs[list[h]] < offs[list[h] + 1]);
        Dev doffs(Gn + 1), dlist(nchain), parts(2 * (size_t)T * PT), buckets((size_t)(Gn + PAD) * PT), count(1);
        doffs.up(offs, Gn + 1);
        dlist.up(list, nchain);
        parts.up(list + nchain, 2 * (size_t)T * PT);
        const i32 cnt = (i32)nchain;
        count.up(&cnt, 1);
        hipLaunchKernelGGL(k_qfixup_chain<KF>, dim3((unsigned)std::min<size_t>(((size_t)max_chain + NPB - 1) / NPB, 512)), dim3(256), 0, 0,
                           (const u32*)doffs.p, Gn, M, T, (const Pt*)parts.p, (Pt*)buckets.p, (const u32*)count.p, (const u32*)dlist.p,
                           (const u32*)nullptr);
        sync();
        Words out;
        buckets.down(out);
        return out;
    }
};

struct Entry {
    const char* name;
    Words (*run)(const Words&, long);
};
#define BOTH(NAME, FN) {NAME "_g1", G<Fp>::FN}, {NAME "_g2", G<Fp2s>::FN}
static const Entry kEntries[] = {
    BOTH("qadd", qadd), BOTH("qtree", qtree), BOTH("rowcol_bits", rowcol_bits), BOTH("qfixup", qfixup_plain),
    BOTH("qfixup_heavy", qfixup_heavy), BOTH("qfixup_chain", qfixup_chain),
};

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        for (const Entry& e : kEntries) std::printf("%s\n", e.name);
        std::printf("pad %d pt_g1 %zu pt_g2 %zu quads_g1 %u quads_g2 %u qfix_heavy %u\n", PAD, G<Fp>::PT, G<Fp2s>::PT, G<Fp>::NPB, G<Fp2s>::NPB,
                    QFIX_HEAVY);
        return 0;
    }
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s OP N IN OUT | --list\n", argv[0]);
        return 2;
    }
    const Entry* ent = nullptr;
    for (const Entry& e : kEntries)
        if (!std::strcmp(e.name, argv[1])) ent = &e;
    const long n = std::atol(argv[2]);
    if (!ent || n <= 0 || n > (1 << 20)) {
        std::fprintf(stderr, "bad operation or case count\n");
        return 2;
    }
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[3]);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    Words in((size_t)bytes / sizeof(i32));
    if (bytes % 4 || std::fread(in.data(), sizeof(i32), in.size(), f) != in.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[3]);
        return 2;
    }
    std::fclose(f);
    const Words out = ent->run(in, n);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), sizeof(i32), out.size(), f) != out.size()) {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    std::fclose(f);
    return 0;
}
