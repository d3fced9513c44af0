// device_field_check.hip -- a test-only program (never linked into the product) that runs the field arithmetic of
// playsnark_amd/csrc/field.hpp ON THE GPU, as the product's kernels compile it: the generated multiply-add chains of
// fp_chain.inc / fr_chain.inc, the lane-pair Fp2 (Fp2s) with its DPP moves, the noinline products.  Built by
// tests/test_device_field.py with the product's flags, once as-is and once with -DPS_FP_MUL_NO_CHAIN -DPS_FR_MUL_NO_CHAIN
// (the C++ forms compiled for the device).
//
//     device_field_check OP N IN OUT
//
// reads N cases of OP's input (int32 words, the layout below) from IN, runs one GPU thread per case (one lane PAIR per case
// for the Fp2s operations: lane 2c + e holds component e), writes the raw result words to OUT.  Launches are padded to whole
// waves: padding lanes compute on the last case, so that every DPP partner is live, and only the stores are masked.
// Exit status 0 = ran; the checking is the test's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../playsnark_amd/csrc/curve.hpp"
#include "../playsnark_amd/csrc/ntt.hpp"

using namespace ps;

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(3);                                                                           \
        }                                                                                           \
    } while (0)

// ---- loads and stores of one case ----
__device__ inline Fp ld_fp(const i32* p) {
    Fp r;
#pragma unroll
    for (int i = 0; i < FP_L; i++) r.l[i] = p[i];
    return r;
}
__device__ inline void st_fp(i32* o, const Fp& a) {
#pragma unroll
    for (int i = 0; i < FP_L; i++) o[i] = a.l[i];
}
__device__ inline Fr ld_fr(const i32* p) {
    Fr r;
#pragma unroll
    for (int i = 0; i < FR_L; i++) r.l[i] = p[i];
    return r;
}
__device__ inline void st_fr(i32* o, const Fr& a) {
#pragma unroll
    for (int i = 0; i < FR_L; i++) o[i] = a.l[i];
}
__device__ inline Fp2 ld_fp2(const i32* p) { return Fp2{ld_fp(p), ld_fp(p + FP_L)}; }
__device__ inline void st_fp2(i32* o, const Fp2& a) { st_fp(o, a.c0); st_fp(o + FP_L, a.c1); }
// operand k of an Fp2s case: the inputs are whole Fp2 elements (c0 then c1); this lane takes its component
__device__ inline Fp2s ld_fp2s(const i32* p, int k) { return Fp2s{ld_fp(p + 2 * FP_L * k + FP_L * pair_lane())}; }
template <class P>
__device__ inline Fe<P> ld_fe(const i32* p) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < P::N; i++) r.l[i] = (u32)p[i];
    return r;
}
template <class P>
__device__ inline void st_fe(i32* o, const Fe<P>& a) {
#pragma unroll
    for (int i = 0; i < P::N; i++) o[i] = (i32)a.l[i];
}

// ---- the operations: IN words per case, OUT words per thread, PAIR = one lane pair per case ----
#define OP(NAME, IN_, OUT_, PAIR_, ...)                                         \
    struct NAME {                                                               \
        static constexpr int IN = IN_, OUT = OUT_;                              \
        static constexpr bool PAIR = PAIR_;                                     \
        __device__ static void run(const i32* in, i32* o) { __VA_ARGS__; }      \
    };
#define A(k) ld_fp(in + FP_L * (k))
#define Q(k) ld_fp2s(in, k)
#define F(k) ld_fr(in + FR_L * (k))

OP(OpFpMul, 28, 14, false, st_fp(o, f_mul(A(0), A(1))))
OP(OpFpSqr, 14, 14, false, st_fp(o, f_sqr(A(0))))
OP(OpFpMul2sub, 56, 14, false, st_fp(o, f_mul2sub(A(0), A(1), A(2), A(3))))
OP(OpFpMul2add, 56, 14, false, st_fp(o, f_mul2add(A(0), A(1), A(2), A(3))))
OP(OpFpMul2add2sub, 112, 14, false, st_fp(o, f_mul2add2sub(A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7))))
OP(OpFpMulIlp, 28, 14, false, st_fp(o, f_mul_ilp(A(0), A(1))))
OP(OpFpMul2subIlp, 56, 14, false, st_fp(o, f_mul2sub_ilp(A(0), A(1), A(2), A(3))))
OP(OpFpMulsumIlp4, 112, 14, false, {
    const Fp x[4] = {A(0), A(2), A(4), A(6)}, y[4] = {A(1), A(3), A(5), A(7)};
    const bool neg[4] = {false, false, true, true};
    st_fp(o, f_mulsum_ilp<4>(x, y, neg));
})
OP(OpFpMulCall, 28, 14, false, st_fp(o, fp_mul_call(A(0), A(1))))
OP(OpFpSqrCall, 14, 14, false, st_fp(o, fp_sqr_call(A(0))))
OP(OpFpNorm, 14, 14, false, st_fp(o, f_norm(A(0))))
OP(OpFpPropagate, 14, 14, false, st_fp(o, fp_propagate(A(0))))
OP(OpFpCanon, 14, 14, false, st_fp(o, fp_canon(A(0))))
OP(OpFpIsZero, 14, 1, false, o[0] = f_is_zero(A(0)) ? 1 : 0)
OP(OpFpIsZeroExact, 14, 1, false, o[0] = fp_is_zero_exact(A(0)) ? 1 : 0)
OP(OpFpToMont, 14, 14, false, st_fp(o, fp_to_mont(A(0))))
OP(OpFpFromMont, 14, 14, false, st_fp(o, fp_from_mont(A(0))))
OP(OpFp2Mul, 56, 28, false, st_fp2(o, f_mul(ld_fp2(in), ld_fp2(in + 2 * FP_L))))
OP(OpFp2Sqr, 28, 28, false, st_fp2(o, f_sqr(ld_fp2(in))))
OP(OpFp2sMul, 56, 14, true, st_fp(o, f_mul(Q(0), Q(1)).v))
OP(OpFp2sSqr, 28, 14, true, st_fp(o, f_sqr(Q(0)).v))
OP(OpFp2sMul2sub, 112, 14, true, st_fp(o, f_mul2sub(Q(0), Q(1), Q(2), Q(3)).v))
OP(OpFp2sMulIlp, 56, 14, true, st_fp(o, f_mul_ilp(Q(0), Q(1)).v))
OP(OpFp2sMul2subIlp, 112, 14, true, st_fp(o, f_mul2sub_ilp(Q(0), Q(1), Q(2), Q(3)).v))
OP(OpFp2sIsZero, 28, 1, true, o[0] = f_is_zero(Q(0)) ? 1 : 0)
OP(OpFrMul, 20, 10, false, st_fr(o, fr_mul(F(0), F(1))))
OP(OpFrReduce, 10, 10, false, st_fr(o, fr_reduce(F(0))))
OP(OpFrNorm, 10, 10, false, st_fr(o, fr_norm(F(0))))
OP(OpFrPropagate, 10, 10, false, st_fr(o, fr_propagate(F(0))))
OP(OpFrCanon, 10, 10, false, st_fr(o, fr_canon(F(0))))
OP(OpFeMulFp, 24, 12, false, st_fe<FpParams>(o, fe_mul<FpParams>(ld_fe<FpParams>(in), ld_fe<FpParams>(in + 12))))
OP(OpFeAddFp, 24, 12, false, st_fe<FpParams>(o, fe_add<FpParams>(ld_fe<FpParams>(in), ld_fe<FpParams>(in + 12))))
OP(OpFeSubFp, 24, 12, false, st_fe<FpParams>(o, fe_sub<FpParams>(ld_fe<FpParams>(in), ld_fe<FpParams>(in + 12))))
OP(OpFeMulFr, 16, 8, false, st_fe<FrParams>(o, fe_mul<FrParams>(ld_fe<FrParams>(in), ld_fe<FrParams>(in + 8))))
OP(OpFeAddFr, 16, 8, false, st_fe<FrParams>(o, fe_add<FrParams>(ld_fe<FrParams>(in), ld_fe<FrParams>(in + 8))))
OP(OpFeSubFr, 16, 8, false, st_fe<FrParams>(o, fe_sub<FrParams>(ld_fe<FrParams>(in), ld_fe<FrParams>(in + 8))))

// ---- the group law: a bucket's life (host_limb_check.cpp, test_group_law) ----
// Input: GL_K affine points (x, y), canonical Montgomery form (Fp: 28 words a point; Fp2s: 56, whole Fp2 elements).
// acc takes every point through xyzz_madd_inl; left the first half, right the second; then left += right (xyzz_add_inl) and
// dbl = 2 acc (xyzz_dbl_inl).  Output (per lane): acc, left, dbl as X, Y, ZZ, ZZZ, then the largest limb class of every
// coordinate stored in acc / left / right along the way.
constexpr int GL_K = 40;
__device__ inline int cls_of(const Fp& a) {
    u32 m = 0;
#pragma unroll
    for (int i = 0; i < FP_L; i++) {
        const u32 v = a.l[i] < 0 ? (u32)(-(i64)a.l[i]) : (u32)a.l[i];
        m = v > m ? v : m;
    }
    return (int)(m >> 28) + 1;
}
__device__ inline int cls_of(const Fp2s& a) { return cls_of(a.v); }
template <class F>
__device__ inline int xyzz_cls(const Xyzz<F>& p) {
    const int a = cls_of(p.x), b = cls_of(p.y), c = cls_of(p.zz), d = cls_of(p.zzz);
    return max(max(a, b), max(c, d));
}
__device__ inline Fp gl_ld(const i32* p, const Fp*) { return ld_fp(p); }
__device__ inline Fp2s gl_ld(const i32* p, const Fp2s*) { return Fp2s{ld_fp(p + FP_L * pair_lane())}; }
__device__ inline void gl_st(i32* o, const Fp& a) { st_fp(o, a); }
__device__ inline void gl_st(i32* o, const Fp2s& a) { st_fp(o, a.v); }
template <class F>
struct IsPair { static constexpr bool value = false; };
template <>
struct IsPair<Fp2s> { static constexpr bool value = true; };
template <class F>
struct OpGroupLaw {
    static constexpr bool PAIR = IsPair<F>::value;
    static constexpr int W = PAIR ? 4 * FP_L : 2 * FP_L;  // input words a point
    static constexpr int IN = GL_K * W, OUT = 12 * FP_L + 1;
    __device__ static void run(const i32* in, i32* o) {
        Xyzz<F> acc = xyzz_identity<F>(), left = xyzz_identity<F>(), right = xyzz_identity<F>();
        int worst = 0;
        for (int i = 0; i < GL_K; i++) {
            const F x = gl_ld(in + W * i, (const F*)0), y = gl_ld(in + W * i + W / 2, (const F*)0);
            xyzz_madd_inl<F>(acc, x, y);
            if (i < GL_K / 2) xyzz_madd_inl<F>(left, x, y);
            else xyzz_madd_inl<F>(right, x, y);
            worst = max(worst, max(xyzz_cls(acc), max(xyzz_cls(left), xyzz_cls(right))));
        }
        xyzz_add_inl<F>(left, right);
        worst = max(worst, xyzz_cls(left));
        const Xyzz<F> dbl = xyzz_dbl_inl<F>(acc);
        worst = max(worst, xyzz_cls(dbl));
        const Xyzz<F>* outs[3] = {&acc, &left, &dbl};
        for (int j = 0; j < 3; j++) {
            gl_st(o + FP_L * (4 * j + 0), outs[j]->x);
            gl_st(o + FP_L * (4 * j + 1), outs[j]->y);
            gl_st(o + FP_L * (4 * j + 2), outs[j]->zz);
            gl_st(o + FP_L * (4 * j + 3), outs[j]->zzz);
        }
        o[12 * FP_L] = worst;
    }
};

// ---- generic launch: one thread (or lane pair) per case, padded to whole waves, stores masked ----
template <class Op>
__global__ void __launch_bounds__(64) k_case(const i32* __restrict__ in, i32* __restrict__ out, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = Op::PAIR ? t >> 1 : t;
    const bool live = c < n;
    const int cc = live ? c : n - 1;
    i32 res[Op::OUT];
    Op::run(in + (size_t)cc * Op::IN, res);
    if (live) {
        for (int i = 0; i < Op::OUT; i++) out[(size_t)t * Op::OUT + i] = res[i];
    }
}

// ---- the NTT butterflies as the shipped pass kernel runs them (ntt.hpp: ntt_tile_stages, the store of k_ntt_pass) ----
// One workgroup per case holds a tile of NB_TILE elements in LDS and runs a sequence of passes over it; pass j is a batch of
// 2^logCols transforms of 2^k points (p = k, logD = 0), followed by k_ntt_pass's store: a product with 2^-scale_log for the
// inverse where ntt_run asks for it.  Repeating passes on the same tile stands for the passes of a deep transform: what
// reaches each pass is what the previous pass stored.
// Input: NB_HDR words (npass, then k, logCols, scale_log per pass), the compact twiddle table (NB_TILE Fr, tw[(1 << M) + blk]),
// the tile (NB_TILE Fr).  Output: the tile.
constexpr int NB_TILE = 512, NB_MAXPASS = 8, NB_HDR = 1 + 3 * NB_MAXPASS;
constexpr int NB_IN = NB_HDR + 2 * NB_TILE * FR_L, NB_OUT = NB_TILE * FR_L;
template <bool INV>
__global__ void __launch_bounds__(256) k_ntt_replay(const i32* __restrict__ in, i32* __restrict__ out) {
    __shared__ Fr tile[NB_TILE];
    const i32* hdr = in + (size_t)blockIdx.x * NB_IN;
    const Fr* tw = reinterpret_cast<const Fr*>(hdr + NB_HDR);
    const Fr* data = tw + NB_TILE;
    for (int e = threadIdx.x; e < NB_TILE; e += blockDim.x) tile[PS_NTT_SW((u32)e)] = data[e];
    __syncthreads();
    const int npass = hdr[0];
    for (int j = 0; j < npass; j++) {
        const int k = hdr[1 + 3 * j], logCols = hdr[2 + 3 * j], scale_log = hdr[3 + 3 * j];
        const NttTile g{k, 0, k, logCols, 0};
        ntt_tile_stages<INV>(tile, g, tw, k);
        if (INV && scale_log) {
            Fr sc;
#pragma unroll
            for (int i = 0; i < FR_L; i++) sc.l[i] = c_fr_inv2pow[scale_log][i];
            for (int e = threadIdx.x; e < (1 << (k + logCols)); e += blockDim.x) {
                const u32 s = PS_NTT_SW((u32)e);
                tile[s] = fr_mul(tile[s], sc);
            }
        }
        __syncthreads();
    }
    Fr* dst = reinterpret_cast<Fr*>(out + (size_t)blockIdx.x * NB_OUT);
    for (int e = threadIdx.x; e < NB_TILE; e += blockDim.x) dst[e] = tile[PS_NTT_SW((u32)e)];
}

// ---- host side ----
struct Entry {
    const char* name;
    int in, out;  // words per case (out: per case, both lanes for a pair)
    void (*launch)(const i32*, i32*, int);
};
template <class Op>
static void launch_case(const i32* in, i32* out, int n) {
    const int threads = (Op::PAIR ? 2 : 1) * n;
    k_case<Op><<<(threads + 63) / 64, 64>>>(in, out, n);
}
template <bool INV>
static void launch_ntt(const i32* in, i32* out, int n) { k_ntt_replay<INV><<<n, 256>>>(in, out); }
#define E(NAME, OPT) {NAME, OPT::IN, (OPT::PAIR ? 2 : 1) * OPT::OUT, launch_case<OPT>}
static const Entry kEntries[] = {
    E("fp_mul", OpFpMul), E("fp_sqr", OpFpSqr), E("fp_mul2sub", OpFpMul2sub), E("fp_mul2add", OpFpMul2add),
    E("fp_mul2add2sub", OpFpMul2add2sub), E("fp_mul_ilp", OpFpMulIlp), E("fp_mul2sub_ilp", OpFpMul2subIlp),
    E("fp_mulsum_ilp4", OpFpMulsumIlp4), E("fp_mul_call", OpFpMulCall), E("fp_sqr_call", OpFpSqrCall), E("fp_norm", OpFpNorm),
    E("fp_propagate", OpFpPropagate), E("fp_canon", OpFpCanon), E("fp_is_zero", OpFpIsZero),
    E("fp_is_zero_exact", OpFpIsZeroExact), E("fp_to_mont", OpFpToMont), E("fp_from_mont", OpFpFromMont),
    E("fp2_mul", OpFp2Mul), E("fp2_sqr", OpFp2Sqr), E("fp2s_mul", OpFp2sMul), E("fp2s_sqr", OpFp2sSqr),
    E("fp2s_mul2sub", OpFp2sMul2sub), E("fp2s_mul_ilp", OpFp2sMulIlp), E("fp2s_mul2sub_ilp", OpFp2sMul2subIlp),
    E("fp2s_is_zero", OpFp2sIsZero), E("fr_mul", OpFrMul), E("fr_reduce", OpFrReduce), E("fr_norm", OpFrNorm),
    E("fr_propagate", OpFrPropagate), E("fr_canon", OpFrCanon), E("fe_mul_fp", OpFeMulFp), E("fe_add_fp", OpFeAddFp),
    E("fe_sub_fp", OpFeSubFp), E("fe_mul_fr", OpFeMulFr), E("fe_add_fr", OpFeAddFr), E("fe_sub_fr", OpFeSubFr),
    E("group_law_g1", OpGroupLaw<Fp>), E("group_law_g2", OpGroupLaw<Fp2s>),
    {"ntt_forward", NB_IN, NB_OUT, launch_ntt<false>}, {"ntt_inverse", NB_IN, NB_OUT, launch_ntt<true>},
};

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        for (const Entry& e : kEntries) std::printf("%s %d %d\n", e.name, e.in, e.out);
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
    std::vector<i32> h_in((size_t)n * ent->in), h_out((size_t)n * ent->out, 0);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(h_in.data(), sizeof(i32), h_in.size(), f) != h_in.size()) {
        std::fprintf(stderr, "cannot read %zu words from %s\n", h_in.size(), argv[3]);
        return 2;
    }
    std::fclose(f);
    i32 *d_in = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc(&d_in, h_in.size() * sizeof(i32)));
    HIP_OK(hipMalloc(&d_out, h_out.size() * sizeof(i32)));
    HIP_OK(hipMemcpy(d_in, h_in.data(), h_in.size() * sizeof(i32), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0, h_out.size() * sizeof(i32)));
    ent->launch(d_in, d_out, (int)n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h_out.data(), d_out, h_out.size() * sizeof(i32), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(h_out.data(), sizeof(i32), h_out.size(), f) != h_out.size()) {
        std::fprintf(stderr, "cannot write %s\n", argv[4]);
        return 2;
    }
    std::fclose(f);
    return 0;
}
