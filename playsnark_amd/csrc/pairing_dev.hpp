// Device side of the batch verifier (verify_batch.inc): Miller loops of many pairs at once, the product of their
// values, and the weighted column sums of the public inputs.  Included by capi.hip after pairing.inc, and -- its PS_HD
// helpers only -- by tests/host_pairing_batch_check.cpp, which drives them on the host with the lanes emulated by a loop.
// tests/device_pairing_check.hip includes it whole and launches these kernels on the device, any lane layout, next to the
// same functions compiled for the host (tests/test_device_pairing.py: every value against Python integers).
// Needs pairing_math.inc (namespace pairing_dev: the tower over Fp / Fp2) in scope.
//
// Layout: ONE Miller loop per lane, the tower in plain C++ over field.hpp (pairing_body.inc's projective miller(): no
// inversion, no canon_wide; every Fp product is the out-of-line multiply-add chain fp_mul_call).  A loop is a latency
// chain of ~9 300 dependent-ish Fp products whatever the batch size, and a wave costs the same time with 1 or 64 of its
// lanes at work, so what decides the time of a batch below 64 x (SIMDs of the chip) pairs is how many SIMDs take part:
// the launch SPREADS the pairs -- `lpw` active lanes per wave, chosen by the host so that every SIMD gets a wave before
// any wave gets a second lane (spread_index below).  4 096 pairs are 1 024 waves of 4 lanes instead of 64 full waves on
// 64 of 1 024 SIMDs.  Beyond 65 536 pairs the waves are full and the kernel is throughput-bound like any other.
// MEASURED (profiles/verify_batch.txt): 64 one-lane waves take 17.6 ms and 1 024 full waves 17.5 ms,
// but 1 024 waves of one or four lanes take 40 ms -- the spreading does not pay at N = 1 024 .. 4 096, cause not found yet.
// The final exponentiation is not here: it runs once per batch, on the host (pairing_body.inc, final_exp).
#pragma once

namespace pairing_dev {

// Thread `tid` of a launch of waves of 64 with `lpw` active lanes each: its element, or false when the lane idles.
// Elements 0 .. n-1 are each taken by exactly one thread of a launch of ceil(n / lpw) waves.
PS_HD static inline bool spread_index(u32 tid, u32 lpw, u32 n, u32& idx) {
    const u32 wave = tid >> 6, lane = tid & 63u;
    if (lane >= lpw) return false;
    idx = wave * lpw + lane;
    return idx < n;
}
// Active lanes per wave for n elements on a chip of `simds` SIMDs (one wave per SIMD first)
PS_HD static inline u32 spread_lanes(u64 n, u32 simds) {
    const u64 l = (n + simds - 1) / (simds ? simds : 1);
    return l < 1 ? 1u : l > 64 ? 64u : (u32)l;
}

// a * b read coefficient by coefficient from memory, for the product tree: over the basis 1, w, .., w^5 (w^6 = xi; the
// coefficient of w^(2j+i) is c_i.c_j of the tower) coefficient d of the product is
//     sum_{d1+d2 = d} a_d1 b_d2  +  xi * sum_{d1+d2 = d+6} a_d1 b_d2,
// 36 Fp2 products where f12_mul's Karatsuba has 18 -- but only one accumulator and two operands are alive at a time, so
// the kernel needs no scratch memory, which f12_mul inlined over two 168-register operands does (841 spilled registers).
// The tree is N products against the N x ~3 100 of the Miller loops.  Lazy limbs: every partial sum is carry-save
// normalised (class <= 2); a sum of up to six Fp2 products reaches (-15 p, 7.5 p), so each of the two sums goes through
// one reducing product by R (back into (-p/8, 9p/8)) before xi and the final addition: the stored coefficients stay
// below 4 p in absolute value at limb class <= 2, whatever the depth of the tree.
PS_HD static inline const Base2& f12_coeff(const Fp12& a, int d) {
    const Fp6& h = (d & 1) ? a.c1 : a.c0;
    return (d >> 1) == 0 ? h.c0 : (d >> 1) == 1 ? h.c1 : h.c2;
}
// (f12_mul_coeff and f12_mul_mem are forced inline: left to the inliner they went out of line the day a second kernel,
// k_f12_segment_products of locate_phgr13_dev.hpp, called them, and k_f12_product went from 187 registers to 280 + 32.)
PS_HD static inline Base2 f2_reduce(const Base2& a) { return Base2{fp_mul_call(f_norm(a.c0), fp_one()), fp_mul_call(f_norm(a.c1), fp_one())}; }
PS_HD static inline __attribute__((always_inline)) Base2 f12_mul_coeff(const Fp12& a, const Fp12& b, int d) {
    Base2 lo = f_zero((const Base2*)0), hi = f_zero((const Base2*)0);
    for (int d1 = 0; d1 < 6; d1++) {
        const int d2 = d1 <= d ? d - d1 : d + 6 - d1;
        const Base2 t = f_mul(f12_coeff(a, d1), f12_coeff(b, d2));
        if (d1 <= d) lo = f_norm(f_add(lo, t)); else hi = f_norm(f_add(hi, t));
    }
    return f_norm(f_add(f2_reduce(lo), mul_xi(f2_reduce(hi))));
}
PS_HD static inline __attribute__((always_inline)) void f12_mul_mem(Fp12& out, const Fp12& a, const Fp12& b) {  // out must not alias a or b
    out.c0.c0 = f12_mul_coeff(a, b, 0); out.c1.c0 = f12_mul_coeff(a, b, 1);
    out.c0.c1 = f12_mul_coeff(a, b, 2); out.c1.c1 = f12_mul_coeff(a, b, 3);
    out.c0.c2 = f12_mul_coeff(a, b, 4); out.c1.c2 = f12_mul_coeff(a, b, 5);
}

// One node of the product tree: level k+1 has ceil(n / 2) values, value i = in[2i] * in[2i+1] (the odd one out is
// carried up).
PS_HD static inline void f12_tree_node(Fp12* out, const Fp12* in, u32 n, u32 i) {
    if (2 * i + 1 < n) f12_mul_mem(out[i], in[2 * i], in[2 * i + 1]);
    else out[i] = in[2 * i];
}

}  // namespace pairing_dev

namespace ps {
// One thread's share of t_j = sum_i w_i m_ij (mod r): rows [row0, row1) of column j.  w in Montgomery form (nullptr: all
// ones), m plain canonical 8 x 32-bit words, row-major; the result canonical plain limbs.  A product leaves (-r/8, 9r/8);
// sixteen of them summed stay far inside fr_mul's |A| |B| <= 2^22 r^2, then one product by R brings the sum back.
PS_HD static inline Fr fr_weighted_column(const Fr* w, const u32* m, u32 cols, u32 j, u32 row0, u32 row1) {
    Fr acc = fr_zero();
    const Fr one = fr_one();
    for (u32 i = row0; i < row1; i++) {
        u32 x[8];
        const u32* src = m + ((size_t)i * cols + j) * 8;
        for (int k = 0; k < 8; k++) x[k] = src[k];
        acc = fr_norm(fr_add(acc, fr_mul(w ? w[i] : one, fr_from_words8(x))));
        if (((i - row0) & 15u) == 15u) acc = fr_reduce(acc);
    }
    return fr_canon(fr_reduce(acc));
}
}  // namespace ps

#if defined(PS_HOSTFIELD)
// The value the device stored (lazy limbs, Montgomery R = 2^392) in the host field: twelve to_host conversions.  What the
// verifier does with the downloaded product; host code only.
static inline pairing::Fp12 f12_to_host(const pairing_dev::Fp12& a) {
    pairing::Fp12 r;
    r.c0 = pairing::Fp6{to_host(a.c0.c0), to_host(a.c0.c1), to_host(a.c0.c2)};
    r.c1 = pairing::Fp6{to_host(a.c1.c0), to_host(a.c1.c1), to_host(a.c1.c2)};
    return r;
}
#endif

#if defined(__HIPCC__) || defined(__HIP__)
namespace ps {

// f_i = miller(P_i, Q_i); identity in either slot gives one.  One wave per SIMD: the loop carries f (168 registers), the
// running point (84), a line (84) and the temporaries of f12_sqr.
__global__ void __launch_bounds__(64, 1) k_miller_batch(const Affine<Fp>* __restrict__ g1, const Affine<Fp2>* __restrict__ g2, u32 n,
                                                        u32 lpw, pairing_dev::Fp12* __restrict__ out) {
    u32 i;
    if (!pairing_dev::spread_index(blockIdx.x * blockDim.x + threadIdx.x, lpw, n, i)) return;
    out[i] = pairing_dev::miller(g1[i], g2[i]);
}

// One level of the product tree: out[i] = in[2i] * in[2i+1], i < ceil(n / 2)
__global__ void __launch_bounds__(64, 1) k_f12_product(const pairing_dev::Fp12* __restrict__ in, u32 n, u32 lpw,
                                                       pairing_dev::Fp12* __restrict__ out) {
    u32 i;
    if (!pairing_dev::spread_index(blockIdx.x * blockDim.x + threadIdx.x, lpw, (n + 1) / 2, i)) return;
    pairing_dev::f12_tree_node(out, in, n, i);
}

// out[chunk][j] = sum over the chunk's rows of w_i m_ij: thread j of grid row `chunk` (neighbouring lanes read neighbouring
// columns of a row).  The host applies it again to the chunks' sums (w = nullptr) until one row is left.
__global__ void __launch_bounds__(256) k_fr_weighted_columns(const Fr* __restrict__ w, const u32* __restrict__ m, u32 rows, u32 cols,
                                                            u32 rows_per_chunk, u32* __restrict__ out) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x, chunk = blockIdx.y;
    if (j >= cols) return;
    const u32 row0 = chunk * rows_per_chunk;
    if (row0 >= rows) return;
    const u32 row1 = rows - row0 < rows_per_chunk ? rows : row0 + rows_per_chunk;
    u32 x[8];
    fr_to_words8(x, fr_weighted_column(w, m, cols, j, row0, row1));
    u32* dst = out + ((size_t)chunk * cols + j) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = x[k];
}

}  // namespace ps
#endif
