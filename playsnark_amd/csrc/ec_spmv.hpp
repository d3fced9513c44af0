// Column sums of an R1CS matrix over POINTS: out[i] = sum_j M[j][i] P[j] for every variable i -- the sparse matrix of the
// setups' per-variable sums (prove.inc, setup_var_evals: u_i(x) = sum_j M[j][i] l_j(x)) applied to a vector of group elements
// instead of field elements.  It is what (beta u_i(x) + alpha v_i(x) + w_i(x)) G1 (groth16.go:254-264) becomes when nobody
// knows x, alpha or beta: three such sums over the Lagrange forms of {beta x^i G1}, {alpha x^i G1}, {x^i G1}.
//
// A coefficient enters as a signed magnitude (coef_width.hpp): v itself up to (r - 1) / 2, else r - v and a sign for the point.
// A row is then Horner over the bit planes of the WHOLE row,
//     acc = 2 acc + sum_{e : bit b of |v_e| set} (+-) P[col_e],        b = the row's highest set bit .. 0,
// one doubling per plane plus one mixed addition per set bit (a +-1 row is a single plane: additions only).
// xyzz_madd's exceptional cases carry the rest: an identity input point (stored as (0, 0)) is skipped, P + P inside a plane
// takes the doubling branch, P + (-P) leaves the identity, and a zero coefficient has no set bit.
//
// Two families of kernels, chosen per matrix by ps_qap's count of wide entries:
//   * no magnitude of the matrix needs more than 64 bits -- every matrix that came through ps_qap_create (int64,
//     Value.ToFieldElement, curve.go:17-19; 2^63 included), and a ps_qap_create_fr matrix of such values: k_colsum_coef keeps
//     one 64-bit word per entry, k_colsum_rows / k_colsum_long walk at most 64 planes;
//   * at least one wide entry (a hash's round constants, 2^k weights for k >= 64): k_colsum_coef_wide keeps four 64-bit words
//     per entry, word-major (word k of entry e at mag[k * nnz + e], so the planes of one word read 8 B per entry as the
//     narrow kernels do), and the number of words the entry needs in three spare bits of its column index.  The Horner walk
//     of k_colsum_rows_wide / k_colsum_long_wide starts at the row's OWN highest set bit: a +-1 row of a wide matrix is still
//     one plane, an int64 row at most 64, and the words above a row's highest are never read.  A wide row pays at most 254
//     doublings.
//
// Rows are the rows of ps_qap::matT (variables).  Rows of more than SPMV_LONG_ROW non-zeros -- the `const` variable's
// column of any circuit of a few thousand gates -- go to the long kernel: one workgroup per row, every logical thread the
// Horner sum of its own stride of the row, then the LDS tree (block_tree_sum), as k_spmv_long_rows does for scalars.
// All row kernels leave XYZZ points; k_batch_to_affine follows.
//
// One kind of row takes neither: a long row that holds a WIDE entry (every round constant of a hash multiplies `const`:
// tens of thousands of full-width terms in one row).  One workgroup needs seconds for it; column_sums_t (srs_setup.inc)
// gathers the row's points and hands them with the coefficients to the library's multi-scalar multiplication instead.
// k_colsum_long_wide keeps the long rows of a wide matrix that hold no wide entry.
#pragma once
#include "coef_width.hpp"
#include "msm.hpp"
#include "quotient.hpp"

namespace ps {

constexpr u32 COLSUM_NEG = 1u << 31;  // flag on the column index (gates < 2^27): the point enters negated
constexpr int COLSUM_LONG_THREADS = 128;

// mag[e] = |v_e| (as the int64 it came from), cs[e] = col[e] | COLSUM_NEG if v_e < 0
__global__ void __launch_bounds__(256) k_colsum_coef(const Fr* __restrict__ val, const u32* __restrict__ col, u32 nnz, u64* __restrict__ mag,
                                                     u32* __restrict__ cs) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const Fr v = val[e];
    u32 w[8];
    fr_to_words8(w, fr_from_mont(v));
    u32 neg = 0;
    if (w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) {  // above 2^64: r - |v|
        fr_to_words8(w, fr_from_mont(fr_neg(v)));
        neg = COLSUM_NEG;
    }
    mag[e] = (u64)w[0] | ((u64)w[1] << 32);
    cs[e] = col[e] | neg;
}

// sum_{e = first, first + step, .. < end} (+-)|v_e| P[col_e]
template <class KF>
__device__ inline Xyzz<KF> colsum_horner(const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts, const u64* __restrict__ mag,
                                         const u32* __restrict__ cs, u32 first, u32 end, u32 step) {
    u64 any = 0;
    for (u32 e = first; e < end; e += step) any |= mag[e];
    Xyzz<KF> acc = xyzz_identity<KF>();
    if (!any) return acc;
#pragma unroll 1
    for (int bit = 63 - __clzll((long long)any); bit >= 0; bit--) {
        acc = xyzz_dbl_inl<KF>(acc);
#pragma unroll 1
        for (u32 e = first; e < end; e += step) {
            if (!((mag[e] >> bit) & 1ull)) continue;
            const u32 c = cs[e];
            Affine<KF> a = ld_affine<KF>(&pts[c & ~COLSUM_NEG]);
            if (affine_is_identity<KF>(a)) continue;
            if (c & COLSUM_NEG) a.y = f_neg(a.y);
            xyzz_madd_inl<KF>(acc, a.x, a.y);
        }
    }
    return acc;
}

// one logical thread per row of at most SPMV_LONG_ROW non-zeros (an empty row: the identity)
template <class KF>
__global__ void __launch_bounds__(256, 1) k_colsum_rows(const u32* __restrict__ row_ptr, const u64* __restrict__ mag, const u32* __restrict__ cs,
                                                        const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts, u32 rows,
                                                        Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out) {
    const u32 r = logical_tid<KF>();
    if (r >= rows) return;
    const u32 first = row_ptr[r], end = row_ptr[r + 1];
    if (end - first > SPMV_LONG_ROW) return;  // k_colsum_long owns it
    st_xyzz<KF>(&out[r], colsum_horner<KF>(pts, mag, cs, first, end, 1));
}

// one workgroup per long row; dynamic LDS: one XYZZ point per logical thread
template <class KF>
__global__ void __launch_bounds__(COLSUM_LONG_THREADS) k_colsum_long(const u32* __restrict__ row_ptr, const u64* __restrict__ mag,
                                                                    const u32* __restrict__ cs,
                                                                    const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts,
                                                                    const u32* __restrict__ long_rows,
                                                                    Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    typedef typename FieldTraits<KF>::Store S;
    Xyzz<S>* sm = reinterpret_cast<Xyzz<S>*>(smem_raw);
    const u32 r = long_rows[blockIdx.x];
    const u32 lt = logical_local<KF>();
    const Xyzz<KF> mine = colsum_horner<KF>(pts, mag, cs, row_ptr[r] + lt, row_ptr[r + 1], logical_block<KF>());
    block_tree_sum<KF>(sm, mine);
    if (lt == 0) st_xyzz<KF>(&out[r], ld_xyzz<KF>(&sm[0]));
}

// ---- matrices with at least one wide entry ----
constexpr u32 COLSUM_WORDS_SHIFT = 28;           // bits 28..30 of cs: the 64-bit words the magnitude needs, 0..4
constexpr u32 COLSUM_COL_MASK = (1u << 27) - 1;  // gates < 2^27

// mag[k * nnz + e] = word k of |v_e|, cs[e] = col[e] | words << 28 | COLSUM_NEG if the magnitude is r - v_e
__global__ void __launch_bounds__(256) k_colsum_coef_wide(const Fr* __restrict__ val, const u32* __restrict__ col, u32 nnz, u64* __restrict__ mag,
                                                          u32* __restrict__ cs) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    u32 v[8], w[8];
    fr_to_words8(v, fr_from_mont(val[e]));
    const bool neg = coef_signed_magnitude(w, v);
#pragma unroll
    for (int k = 0; k < 4; k++) mag[(size_t)k * nnz + e] = (u64)w[2 * k] | ((u64)w[2 * k + 1] << 32);
    cs[e] = col[e] | ((u32)coef_words64(w) << COLSUM_WORDS_SHIFT) | (neg ? COLSUM_NEG : 0u);
}

// sum_{e = first, first + step, .. < end} (+-)|v_e| P[col_e], magnitudes of up to four words
template <class KF>
__device__ inline Xyzz<KF> colsum_horner_wide(const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts, const u64* __restrict__ mag,
                                              const u32* __restrict__ cs, u32 nnz, u32 first, u32 end, u32 step) {
    u32 words = 0;
    for (u32 e = first; e < end; e += step) words = max(words, (cs[e] >> COLSUM_WORDS_SHIFT) & 7u);
    Xyzz<KF> acc = xyzz_identity<KF>();
    if (!words) return acc;
    const u64* top = mag + (size_t)(words - 1) * nnz;
    u64 any = 0;
    for (u32 e = first; e < end; e += step) any |= top[e];  // (non-zero: some entry needs this word)
#pragma unroll 1
    for (int bit = 64 * (int)(words - 1) + 63 - __clzll((long long)any); bit >= 0; bit--) {
        acc = xyzz_dbl_inl<KF>(acc);
        const u64* plane = mag + (size_t)(bit >> 6) * nnz;
        const int sh = bit & 63;
#pragma unroll 1
        for (u32 e = first; e < end; e += step) {
            if (!((plane[e] >> sh) & 1ull)) continue;
            const u32 c = cs[e];
            Affine<KF> a = ld_affine<KF>(&pts[c & COLSUM_COL_MASK]);
            if (affine_is_identity<KF>(a)) continue;
            if (c & COLSUM_NEG) a.y = f_neg(a.y);
            xyzz_madd_inl<KF>(acc, a.x, a.y);
        }
    }
    return acc;
}

template <class KF>
__global__ void __launch_bounds__(256, 1) k_colsum_rows_wide(const u32* __restrict__ row_ptr, const u64* __restrict__ mag, const u32* __restrict__ cs,
                                                             u32 nnz, const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts, u32 rows,
                                                             Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out) {
    const u32 r = logical_tid<KF>();
    if (r >= rows) return;
    const u32 first = row_ptr[r], end = row_ptr[r + 1];
    if (end - first > SPMV_LONG_ROW) return;  // k_colsum_long_wide owns it
    st_xyzz<KF>(&out[r], colsum_horner_wide<KF>(pts, mag, cs, nnz, first, end, 1));
}

template <class KF>
__global__ void __launch_bounds__(COLSUM_LONG_THREADS) k_colsum_long_wide(const u32* __restrict__ row_ptr, const u64* __restrict__ mag,
                                                                         const u32* __restrict__ cs, u32 nnz,
                                                                         const Affine<typename FieldTraits<KF>::Store>* __restrict__ pts,
                                                                         const u32* __restrict__ long_rows,
                                                                         Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    typedef typename FieldTraits<KF>::Store S;
    Xyzz<S>* sm = reinterpret_cast<Xyzz<S>*>(smem_raw);
    const u32 r = long_rows[blockIdx.x];
    const u32 lt = logical_local<KF>();
    const Xyzz<KF> mine = colsum_horner_wide<KF>(pts, mag, cs, nnz, row_ptr[r] + lt, row_ptr[r + 1], logical_block<KF>());
    block_tree_sum<KF>(sm, mine);
    if (lt == 0) st_xyzz<KF>(&out[r], ld_xyzz<KF>(&sm[0]));
}

}  // namespace ps
