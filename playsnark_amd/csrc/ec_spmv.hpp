// Column sums of an R1CS matrix over POINTS: out[i] = sum_j M[j][i] P[j] for every variable i -- the sparse matrix of the
// setups' per-variable sums (prove.inc, setup_var_evals: u_i(x) = sum_j M[j][i] l_j(x)) applied to a vector of group elements
// instead of field elements.  It is what (beta u_i(x) + alpha v_i(x) + w_i(x)) G1 (groth16.go:254-264) becomes when nobody
// knows x, alpha or beta: three such sums over the Lagrange forms of {beta x^i G1}, {alpha x^i G1}, {x^i G1}.
//
// The coefficients came from int64 (Value.ToFieldElement, curve.go:17-19), so a row is NOT a sum of 255-bit multiplications:
// k_colsum_coef brings each value out of Montgomery form once and, when it is above r / 2, stores r - v and a sign for the
// point; the magnitude fits 64 bits (2^63 included).  A row is then Horner over the bit planes of the WHOLE row,
//     acc = 2 acc + sum_{e : bit b of |v_e| set} (+-) P[col_e],        b = the row's highest set bit .. 0,
// at most 64 doublings plus one mixed addition per set bit (a +-1 row is a single plane: additions only).
// xyzz_madd's exceptional cases carry the rest: an identity input point (stored as (0, 0)) is skipped, P + P inside a plane
// takes the doubling branch, P + (-P) leaves the identity, and a zero coefficient has no set bit.
//
// Rows are the rows of ps_qap::matT (variables).  Rows of more than SPMV_LONG_ROW non-zeros -- the `const` variable's
// column of any circuit of a few thousand gates -- go to k_colsum_long: one workgroup per row, every logical thread the
// Horner sum of its own stride of the row, then the LDS tree (block_tree_sum), as k_spmv_long_rows does for scalars.
// Both kernels leave XYZZ points; k_batch_to_affine follows.
#pragma once
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

}  // namespace ps
