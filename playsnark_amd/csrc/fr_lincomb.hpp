// Linear combinations of scalar vectors on the device: Poly.Add / Poly.Sub (algebra.go:161-196), scaling, and the rows
// f_j = sum_l c_lj p_l a KZG prover divides once per point instead of once per (polynomial, point) pair (kzg.inc).
//
//   out[j * N + i] = sum_l c_lj v_l[i],   l < m inputs, j < t rows, i < N = max_l len_l, every v_l zero behind its end
//
// One index i per thread and FR_LINCOMB_ROWS rows per workgroup row (blockIdx.y): an input word is loaded once and meets the
// R coefficients of its group.  The per-input (pointer, length) and the m x t coefficients do not fit kernel arguments: they lie
// in device memory and every lane of a wave reads the same entry, so the loads are uniform.  A zero entry (PLONK's matrices are
// mostly zero) costs a workgroup-uniform branch on its flag and no product.  No atomics, no waiting on another workgroup.
//
// Number forms, the convention of poly_scan.hpp: the inputs are the plain canonical words of a ps_scalars and are NOT
// converted; with c in Montgomery form fr_mul(plain, mont) is the plain product, so the sum is plain and is stored as canonical
// words through poly_scan_store.  Index arithmetic and table layout: fr_lincomb_plan.hpp.
#pragma once
#include "fr_lincomb_plan.hpp"
#include "poly_scan.hpp"

namespace ps {

__device__ inline Fr fr_lincomb_coef(const FrLincombCoef* __restrict__ c) {
    Fr r;
#pragma unroll
    for (int k = 0; k < FR_L; k++) r.l[k] = c->l[k];
    return r;
}

// Rows [(g0 + blockIdx.y) R, ..) of out at index i = blockIdx.x * 256 + threadIdx.x.
__global__ void __launch_bounds__(FR_LINCOMB_THREADS) k_fr_lincomb(const FrLincombInput* __restrict__ in, u32 m, const FrLincombCoef* __restrict__ coef,
                                                                   u32 t, u32 g0, u64 N, u32* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * FR_LINCOMB_THREADS + threadIdx.x;
    const u32 j0 = (g0 + blockIdx.y) * FR_LINCOMB_ROWS;
    Fr acc[FR_LINCOMB_ROWS];
#pragma unroll
    for (int r = 0; r < FR_LINCOMB_ROWS; r++) acc[r] = fr_zero();
    // Lazy ranges (field.hpp): a product of a canonical word and a canonical coefficient lies in (-r/8, 9r/8) and so does a
    // reduced accumulator.  An input adds at most one product to each accumulator and the accumulators are reduced behind
    // every 32nd input, so between two reductions a value stays in (-33r/8, 297r/8): |V| < 38 r, and fr_norm keeps the limbs
    // at class 1 after every addition.  fr_reduce's product with one then has |A| |B| < 38 r^2, far below the 2^22 r^2 of
    // fr_mul's contract, and its result is back in (-r/8, 9r/8), inside poly_scan_store's (-2r, 3r).
#pragma unroll 1
    for (u32 l = 0; l < m; l++) {
        const u64 len = in[l].n;
        if (i < len) {
            const Fr v = poly_scan_load(in[l].p, i, len);
#pragma unroll
            for (int r = 0; r < FR_LINCOMB_ROWS; r++) {
                const u32 j = j0 + r;
                if (j < t) {
                    const FrLincombCoef* c = coef + (u64)l * t + j;
                    if (c->nonzero) acc[r] = fr_norm(fr_add(acc[r], fr_mul(v, fr_lincomb_coef(c))));
                }
            }
        }
        if (fr_lincomb_reduce_after(l)) {
#pragma unroll
            for (int r = 0; r < FR_LINCOMB_ROWS; r++) acc[r] = fr_reduce(acc[r]);
        }
    }
    if (i >= N) return;
#pragma unroll
    for (int r = 0; r < FR_LINCOMB_ROWS; r++) {
        const u32 j = j0 + r;
        if (j < t) poly_scan_store(out + 8 * ((u64)j * N + i), fr_reduce(acc[r]));
    }
}

}  // namespace ps
