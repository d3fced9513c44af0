// Value and linear quotient of a polynomial at several points: Poly.Eval (algebra.go:107-115) and Poly.Div by (X - z)
// (algebra.go:119-137), the step between a commitment and its KZG opening proofs (kzg.inc).
//
// With h_n = 0 and h_i = p_i + z h_{i+1}:  h_0 = p(z), and q_{i-1} = h_i, 1 <= i < n, is (p(X) - p(z)) / (X - z), lowest
// degree first.  One linear recurrence, so a scan; and every multiplier a carry meets is a power of z, so the scan needs
// no composition of operators: a suffix sum S_t = v_t + m S_{t+1} over values spaced by a fixed distance doubles with the
// multipliers m, m^2, m^4, .. -- entries of the table {z^(2^k)} the host squares once per point (FrPow2Table, as for
// k_fr_powers; here one table per point in device memory, read through uniform loads, because blockIdx.y picks the point).
//
// Reduce-then-scan in three launches (index arithmetic: poly_scan_plan.hpp):
//   k_poly_scan_tile<false>   tile totals H_b: a thread's Horner over its I items, then eight doubling steps in LDS
//   k_poly_scan_carries       one workgroup per point walks the totals from the top in chunks of 256 tiles:
//                             carry_b = H_{b+1} + z^T carry_{b+1}; its last value is p(z)
//   k_poly_scan_tile<true>    the same tile scan with carry_b entering as the value behind thread 255's items, then a second
//                             Horner pass from each thread's exclusive suffix that writes q_{i-1} = h_i
// No look-back and no flag another workgroup has to set: a workgroup never waits for one that may not be scheduled.
//
// Number forms: the coefficients are the plain canonical 8 x 32-bit words of a ps_scalars and are NOT converted: with z and
// its powers in Montgomery form, fr_mul(plain, mont) is the plain product, so h stays plain throughout -- one product per
// item in the totals, two in the apply pass, none for conversions.  Values are lazy (field.hpp): a Horner step p + z h
// lies in (-r/8, 17r/8), inside fr_canon's range; a scan adds at most eight products to that (|V| < 12 r, limbs brought
// back by fr_norm), a carry at most nine more: far inside fr_mul's contract.  Exact in Fr, so every order gives the
// oracle's bytes.
#pragma once
#include "poly_scan_plan.hpp"
#include "quotient.hpp"

namespace ps {

__device__ inline Fr poly_scan_load(const u32* __restrict__ p, u64 i, u64 n) {  // coefficient i, zero behind the end
    if (i >= n) return fr_zero();
    const uint4* p4 = reinterpret_cast<const uint4*>(p + 8 * i);
    const uint4 lo = p4[0], hi = p4[1];
    const u32 w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return fr_from_words8(w);
}
__device__ inline void poly_scan_store(u32* __restrict__ dst, const Fr& v) {  // v in (-2r, 3r), plain -> canonical words
    u32 w[8];
    fr_to_words8(w, fr_canon(v));
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// S_t = v_t + m S_{t+1} over the 256 threads of a workgroup, m = z^(2^log_m): eight doubling steps, sm ping-pongs.
// Returns S_t; the final values are also in sm[0][.] (eight flips), behind a barrier.
__device__ inline Fr poly_scan_suffix256(Fr v, Fr (*sm)[POLY_SCAN_THREADS], const FrPow2Table* __restrict__ tab, int log_m) {
    const u32 t = threadIdx.x;
    int cur = 0;
    sm[0][t] = v;
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 8; s++) {
        const u32 d = 1u << s;
        if (t + d < (u32)POLY_SCAN_THREADS) v = fr_norm(fr_add(v, fr_mul(sm[cur][t + d], tab->p[log_m + s])));
        cur ^= 1;
        sm[cur][t] = v;
        __syncthreads();
    }
    return v;
}

// Tile b = blockIdx.x of point j = blockIdx.y.  APPLY = false: totals[j * tiles + b] = H_b.  APPLY = true: row j of q
// (n - 1 scalars, plain words) gets q_{i-1} = h_i for the tile's i >= 1, with carries[j * tiles + b] = h at the tile's end.
template <bool APPLY>
__global__ void __launch_bounds__(POLY_SCAN_THREADS) k_poly_scan_tile(const u32* __restrict__ p, u64 n, u32 tiles,
                                                                      const FrPow2Table* __restrict__ tabs, Fr* __restrict__ totals,
                                                                      const Fr* __restrict__ carries, u32* __restrict__ q) {
    __shared__ Fr sm[2][POLY_SCAN_THREADS];
    const u32 b = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    const FrPow2Table* tab = tabs + j;
    const Fr z = tab->p[0];
    const u64 base = (u64)b * POLY_SCAN_TILE + (u64)t * POLY_SCAN_ITEMS;
    Fr h = fr_zero();
    if (APPLY && t == POLY_SCAN_THREADS - 1) h = carries[(u64)j * tiles + b];  // the value behind the tile's last item
#pragma unroll 1
    for (int m = POLY_SCAN_ITEMS - 1; m >= 0; m--) h = fr_add(poly_scan_load(p, base + m, n), fr_mul(h, z));
    const Fr S = poly_scan_suffix256(h, sm, tab, POLY_SCAN_LOG_ITEMS);
    if (!APPLY) {
        if (t == 0) totals[(u64)j * tiles + b] = S;
        return;
    }
    // h behind this thread's items: the next thread's inclusive suffix (the carry is inside it), or the carry itself
    h = t + 1 < (u32)POLY_SCAN_THREADS ? sm[0][t + 1] : carries[(u64)j * tiles + b];
    u32* row = q + 8 * (u64)j * (n - 1);
#pragma unroll 1
    for (int m = POLY_SCAN_ITEMS - 1; m >= 0; m--) {
        const u64 i = base + m;
        h = fr_add(poly_scan_load(p, i, n), fr_mul(h, z));
        if (i >= 1 && i < n) poly_scan_store(row + 8 * (i - 1), h);
    }
}

// Point j = blockIdx.x: G_b = H_b + z^T G_{b+1} from the last tile down, 256 tiles at a time; carries[b] = G_{b+1}
// (zero behind the last tile), y[j] = G_0 = p(z_j) as canonical plain words.
__global__ void __launch_bounds__(POLY_SCAN_THREADS) k_poly_scan_carries(const Fr* __restrict__ totals, Fr* __restrict__ carries, u32 tiles,
                                                                         const FrPow2Table* __restrict__ tabs, u32* __restrict__ y) {
    __shared__ Fr sm[2][POLY_SCAN_THREADS];
    const u32 j = blockIdx.x, t = threadIdx.x;
    const FrPow2Table* tab = tabs + j;
    const Fr* H = totals + (u64)j * tiles;
    Fr* out = carries + (u64)j * tiles;
    if (t == 0) out[tiles - 1] = fr_zero();
    Fr above = fr_zero();  // G at the first tile of the chunk above
    for (u32 c = (tiles + POLY_SCAN_CHUNK - 1) / POLY_SCAN_CHUNK; c-- > 0;) {
        const u32 b = c * POLY_SCAN_CHUNK + t;
        Fr v = b < tiles ? H[b] : fr_zero();
        if (t == POLY_SCAN_CHUNK - 1) v = fr_norm(fr_add(v, fr_mul(above, tab->p[POLY_SCAN_LOG_TILE])));
        const Fr G = poly_scan_suffix256(v, sm, tab, POLY_SCAN_LOG_TILE);
        if (b >= 1 && b < tiles) out[b - 1] = G;
        above = sm[0][0];
        __syncthreads();  // sm[0] is the next chunk's
    }
    if (t == 0) poly_scan_store(y + 8 * (u64)j, fr_reduce(above));
}

}  // namespace ps
