// Quotient of a polynomial by the vanishing polynomial of a point set: Poly.Div (algebra.go:119-137) by Z_S = prod_j (X - z_j),
// the step between a commitment and ONE KZG proof for k points of one polynomial (kzg.inc, ps_kzg_open_set).
//
// Partial fractions: 1 / Z_S = sum_j w_j / (X - z_j) with w_j = 1 / prod_{l != j} (z_j - z_l), hence
//     q = (p - r) / Z_S = sum_j w_j q_j,   q_j = (p - p(z_j)) / (X - z_j)
// and the q_j are the rows the linear scan writes (poly_scan.hpp).  So no new scan: tile totals and the carry walk run as they
// are for the k points (k_poly_scan_tile<false>, k_poly_scan_carries; they also give the values p(z_j)), and the kernel below is
// the apply pass that FOLDS the k weighted rows into one while it scans instead of writing them.  The top k - 1 coefficients of
// the sum are zero by the identity and are not stored: q has n - k coefficients.
//
// Work split (index arithmetic: poly_scan_set_plan.hpp): a workgroup owns tile blockIdx.x and the group blockIdx.y of G
// consecutive points, runs the apply pass once per point of its group and adds w_j h_i into I accumulators per thread; behind
// the group's last point they go out to partial row blockIdx.y.  One group (k <= G): the partial row is q.  More: the
// ceil(k / G) rows are summed by k_fr_lincomb with unit weights.  Extra device memory: ceil(k / G) rows of n - k scalars where the
// composed route (ps_poly_div_linear, then a weighted sum of its rows) holds k rows of n - 1.
// No look-back, no flag another workgroup has to set, no atomics: a workgroup never waits for one that may not be scheduled.
//
// Number forms: p plain canonical words, z_j, its powers and w_j in Montgomery form, so h and w h are plain (poly_scan.hpp).
#pragma once
#include "poly_scan.hpp"
#include "poly_scan_set_plan.hpp"

namespace ps {

static_assert(POLY_SCAN_ITEMS == 8, "the accumulators below are named item by item");

// Tile b = blockIdx.x, points [g G, min(k, (g + 1) G)) for g = blockIdx.y.  out: partial rows of nq = n - k scalars (plain
// canonical words); row g gets sum_j w_j h_i at i - 1 for the tile's i with 1 <= i <= nq.  carries[j * tiles + b] = h of point j
// at the tile's end (k_poly_scan_carries), weights[j] = w_j.
__global__ void __launch_bounds__(POLY_SCAN_THREADS) k_poly_scan_set_apply(const u32* __restrict__ p, u64 n, u32 tiles, u32 k, u64 nq,
                                                                           const FrPow2Table* __restrict__ tabs, const Fr* __restrict__ weights,
                                                                           const Fr* __restrict__ carries, u32* __restrict__ out) {
    __shared__ Fr sm[2][POLY_SCAN_THREADS];
    const u32 b = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    if (!poly_scan_set_tile_stores(b, nq)) return;  // the whole tile lies in the zero top (uniform: before any barrier)
    const u32 j0 = g * POLY_SCAN_SET_GROUP;
    const u32 len = k - j0 < (u32)POLY_SCAN_SET_GROUP ? k - j0 : (u32)POLY_SCAN_SET_GROUP;
    const u64 base = (u64)b * POLY_SCAN_TILE + (u64)t * POLY_SCAN_ITEMS;
    // Eight accumulators, never indexed by a run-time value: the item loops over them are fully unrolled, so they stay in
    // registers (a dynamic index would send them to scratch).
    Fr acc[POLY_SCAN_ITEMS];
#pragma unroll
    for (int m = 0; m < POLY_SCAN_ITEMS; m++) acc[m] = fr_zero();
    // Lazy ranges (field.hpp).  A Horner value h = p_i + z h' is a canonical word plus a product: value in (-r/8, 17r/8), limbs
    // in (-2^28, 2^28), class 1 -- exactly what the next Horner step hands to fr_mul, so it meets w (canonical Montgomery limbs,
    // class 1, below r) WITHOUT an fr_reduce or fr_norm: |h| |w| < 17/8 r^2 against the 2^22 r^2 of fr_mul's contract.  The
    // product w h lies in (-r/8, 9r/8).  A point adds one product to each accumulator and fr_norm keeps the limbs at class 1
    // after every addition; the accumulators are reduced behind every 32nd point of a group (never, while G <= 32), so between
    // two reductions a value stays in (-33r/8, 297r/8): |V| < 38 r.  fr_reduce's product with one then has |A| |B| < 38 r^2, far
    // below 2^22 r^2, and its result is back in (-r/8, 9r/8), inside poly_scan_store's (-2r, 3r).  With G = 8 the value before
    // the store is in (-r, 9r).
#pragma unroll 1
    for (u32 l = 0; l < len; l++) {
        const u32 j = j0 + l;
        const FrPow2Table* tab = tabs + j;
        const Fr z = tab->p[0];
        const Fr carry = carries[(u64)j * tiles + b];
        Fr h = fr_zero();
        if (t == POLY_SCAN_THREADS - 1) h = carry;  // the value behind the tile's last item
#pragma unroll 1
        for (int m = POLY_SCAN_ITEMS - 1; m >= 0; m--) h = fr_add(poly_scan_load(p, base + m, n), fr_mul(h, z));
        (void)poly_scan_suffix256(h, sm, tab, POLY_SCAN_LOG_ITEMS);
        // h behind this thread's items: the next thread's inclusive suffix (the carry is inside it), or the carry itself
        h = t + 1 < (u32)POLY_SCAN_THREADS ? sm[0][t + 1] : carry;
        __syncthreads();  // sm[0] is the next point's
        const Fr w = weights[j];
#pragma unroll
        for (int m = POLY_SCAN_ITEMS - 1; m >= 0; m--) {
            h = fr_add(poly_scan_load(p, base + m, n), fr_mul(h, z));
            acc[m] = fr_norm(fr_add(acc[m], fr_mul(h, w)));
        }
        if (POLY_SCAN_SET_GROUP > POLY_SCAN_SET_REDUCE_EVERY && poly_scan_set_reduce_after(l)) {
#pragma unroll
            for (int m = 0; m < POLY_SCAN_ITEMS; m++) acc[m] = fr_reduce(acc[m]);
        }
    }
    u32* row = out + 8 * (u64)g * nq;
#pragma unroll
    for (int m = 0; m < POLY_SCAN_ITEMS; m++) {
        const u64 i = base + m;
        if (poly_scan_set_stored(i, nq)) poly_scan_store(row + 8 * (i - 1), fr_reduce(acc[m]));
    }
}

}  // namespace ps
