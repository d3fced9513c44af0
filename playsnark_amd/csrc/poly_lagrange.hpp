// Value and linear quotient of a polynomial GIVEN BY ITS VALUES v_1 .. v_n on the nodes 1 .. n, at several points: what
// ps_poly_eval and ps_poly_div_linear do for coefficients, with no interpolation.  The quotient comes out as its values on the
// same nodes, so its commitment is a sum over the Lagrange-form string (kzg.inc).
//
// With the barycentric weights w_i = (-1)^(n-i) / ((i-1)! (n-i)!) and e_i = 1 / (z - i):
//   z off the domain      A = sum_i w_i v_i e_i, P = prod_i (z - i):  p(z) = P A   (and B = sum_i w_i e_i has B P = 1)
//   quotient values       q_i = (y - v_i) e_i at every node i != z, the values of (p - y) / (X - z), of degree <= n - 2
//   z = m on the domain   y = v_m, and deg q <= n - 2 means sum_i w_i q_i = 0:  q_m = (A - v_m B) / w_m with A and B summed
//                         over i != m, and 1 / w_m = (-1)^(n-m) (m-1)! (n-m)!
// The n inversions are one fr_inv per WORKGROUP (Montgomery's trick over a tile), a few products per node besides.
//
// Three launches (index arithmetic: poly_lagrange_plan.hpp); blockIdx.y -- blockIdx.x for the walk -- picks the point:
//   k_lagr_tile<STORE>   tile b: d_i = z - i computed, not loaded (the on-domain hit and the nodes behind n take d = 1); a
//                        thread's running products over its I nodes; exclusive prefix and suffix products of the 256 thread
//                        products by eight doubling steps in LDS; ONE fr_inv of the tile's product, on thread 0 while the
//                        other three waves sleep at the barrier; every thread unwinds its e_i, forms w_i from 1/j! at one
//                        product and a sign, adds w_i e_i and w_i e_i v_i (not for the hit); the workgroup's sums and its
//                        product go to parts as A_b, B_b, P_b.  STORE: e_i goes to row j as canonical words (Montgomery
//                        form), the row being its own scratch.
//   k_lagr_walk          one workgroup per point folds the partials 256 tiles at a time: y = (prod P_b)(sum A_b) off the domain;
//                        y = v_m and q_m = (A - v_m B)(+/-)(m-1)!(n-m)! on it.  y as canonical words, and y, q_m as Fr for ...
//   k_lagr_apply         ... row[i] <- (y - v_i) e_i in place, q_m at the hit.
// No look-back, no flag another workgroup sets, no atomics: a workgroup waits at its own barriers only.
//
// Number forms: the values are the plain canonical 8 x 32-bit words of a ps_scalars and are NOT converted; z, d_i, e_i, w_i, the
// factorials and P are in Montgomery form.  fr_mul(plain, mont) is the plain product, so A, y and q are plain, B is Montgomery.
// Lazy ranges (field.hpp):
//   d_i      z - mont(first) is a difference of two products' values, |V| < 10r/8, limbs below 2^29; every further node
//            subtracts R mod r (< r) and is fr_norm'ed: |V| < 10r/8 + (I - 1) r <= 17r, class ~1 -- an operand of fr_mul
//   products running products, prefixes, suffixes, e_i, w_i: fr_mul results, in (-r/8, 9r/8)
//   fr_inv   its input is the tile's product, an fr_mul result (fr_inv reduces it once more); never zero, since d_i = 0 only for
//            the hit, which takes 1
//   sums     a thread adds I <= 16 products and fr_norms behind each: |V| < 16 * 9r/8 = 18r.  The workgroup's tree adds 256 of
//            those, fr_norm'ed at every level: |V| < 256 * 18r = 4608r, class ~1, inside fr_mul's |A||B| <= 2^22 r^2 with the
//            one it is reduced by (ONE fr_reduce per sum and workgroup): A_b, B_b in (-r/8, 9r/8)
//   walk     a thread adds one partial per chunk, fr_norm'ed, and reduces behind every 32nd chunk: |V| < 33 * 9r/8 < 38r, for
//            any number of chunks (2^21 tiles and more are 2^13 chunks); fr_reduce before the tree: its 256 values add up to
//            |V| < 288r, reduced once more
//   canon    y = P A, q_m and (y - v_i) e_i are fr_mul results: fr_canon's range (-2r, 3r) holds; y - v_i with both canonical
//            is in (-r, r), limbs below 2^28 in magnitude
// Exact in Fr, so every order of the sums gives the oracle's bytes.
#pragma once
#include "poly_lagrange_plan.hpp"
#include "poly_scan.hpp"

namespace ps {

struct LagrPoint {
    Fr z;      // the point, Montgomery form
    u32 hit;   // the node z is (1 .. n), or 0 off the domain (poly_lagr_hit)
    u32 pad;
};

// The sum of the 256 values v over the workgroup, fr_norm'ed at every level, in sm[0] behind a barrier (and returned).
__device__ inline Fr lagr_sum256(Fr v, Fr* sm) {
    const u32 t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
#pragma unroll 1
    for (u32 stride = POLY_LAGR_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) sm[t] = fr_norm(fr_add(sm[t], sm[t + stride]));
        __syncthreads();
    }
    return sm[0];
}

// Tile b = blockIdx.x of point j = blockIdx.y: parts[plane][j * tiles + b] = A_b, B_b, P_b (planes `plane` elements apart).
// STORE: row j of rows (n scalars) gets e_i = 1 / (z_j - i) for the tile's nodes, Montgomery form as canonical words; 1 at the hit.
template <bool STORE>
__global__ void __launch_bounds__(POLY_LAGR_THREADS) k_lagr_tile(const u32* __restrict__ v, u64 n, u32 tiles, const LagrPoint* __restrict__ pts,
                                                                 const Fr* __restrict__ invfact, Fr* __restrict__ parts, u64 plane,
                                                                 u32* __restrict__ rows) {
    constexpr int I = POLY_LAGR_ITEMS;
    __shared__ Fr sm[2][2][POLY_LAGR_THREADS];  // [ping-pong][prefix, suffix][thread]
    __shared__ Fr sm_inv;
    const u32 b = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    const u64 hit = pts[j].hit;
    const u64 first = poly_lagr_node(b, t, 0);
    const Fr one = fr_one();
    // 1. d_i and the thread's prefix products: pre = P_0 .. P_{I-2} (pushed in from the right), run = P_{I-1}
    Fr d = fr_norm(fr_sub(pts[j].z, fr_from_u64(first)));
    Fr run = (first == hit || first > n) ? one : d;
    Fr pre[I - 1];
#pragma unroll
    for (int s = 0; s < I - 1; s++) pre[s] = one;
#pragma unroll 1
    for (int m = 1; m < I; m++) {
#pragma unroll
        for (int s = 0; s + 1 < I - 1; s++) pre[s] = pre[s + 1];
        pre[I - 2] = run;
        const u64 node = first + m;
        d = fr_norm(fr_sub(d, one));
        run = fr_mul(run, (node == hit || node > n) ? one : d);
    }
    // 2. inclusive prefix and suffix products of the 256 thread products: eight doubling steps, sm ping-pongs (ends in sm[0])
    Fr pf = run, sf = run;
    int cur = 0;
    sm[0][0][t] = pf;
    sm[0][1][t] = sf;
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 8; s++) {
        const u32 dist = 1u << s;
        if (t >= dist) pf = fr_mul(pf, sm[cur][0][t - dist]);
        if (t + dist < (u32)POLY_LAGR_THREADS) sf = fr_mul(sf, sm[cur][1][t + dist]);
        cur ^= 1;
        sm[cur][0][t] = pf;
        sm[cur][1][t] = sf;
        __syncthreads();
    }
    // 3. the one inversion: thread 0 alone, its wave pays what a lane pays, the other waves wait at the barrier
    if (t == 0) sm_inv = fr_inv(sf);  // sf of thread 0 is the tile's product
    __syncthreads();
    // 1 / (this thread's product) = (1 / total) x (the product before it) x (the product behind it)
    Fr inv = sm_inv;
    if (t > 0) inv = fr_mul(inv, sm[0][0][t - 1]);
    if (t + 1 < (u32)POLY_LAGR_THREADS) inv = fr_mul(inv, sm[0][1][t + 1]);
    // 4. unwind from the last node down: e = inv P_{m-1}, inv <- inv d_m; the prefixes leave pre to the right
    Fr A = fr_zero(), B = fr_zero();
    u32* row = STORE ? rows + 8 * (u64)j * n : nullptr;
#pragma unroll 1
    for (int m = I - 1; m >= 0; m--) {
        const u64 node = first + m;
        const bool skip = node == hit || node > n;
        Fr e = inv;
        if (m) {
            e = fr_mul(inv, pre[I - 2]);
            inv = fr_mul(inv, skip ? one : d);
#pragma unroll
            for (int s = I - 2; s > 0; s--) pre[s] = pre[s - 1];
            d = fr_norm(fr_add(d, one));
        }
        if (node <= n) {
            if (STORE) poly_scan_store(row + 8 * (node - 1), e);
            if (!skip) {
                Fr w = fr_mul(invfact[node - 1], invfact[n - node]);
                if ((n - node) & 1) w = fr_neg(w);
                const Fr we = fr_mul(w, e);
                B = fr_norm(fr_add(B, we));
                A = fr_norm(fr_add(A, fr_mul(poly_scan_load(v, node - 1, n), we)));
            }
        }
    }
    // 5. the workgroup's sums (sm[1] is free: the last doubling step wrote sm[0]) and its product
    A = lagr_sum256(A, sm[1][0]);
    B = lagr_sum256(B, sm[1][1]);
    if (t == 0) {
        const u64 at = (u64)j * tiles + b;
        parts[at] = fr_reduce(A);
        parts[plane + at] = fr_reduce(B);
        parts[2 * plane + at] = sm[0][1][0];
    }
}

// Point j = blockIdx.x: the partials of its tiles folded 256 at a time.  y[j] = p(z_j) as canonical plain words;
// yq[2 j] = the same as Fr, yq[2 j + 1] = q_m for a point on the domain (zero off it).
__global__ void __launch_bounds__(POLY_LAGR_THREADS) k_lagr_walk(const Fr* __restrict__ parts, u64 plane, u32 tiles, const LagrPoint* __restrict__ pts,
                                                                 const u32* __restrict__ v, u64 n, const Fr* __restrict__ fact, u32* __restrict__ y,
                                                                 Fr* __restrict__ yq) {
    __shared__ Fr sm[2][POLY_LAGR_THREADS];
    const u32 j = blockIdx.x, t = threadIdx.x;
    const Fr* pa = parts + (u64)j * tiles;
    Fr A = fr_zero(), B = fr_zero(), P = fr_one();
#pragma unroll 1
    for (u32 c = 0; c < (u32)poly_lagr_chunks(tiles); c++) {
        const u32 b = c * POLY_LAGR_CHUNK + t;
        if (b < tiles) {
            A = fr_norm(fr_add(A, pa[b]));
            B = fr_norm(fr_add(B, pa[plane + b]));
            P = fr_mul(P, pa[2 * plane + b]);
        }
        if (poly_lagr_reduce_after(c)) {
            A = fr_reduce(A);
            B = fr_reduce(B);
        }
    }
    A = lagr_sum256(fr_reduce(A), sm[0]);
    B = lagr_sum256(fr_reduce(B), sm[1]);
    __syncthreads();  // every thread holds both sums: sm is the product's now
    sm[0][t] = P;
    __syncthreads();
#pragma unroll 1
    for (u32 stride = POLY_LAGR_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) sm[0][t] = fr_mul(sm[0][t], sm[0][t + stride]);
        __syncthreads();
    }
    if (t != 0) return;
    A = fr_reduce(A);
    B = fr_reduce(B);
    const u64 m = pts[j].hit;
    Fr val, qm = fr_zero();
    if (m == 0) {
        val = fr_canon(fr_mul(sm[0][0], A));
    } else {
        val = poly_scan_load(v, m - 1, n);  // canonical as stored
        Fr iw = fr_mul(fact[m - 1], fact[n - m]);
        if ((n - m) & 1) iw = fr_neg(iw);
        qm = fr_canon(fr_mul(fr_sub(A, fr_mul(val, B)), iw));
    }
    poly_scan_store(y + 8 * (u64)j, val);
    yq[2 * (u64)j] = val;
    yq[2 * (u64)j + 1] = qm;
}

// Row j = blockIdx.y, one node per thread, in place: rows[j][i] = (y_j - v_i) e_i with e_i as k_lagr_tile<true> left it, and
// q_m at the hit.
__global__ void __launch_bounds__(POLY_LAGR_THREADS) k_lagr_apply(const u32* __restrict__ v, u64 n, const LagrPoint* __restrict__ pts,
                                                                  const Fr* __restrict__ yq, u32* __restrict__ rows) {
    const u32 j = blockIdx.y;
    const u64 i = (u64)blockIdx.x * POLY_LAGR_THREADS + threadIdx.x;  // node i + 1
    if (i >= n) return;
    u32* at = rows + 8 * ((u64)j * n + i);
    Fr q;
    if (i + 1 == pts[j].hit) q = yq[2 * (u64)j + 1];
    else q = fr_mul(fr_sub(yq[2 * (u64)j], poly_scan_load(v, i, n)), poly_scan_load(at, 0, 1));
    poly_scan_store(at, q);
}

}  // namespace ps
