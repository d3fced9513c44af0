// Quotient of a polynomial GIVEN BY ITS VALUES v_1 .. v_n on the nodes 1 .. n by the vanishing polynomial of a point set, as its
// values on the same nodes: what ps_poly_div_roots does for coefficients, with no interpolation -- the step between the values
// and ONE KZG proof for k points (kzg.inc, ps_kzg_open_set_lagrange).
//
// Partial fractions (poly_scan_set.hpp), read value by value on the nodes: with c_j = 1 / prod_{l != j} (z_j - z_l), y_j = p(z_j)
// and e_{j,i} = 1 / (z_j - i),
//     q(i) = sum_j c_j (y_j - v_i) e_{j,i}                              at a node i that no z_j equals
//     q(m) = c_j* q_m^(j*) + sum_{j != j*} c_j (y_j - v_m) e_{j,m}     at a node m = z_j*, q_m^(j*) = (A - v_m B) / w_m of the walk
// a polynomial identity, so on-domain points need nothing else; deg q <= n - 1 - k, so sum_i q(i) lag_g1[i] = [q(tau)] G1.
//
// Phase 1 is poly_lagrange.hpp as it stands: k_lagr_tile<false> and k_lagr_walk give y_j and q_m^(j).  Phase 2 is the kernel below
// (index arithmetic: poly_lagrange_set_plan.hpp): a workgroup owns tile blockIdx.x and the group blockIdx.y of G consecutive points
// and FOLDS their weighted linear quotients into one row while it computes them; nothing of k n elements is ever written.
//   forward   per point of the group: d_i = z_j - i as in k_lagr_tile (1 at the hit and behind n) and the thread's product over
//             its I nodes; the product of those over the points BEFORE this one goes to the thread's own LDS slot
//   scan      inclusive prefix and suffix products of the 256 thread products (each of G I differences) by eight doubling steps
//   invert    ONE fr_inv per workgroup -- for 256 I G differences where k_lagr_tile pays one per 256 I -- on thread 0
//   unwind    from the group's last point down: c_j / (the point's thread product) = c_j x (running inverse) x (its slot), and
//             the running inverse takes the point's product in and waits in the slot just read.  The thread's I nodes are two
//             halves: 1 / (upper half's product) = (that) x (lower half's product) and the other way round.  The upper half is
//             unwound from its last node down over its prefix products, the lower half from its first node up over its suffix
//             products -- I / 2 - 1 of either, in the thread's own LDS elements (the scan's, free by then), so that the I
//             accumulators are the only array a thread keeps in registers:  acc_i += (y_j - v_i) (c_j e_i), c_j q_m at the hit
//   store     the I sums, reduced, as canonical plain words into partial row g (the result itself when k <= G)
// For k > G the rows are summed by k_fr_lincomb with unit weights (fr_lincomb.hpp), as the coefficient route sums its own.
// No look-back, no flag another workgroup sets, no atomics: a workgroup waits at its own barriers only.
//
// Number forms: v, y_j and q_m are plain canonical; z_j, d, every product of them, the inverse and c_j are in Montgomery form, so
// the terms and the sums are plain (fr_mul(plain, mont) is the plain product).  Lazy ranges (field.hpp):
//   d_i       as in poly_lagrange.hpp: z - mont(first) has |V| < 10r/8; a step to the next node adds or subtracts R mod r and is
//             fr_norm'ed.  The walk goes up and down the thread's I nodes and never leaves them: |V| < 10r/8 + (I - 1) r
//   products  thread and half products, slots, prefixes, suffixes, inverses, c_j e_i: fr_mul results, in (-r/8, 9r/8); the operand
//             of fr_inv is one (reduced once more inside) and never zero, since d = 0 only at a hit, which takes 1
//   terms     y_j - v_i with both canonical lies in (-r, r), limbs below 2^28 in magnitude; q_m and c_j are canonical; so a term is
//             an fr_mul result in (-r/8, 9r/8)
//   sums      THE NEW POINT: a node's accumulator adds up to G such terms with an fr_norm behind each: |V| < G 9r/8 <= 36r at the
//             largest G the plan admits (32), limbs at class 1.  That leaves fr_canon's (-2r, 3r) from G = 3 on, so ONE fr_reduce
//             per node and group brings it back to (-r/8, 9r/8) before the store (|A||B| < 36 r^2 against fr_mul's 2^22 r^2)
// Exact in Fr, so every grouping of the sum gives the oracle's bytes.
#pragma once
#include "poly_lagrange.hpp"
#include "poly_lagrange_set_plan.hpp"

namespace ps {

// Tile b = blockIdx.x, points [g G, min(k, (g + 1) G)) for g = blockIdx.y.  rows: partial rows of n scalars (plain canonical
// words); row g gets sum_j c_j q_j(i) over the group's points at element i - 1 for the tile's nodes i <= n.  cw[j] = c_j;
// yq[2 j] = y_j and yq[2 j + 1] = q_m of point j, as k_lagr_walk left them.
__global__ void __launch_bounds__(POLY_LAGR_THREADS) k_lagr_fold(const u32* __restrict__ v, u64 n, u32 k, const LagrPoint* __restrict__ pts,
                                                                 const Fr* __restrict__ cw, const Fr* __restrict__ yq, u32* __restrict__ rows) {
    constexpr int I = POLY_LAGR_ITEMS, H = POLY_LAGR_SET_HALF, G = POLY_LAGR_SET_GROUP;
    __shared__ Fr sm[POLY_LAGR_SET_SCRATCH_ARRAYS][POLY_LAGR_THREADS];  // [0], [1]: the scan; then element t is thread t's own
    __shared__ Fr slot[POLY_LAGR_SET_SLOT_ARRAYS * POLY_LAGR_THREADS];  // poly_lagr_set_slot_elem: thread t's own
    __shared__ Fr sm_inv;
    const u32 b = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const u32 j0 = (u32)poly_lagr_set_point(g, 0);
    const u32 len = k - j0 < (u32)G ? k - j0 : (u32)G;
    const u64 first = poly_lagr_set_node(b, t, 0);
    const Fr one = fr_one();
    // forward: the thread's product over its nodes and the points so far
    Fr tp = one;
#pragma unroll 1
    for (u32 l = 0; l < len; l++) {
        const u64 hit = pts[j0 + l].hit;
        Fr d = fr_norm(fr_sub(pts[j0 + l].z, fr_from_u64(first)));
        Fr run = (first == hit || first > n) ? one : d;
#pragma unroll 1
        for (int m = 1; m < I; m++) {
            const u64 node = first + m;
            d = fr_norm(fr_sub(d, one));
            run = fr_mul(run, (node == hit || node > n) ? one : d);
        }
        if (l == 0) {
            tp = run;
        } else {
            slot[poly_lagr_set_slot_elem(l, t)] = tp;
            tp = fr_mul(tp, run);
        }
    }
    // scan: a step reads its two neighbours, waits, writes, waits
    {
        Fr pf = tp, sf = tp;
        sm[0][t] = pf;
        sm[1][t] = sf;
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < 8; s++) {
            const u32 dist = 1u << s;
            if (t >= dist) pf = fr_mul(pf, sm[0][t - dist]);
            if (t + dist < (u32)POLY_LAGR_THREADS) sf = fr_mul(sf, sm[1][t + dist]);
            __syncthreads();
            sm[0][t] = pf;
            sm[1][t] = sf;
            __syncthreads();
        }
        // invert: thread 0 alone, its wave pays what a lane pays, the other waves wait at the barrier
        if (t == 0) sm_inv = fr_inv(sf);  // sf of thread 0 is the product of every difference of the tile and the group
        __syncthreads();
        Fr inv_tp = sm_inv;
        if (t > 0) inv_tp = fr_mul(inv_tp, sm[0][t - 1]);
        if (t + 1 < (u32)POLY_LAGR_THREADS) inv_tp = fr_mul(inv_tp, sm[1][t + 1]);
        __syncthreads();  // the neighbours have read: sm[.][t] is this thread's own from here on
        sm[0][t] = inv_tp;
    }
    // unwind.  The accumulators are never indexed by a run-time value: the item loops are rolled and the array is TURNED by a
    // fully unrolled move, so it stays in registers (a dynamic index would send it to scratch).
    Fr acc[I];
#pragma unroll
    for (int m = 0; m < I; m++) acc[m] = fr_zero();
#pragma unroll 1
    for (u32 l = len; l-- > 0;) {
        const u32 j = j0 + l;
        const u64 hit = pts[j].hit;
        // 1 / (the thread's product over the points up to this one): the inversion's for the last point, then the slot above
        const Fr inv_tp = l + 1 == len ? sm[0][t] : slot[poly_lagr_set_slot_elem(l + 1, t)];
        // up: the lower half's product, then the upper half's with its prefixes d_H .. d_{m-1} at sm[m - H - 1]
        Fr d = fr_norm(fr_sub(pts[j].z, fr_from_u64(first)));
        Fr run_lo = (first == hit || first > n) ? one : d;
#pragma unroll 1
        for (int m = 1; m < H; m++) {
            const u64 node = first + m;
            d = fr_norm(fr_sub(d, one));
            run_lo = fr_mul(run_lo, (node == hit || node > n) ? one : d);
        }
        d = fr_norm(fr_sub(d, one));
        Fr run_hi = (first + H == hit || first + H > n) ? one : d;
#pragma unroll 1
        for (int m = H + 1; m < I; m++) {
            const u64 node = first + m;
            sm[m - H - 1][t] = run_hi;
            d = fr_norm(fr_sub(d, one));
            run_hi = fr_mul(run_hi, (node == hit || node > n) ? one : d);
        }
        // c_j / (this point's thread product), and the running inverse moves on to the points before it
        Fr inv = inv_tp;
        if (l > 0) {
            inv = fr_mul(inv, slot[poly_lagr_set_slot_elem(l, t)]);
            slot[poly_lagr_set_slot_elem(l, t)] = fr_mul(inv_tp, fr_mul(run_lo, run_hi));
        }
        const Fr c = cw[j];
        inv = fr_mul(inv, c);
        const Fr inv_lo = fr_mul(inv, run_hi);  // c_j / (the lower half's product)
        inv = fr_mul(inv, run_lo);              // c_j / (the upper half's product)
        const Fr y = yq[2 * (u64)j], qm = yq[2 * (u64)j + 1];
        // upper half, from the last node down: c e = inv P, inv <- inv d_m.  d ends at node H - 1.
#pragma unroll 1
        for (int m = I - 1; m >= H; m--) {
            const u64 node = first + m;
            const bool at_hit = node == hit;
            Fr ce = inv;
            if (m > H) {
                ce = fr_mul(inv, sm[m - H - 1][t]);
                inv = fr_mul(inv, (at_hit || node > n) ? one : d);
            }
            d = fr_norm(fr_add(d, one));
            // a node behind n loads zero and is never stored
            const Fr left = at_hit ? qm : fr_sub(y, poly_scan_load(v, node - 1, n));
            const Fr sum = fr_norm(fr_add(acc[I - 1], fr_mul(left, at_hit ? c : ce)));
#pragma unroll
            for (int s = I - 1; s > 0; s--) acc[s] = acc[s - 1];
            acc[0] = sum;  // H turns to the right: item 0 is at H now
        }
        // lower half: its suffixes d_s .. d_{H-1}, s = 1 .. H - 1, at sm[s - 1].  d ends at the first node.
        Fr suf = (first + H - 1 == hit || first + H - 1 > n) ? one : d;
#pragma unroll 1
        for (int m = H - 1; m >= 1; m--) {
            const u64 node = first + m - 1;
            sm[m - 1][t] = suf;
            d = fr_norm(fr_add(d, one));
            if (m > 1) suf = fr_mul(suf, (node == hit || node > n) ? one : d);
        }
        // ... and from the first node up: c e = inv S, inv <- inv d_m
        inv = inv_lo;
#pragma unroll 1
        for (int m = 0; m < H; m++) {
            const u64 node = first + m;
            const bool at_hit = node == hit;
            Fr ce = inv;
            if (m < H - 1) {
                ce = fr_mul(inv, sm[m][t]);
                inv = fr_mul(inv, (at_hit || node > n) ? one : d);
            }
            d = fr_norm(fr_sub(d, one));
            const Fr left = at_hit ? qm : fr_sub(y, poly_scan_load(v, node - 1, n));
            const Fr sum = fr_norm(fr_add(acc[H], fr_mul(left, at_hit ? c : ce)));
            const Fr turn = acc[0];
#pragma unroll
            for (int s = 0; s < I - 1; s++) acc[s] = s + 1 == H ? sum : acc[s + 1];
            acc[I - 1] = turn;  // H turns to the left: every accumulator is back at its item
        }
    }
    u32* row = rows + poly_lagr_set_partial_word(g, first, n);
#pragma unroll
    for (int m = 0; m < I; m++)
        if (first + m <= n) poly_scan_store(row + 8 * m, fr_reduce(acc[m]));
}

}  // namespace ps
