// Device side of ps_groth16_verify_batch_locate (verify_locate.inc): the trees of partial results the bisection reads.
// Included by capi.hip after pairing_dev.hpp; its PS_HD part alone (the index arithmetic and the modular addition of plain
// words) by tests/host_locate_index.cpp, which runs it on the host under ASan + UBSan; tests/device_locate_check.hip
// includes it whole and launches k_g1_pair_sums and k_fr_row_pair_sums directly (tests/test_device_locate.py: every node
// of every level against Python integers and the oracle's point addition).  The descent over these trees is locate_bisect
// (locate_descent.hpp, on top of the PS_HD part), which the same host test runs as it ships.
//
// Every tree is laid out as the product tree of k_f12_product: level 0 holds one value per proof, level l + 1 has
// ceil(n_l / 2) nodes, node i combines nodes 2i and 2i + 1 of the level below and the odd one out is carried up unchanged.
// Node (l, i) therefore covers the proofs [i 2^l, min((i + 1) 2^l, N)).  All levels are kept, one behind the other.
//   F tree      Fp12 values, k_miller_batch then k_f12_product per level (pairing_dev.hpp, unchanged)
//   C tree      rho_i C_i in XYZZ form (k_ec_scale), one k_g1_pair_sums per level
//   scalar tree rows of diff + 1 plain canonical words8: rho_i, then rho_i io_ij (k_fr_locate_rows), one k_fr_row_pair_sums
//               per level: column 0 of a node is R_S, columns 1 .. diff are t_S
// Per round of the descent k_gather_words picks the rows, points and Fp12 values of the K sets under test, one launch per
// array; X_S = sum_j t_S,j IoLP_j is k_ec_scale over IoLP repeated K times, then k_g1_pair_sums over K segments of diff points.
#pragma once
#include "field.hpp"

namespace ps {
namespace locate {

constexpr int MAX_LEVELS = 34;  // a tree over n < 2^32 leaves has at most 33 levels

// Sizes and offsets (in nodes) of the levels of a tree over n >= 1 leaves; returns the number of levels L + 1 (the root is
// level L, alone).  off[L + 1] is the total number of nodes: below 2 n + 32.
PS_HD inline int tree_levels(u64 n, u64* size, u64* off) {
    int l = 0;
    u64 at = 0;
    for (u64 m = n;; m = (m + 1) / 2) {
        size[l] = m;
        off[l] = at;
        at += m;
        l++;
        if (m <= 1) break;
    }
    off[l] = at;
    return l;
}
// Leaves [lo, hi) under node i of level l of a tree over n leaves
PS_HD inline void node_range(int l, u64 i, u64 n, u64* lo, u64* hi) {
    *lo = i << l;
    const u64 end = (i + 1) << l;
    *hi = end < n ? end : n;
}
// Node i of a level whose level BELOW has `below` nodes: two children (2i, 2i + 1), or the carried node 2i alone
PS_HD inline bool node_has_two_children(u64 i, u64 below) { return 2 * i + 1 < below; }
// First value of level l of an F tree whose level 0 is followed by `diff` more values (the loops with the key's points of a
// PHGR13 batch, locate_phgr13_dev.hpp; 0 for Groth16: off[l])
PS_HD inline u64 f_level_base(const u64* off, int l, u64 diff) { return off[l] + (l > 0 ? diff : 0); }

// acc = acc + x mod r for plain canonical words (both below r < 2^255: the sum fits 256 bits)
PS_HD inline void words8_add_mod_r(u32* acc, const u32* x) {
    u64 carry = 0;
    for (int i = 0; i < 8; i++) {
        const u64 s = (u64)acc[i] + x[i] + carry;
        acc[i] = (u32)s;
        carry = s >> 32;
    }
    u32 d[8];
    u64 borrow = 0;
    for (int i = 0; i < 8; i++) {
        const u64 t = (u64)acc[i] - FrParams::mod(i) - borrow;
        d[i] = (u32)t;
        borrow = (t >> 63) & 1;
    }
    if (!borrow)
        for (int i = 0; i < 8; i++) acc[i] = d[i];
}

}  // namespace locate
}  // namespace ps

#if defined(__HIPCC__) || defined(__HIP__)
namespace ps {

// One level of `segs` trees of G1 points side by side: segment s reads n nodes at in + s * in_stride and writes
// ceil(n / 2) at out + s * out_stride; out[i] = in[2i] + in[2i + 1], or in[2i] for the carried node.  The addition is
// the complete one of curve.hpp: identity operands, equal operands (the doubling) and P + (-P) are ordinary inputs.
// One thread per output node; segs * ceil(n / 2) < 2^32 (the host keeps it below 2^21).  Registers: one XYZZ addition with
// both operands alive, the shape of k_fixup_pair -- two waves per SIMD (<= 256 registers), like every tail kernel.
__global__ void __launch_bounds__(256, PS_TAIL_WAVES) k_g1_pair_sums(const Xyzz<Fp>* __restrict__ in, u32 n, u32 segs, u32 in_stride,
                                                                     Xyzz<Fp>* __restrict__ out, u32 out_stride) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, h = (n + 1) / 2;
    if (t >= segs * h) return;
    const u32 seg = t / h, i = t - seg * h;
    const Xyzz<Fp>* src = in + (size_t)seg * in_stride;
    Xyzz<Fp> acc = src[2 * i];
    if (2 * i + 1 < n) {
        const Xyzz<Fp> right = src[2 * i + 1];
        xyzz_add_inl<Fp>(acc, right);
    }
    out[(size_t)seg * out_stride + i] = acc;
}

// One level of the scalar tree: rows of `cols` plain canonical words8; out[i][j] = in[2i][j] + in[2i + 1][j] mod r, or
// in[2i][j] for the carried node.  Neighbouring lanes take neighbouring columns of a row, as k_fr_weighted_columns reads.
__global__ void __launch_bounds__(256) k_fr_row_pair_sums(const u32* __restrict__ in, u32 n, u32 cols, u32* __restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (u64)((n + 1) / 2) * cols) return;
    const u64 i = t / cols, j = t - i * cols;
    const u32* a = in + ((2 * i) * cols + j) * 8;
    u32 x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = a[k];
    if (2 * i + 1 < n) {
        const u32* b = a + (u64)cols * 8;
        u32 y[8];
#pragma unroll
        for (int k = 0; k < 8; k++) y[k] = b[k];
        locate::words8_add_mod_r(x, y);
    }
    u32* dst = out + t * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = x[k];
}

// Level 0 of the scalar tree: row i = (rho_i, rho_i io_i0, .., rho_i io_i,diff-1), plain canonical words8.  rho in both of
// its forms (plain words, Montgomery); the products are fr_weighted_column's over the one row.
__global__ void __launch_bounds__(256) k_fr_locate_rows(const u32* __restrict__ rho, const Fr* __restrict__ rho_mont, const u32* __restrict__ io,
                                                       u32 rows, u32 diff, u32* __restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 cols = diff + 1;
    if (t >= (u64)rows * cols) return;
    const u32 i = (u32)(t / cols), j = (u32)(t - (u64)i * cols);
    u32 x[8];
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = rho[(size_t)i * 8 + k];
    } else {
        fr_to_words8(x, fr_weighted_column(rho_mont, io, diff, j - 1, i, i + 1));
    }
    u32* dst = out + t * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = x[k];
}

// out[e][0 .. w) = in[(idx ? idx[e] : e) * stride + off + (0 .. w)], e < count, in 32-bit words: the values of the sets
// under test out of a level of a tree (idx: their nodes), one column range of their rows (off, w), the first node of every
// segment (idx = nullptr, stride = the segment stride), or one array repeated (idx = nullptr, stride = 0).
__global__ void __launch_bounds__(256) k_gather_words(const u32* __restrict__ in, const u32* __restrict__ idx, u32 count, u64 stride, u64 off, u32 w,
                                                     u32* __restrict__ out) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (u64)count * w) return;
    const u64 e = t / w, x = t - e * w;
    out[t] = in[(u64)(idx ? idx[e] : (u32)e) * stride + off + x];
}

}  // namespace ps
#endif
