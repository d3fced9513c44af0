// Kernels of ps_groth16_prove_batch (prove_batch.inc): K witnesses of one circuit under one Lagrange-form key.
//
// Whole-matrix forms of the single prover's per-proof kernels: the witnesses are a [K][m] matrix X (Montgomery), the wire
// values y = M X^T a [3][K][n] array (matrix, witness, gate), the sums' scalar vectors [K][n + 2] (A, B) and [K][LC] (C) in
// the unsplit layout of g16_quotient_stage, every witness's row back to back -- the virtual scalar array ps_msm_batch sorts.
// Per-proof randomness: `small` holds r_j, s_j, r_j s_j as plain limbs, 3 x 8 words per proof.
#pragma once
#include "quotient.hpp"

namespace ps {

// y[k][j][r] = sum_e M_k[r][e] x_j[col e]: k_spmv for every (matrix, witness, row); rows of more than SPMV_LONG_ROW entries
// are k_spmv_long_rows_batch's.  Grid: x over K * n, y = the matrix.
__global__ void __launch_bounds__(256) k_spmv_batch(Csr3 m, const Fr* __restrict__ X, u32 mvars, u32 n, u32 K, Fr* __restrict__ Y) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (u64)K * n) return;
    const u32 j = (u32)(idx / n), r = (u32)(idx % n);
    const CsrView& mk = m.m[blockIdx.y];
    if (mk.row_ptr[r + 1] - mk.row_ptr[r] > SPMV_LONG_ROW) return;
    Y[((size_t)blockIdx.y * K + j) * n + r] = spmv_row(mk, X + (size_t)j * mvars, r);
}
// one workgroup per (long row, witness) of ONE matrix: k_spmv_long_rows, value for value.  Grid: n_long * K, y = y[k].
__global__ void __launch_bounds__(256) k_spmv_long_rows_batch(const u32* __restrict__ row_ptr, const u32* __restrict__ col,
                                                              const Fr* __restrict__ val, const Fr* __restrict__ X, u32 mvars, u32 n,
                                                              Fr* __restrict__ y, const u32* __restrict__ long_rows, u32 n_long) {
    __shared__ Fr sm[256];
    const u32 r = long_rows[blockIdx.x % n_long], j = blockIdx.x / n_long;
    const Fr* x = X + (size_t)j * mvars;
    Fr acc = fr_zero();
    u32 cnt = 0;
    for (u32 e = row_ptr[r] + threadIdx.x; e < row_ptr[r + 1]; e += blockDim.x) {
        acc = fr_norm(fr_add(acc, fr_mul(val[e], x[col[e]])));
        if ((++cnt & 31u) == 0) acc = fr_reduce(acc);
    }
    sm[threadIdx.x] = fr_reduce(acc);
    __syncthreads();
    for (u32 stride = 128; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) sm[threadIdx.x] = fr_norm(fr_add(sm[threadIdx.x], sm[threadIdx.x + stride]));
        __syncthreads();
    }
    if (threadIdx.x == 0) y[(size_t)j * n + r] = fr_reduce(sm[0]);
}
// flags[j] != 0: witness j violates a gate (k_check_gates per witness)
__global__ void __launch_bounds__(256) k_check_gates_batch(const Fr* __restrict__ Y, u32 n, u32 K, u32* __restrict__ flags) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 kn = (u64)K * n;
    if (idx >= kn) return;
    if (!fr_is_zero(fr_sub(fr_mul(Y[idx], Y[kn + idx]), Y[2 * kn + idx]))) atomicOr(&flags[idx / n], 1u);
}

__device__ inline void copy_plain(u32* __restrict__ dst, const u32* __restrict__ src) {  // both 32-byte aligned
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    d4[0] = s4[0];
    d4[1] = s4[1];
}
// SA / SB: row j = [y_j (n values, plain) | small[3 j + which] | 1]   (which: 0 = r for A, 1 = s for B)
__global__ void __launch_bounds__(256) k_g16b_fill_ab(u32* __restrict__ out, const Fr* __restrict__ y, const u32* __restrict__ small,
                                                      int which, u32 n, u32 K) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 row = (u64)n + 2;
    if (idx >= (u64)K * row) return;
    const u32 j = (u32)(idx / row), i = (u32)(idx % row);
    u32* dst = out + 8 * idx;
    if (i < n) {
        fr_store_plain(dst, y[(size_t)j * n + i]);
    } else if (i == n) {
        copy_plain(dst, small + 8 * (3 * (size_t)j + (u32)which));
    } else {
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        d4[0] = make_uint4(1u, 0u, 0u, 0u);
        d4[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}
// SC: row j = [sol_j[diff .. diff + nn) | h_j (n - 1, written by k_fr_from_mont per witness) | s_j a_j + r_j b_j (n) | r_j s_j | s_j | r_j]
// -- every part but h.  Grid over K * (nn + n + 3) elements.
__global__ void __launch_bounds__(256) k_g16b_fill_c(u32* __restrict__ out, const u32* __restrict__ sols, const Fr* __restrict__ yA,
                                                     const Fr* __restrict__ yB, const u32* __restrict__ small, u32 n, u32 nn, u32 mvars,
                                                     u32 diff, u32 K) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 per = (u64)nn + n + 3, LC = (u64)nn + (n - 1) + n + 3;
    if (idx >= (u64)K * per) return;
    const u32 j = (u32)(idx / per), i = (u32)(idx % per);
    u32* rowp = out + 8 * ((u64)j * LC);
    const u32* sm = small + 8 * 3 * (size_t)j;
    if (i < nn) {
        copy_plain(rowp + 8 * (size_t)i, sols + 8 * ((size_t)j * mvars + diff + i));
    } else if (i < nn + n) {
        const u32 t = i - nn;
        u32 rw[8], sw[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { rw[q] = sm[q]; sw[q] = sm[8 + q]; }
        const Fr r = fr_to_mont(fr_from_words8(rw)), s = fr_to_mont(fr_from_words8(sw));
        const Fr a = yA[(size_t)j * n + t], b = yB[(size_t)j * n + t];
        fr_store_plain(rowp + 8 * ((size_t)nn + (n - 1) + t), fr_add(fr_mul(a, s), fr_mul(b, r)));  // k_fr_lincomb_plain
    } else {
        const u32 t = i - nn - n;  // 0: rs * Delta, 1: s * Alpha, 2: r * Beta
        copy_plain(rowp + 8 * ((size_t)nn + (n - 1) + n + t), sm + 8 * (t == 0 ? 2u : t == 1 ? 1u : 0u));
    }
}

}  // namespace ps
