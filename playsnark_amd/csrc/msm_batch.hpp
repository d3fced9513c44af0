// ps_msm_batch: K scalar vectors over ONE point array as one bucket problem of K * W bucket sets -- the dual of
// ps_msm_multi (k point arrays, one scalar vector, one sort).
//
// A small sum leaves the chip idle: its time is launches and a chain of dependent additions.  The members of a batch share
// all of that.  The sort below runs over the VIRTUAL scalar array of N = Kc * n entries (Kc members of a pass, back to
// back): entry j belongs to member j / n, names point j % n, and its digit of window w goes to bucket
// ((j / n) * W + w) * NB + digit - 1.  A workgroup's chunk of the virtual array may straddle members, so the member is found
// per thread.  Behind these two kernels nothing knows about the batch: k_sort_scan, k_sort_fine and k_sort_big_* see keys
// below G = Kc * W * NB, the accumulation, fix-up and reduction (msm.hpp, qtail.hpp) see `sets = Kc * W` bucket sets of a
// plain plan.  k_batch_fold then does per member what msm_fold_host does for one sum.
//
// Over a window table T[w][i] = 2^(c w) P[i] (k_sort_*_batch_tab) all windows of a member share ONE bucket set: the digit of
// window w of entry j goes to bucket (j / n) * NB + digit - 1 and the entry carries w in its tag bits, as k_sort_partition
// tags the entries of a single tabled sum.  A pass then has Kc sets instead of Kc * W, G = Kc * NB, and a member's set sum
// IS its result: nothing to fold.
#pragma once
#include "msm.hpp"

namespace ps {

// k_sort_count over the virtual array: codes[w][j] for j < N, coarse histogram of the batch keys.  Member j's scalars start
// at scalar index j * stride (stride >= n: ps_msm_batch packs its members, stride == n, and reads the addresses it always
// read; ps_msm_batch_multi reads n scalars out of each solution vector and never touches what lies between them)
__global__ void __launch_bounds__(DIGITS_THREADS) k_sort_count_batch(const u32* __restrict__ scalars, u32 n, u32 stride, u32 N, int c, int W, u32 NB,
                                                                     DigitConst cadd, int fold_neg, u32 ncoarse, int fb,
                                                                     u32* __restrict__ codes, u32* __restrict__ coarse_cnt) {
    PS_TAIL_PRIO_HERE;
    __shared__ u32 hist[SORT_MAX_COARSE];
    const u32 tid = threadIdx.x;
    hist[tid] = 0;  // DIGITS_THREADS == SORT_MAX_COARSE
    __syncthreads();
    for (int j = 0; j < COUNT_PER_THREAD; j++) {
        const u32 i = (blockIdx.x * COUNT_PER_THREAD + (u32)j) * DIGITS_THREADS + tid;
        const bool in = i < N;
        u32 k[8], carry = 0, flip = 0;
        const u32 mem = in ? i / n : 0u;  // this entry's member
        if (in) scalar_plus_c(scalars, mem * stride + (i - mem * n), cadd, fold_neg, k, carry, flip);
        const u32 set0 = mem * (u32)W;  // first bucket set of the member
        for (int w = 0; w < W; w++) {  // uniform trip count: lds_count is called by whole waves
            u32 code = 0xffffffffu;
            if (in) {
                code = digit_from(k, carry, c, W, w, NB, flip);
                codes[(size_t)w * N + i] = code;
            }
            const bool act = code != 0xffffffffu;
            const u32 key = act ? (set0 + (u32)w) * NB + (code & 0x7fffffffu) : 0u;
            lds_count(hist, key >> fb, act);
        }
    }
    __syncthreads();
    if (tid < ncoarse && hist[tid]) atomicAdd(&coarse_cnt[tid], hist[tid]);
}

// k_sort_count_batch over a window table: the same codes, the key names the member's ONE bucket set.  (A kernel of its own,
// not a shared inlined body: with the body shared, k_sort_partition_batch no longer kept its sixteen waves of 64 registers.)
__global__ void __launch_bounds__(DIGITS_THREADS) k_sort_count_batch_tab(const u32* __restrict__ scalars, u32 n, u32 stride, u32 N, int c, int W, u32 NB,
                                                                     DigitConst cadd, int fold_neg, u32 ncoarse, int fb,
                                                                     u32* __restrict__ codes, u32* __restrict__ coarse_cnt) {
    PS_TAIL_PRIO_HERE;
    __shared__ u32 hist[SORT_MAX_COARSE];
    const u32 tid = threadIdx.x;
    hist[tid] = 0;  // DIGITS_THREADS == SORT_MAX_COARSE
    __syncthreads();
    for (int j = 0; j < COUNT_PER_THREAD; j++) {
        const u32 i = (blockIdx.x * COUNT_PER_THREAD + (u32)j) * DIGITS_THREADS + tid;
        const bool in = i < N;
        u32 k[8], carry = 0, flip = 0;
        const u32 mem = in ? i / n : 0u;  // this entry's member
        if (in) scalar_plus_c(scalars, mem * stride + (i - mem * n), cadd, fold_neg, k, carry, flip);
        for (int w = 0; w < W; w++) {  // uniform trip count: lds_count is called by whole waves
            u32 code = 0xffffffffu;
            if (in) {
                code = digit_from(k, carry, c, W, w, NB, flip);
                codes[(size_t)w * N + i] = code;
            }
            const bool act = code != 0xffffffffu;
            const u32 key = act ? mem * NB + (code & 0x7fffffffu) : 0u;  // the member's one bucket set
            lds_count(hist, key >> fb, act);
        }
    }
    __syncthreads();
    if (tid < ncoarse && hist[tid]) atomicAdd(&coarse_cnt[tid], hist[tid]);
}

// k_sort_partition over the virtual array: (fine key, point index | sign) into the coarse bin's region
__global__ void __launch_bounds__(DIGITS_THREADS, 8) k_sort_partition_batch(const u32* __restrict__ codes, u32 n, u32 N, int W, u32 NB, int fb,
                                                                         u32* __restrict__ coarse_cur,
                                                                         unsigned short* __restrict__ part_key,
                                                                         u32* __restrict__ part_val) {
    PS_TAIL_PRIO_HERE;
    __shared__ u32 hist[SORT_MAX_COARSE], binstart[SORT_MAX_COARSE], gbase[SORT_MAX_COARSE];
    __shared__ u32 wtot[DIGITS_THREADS / 64];
    extern __shared__ __align__(16) unsigned char dg_smem[];
    u32* lkey = reinterpret_cast<u32*>(dg_smem);
    u32* lval = lkey + DIGITS_CHUNK;
    const u32 w = blockIdx.y;
    const u32 chunk_base = blockIdx.x * DIGITS_CHUNK;
    const u32 tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    u32 dig[DIGITS_PER_THREAD], keyb[DIGITS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DIGITS_PER_THREAD; j++) {
        const u32 i = chunk_base + j * DIGITS_THREADS + tid;
        const u32 code = i < N ? codes[(size_t)w * N + i] : 0xffffffffu;
        dig[j] = code;
        const bool act = code != 0xffffffffu;
        keyb[j] = act ? ((i / n) * (u32)W + w) * NB : 0u;
        lds_count(hist, act ? (keyb[j] + (code & 0x7fffffffu)) >> fb : 0u, act);
    }
    __syncthreads();
    // exclusive scan of the 1024 bins, one per thread; reserve each non-empty bin's run in its global region
    const u32 cnt = hist[tid];
    const u32 inc = wave_incl_scan(cnt);
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int q = 0; q < DIGITS_THREADS / 64; q++) {
        const u32 t = wtot[q];
        if (q < (int)(tid >> 6)) before += t;
        total += t;
    }
    const u32 ex = before + inc - cnt;
    __syncthreads();
    binstart[tid] = ex;
    hist[tid] = ex;  // now the bin's fill cursor
    gbase[tid] = cnt ? atomicAdd(&coarse_cur[tid], cnt) : 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DIGITS_PER_THREAD; j++) {
        const u32 code = dig[j];
        const bool act = code != 0xffffffffu;
        const u32 key = act ? keyb[j] + (code & 0x7fffffffu) : 0u;
        const u32 pos = lds_rank(hist, key >> fb, act);
        if (act) {
            const u32 i = chunk_base + j * DIGITS_THREADS + tid;
            lkey[pos] = key;
            lval[pos] = (i % n) | (code & 0x80000000u);
        }
    }
    __syncthreads();
    for (u32 p = tid; p < total; p += DIGITS_THREADS) {
        const u32 key = lkey[p], b = key >> fb;
        const u32 dst = gbase[b] + (p - binstart[b]);
        part_key[dst] = (unsigned short)(key & ((1u << fb) - 1u));
        part_val[dst] = lval[p];
    }
}

// k_sort_partition_batch over a window table: (fine key of the member's one set, point index | sign | window tag), as
// k_sort_partition tags the entries of a single tabled sum.  `W` is not needed for the key; the argument list stays that of
// k_sort_partition_batch.
__global__ void __launch_bounds__(DIGITS_THREADS, 8) k_sort_partition_batch_tab(const u32* __restrict__ codes, u32 n, u32 N, int W, u32 NB, int fb,
                                                                         u32* __restrict__ coarse_cur,
                                                                         unsigned short* __restrict__ part_key,
                                                                         u32* __restrict__ part_val) {
    PS_TAIL_PRIO_HERE;
    __shared__ u32 hist[SORT_MAX_COARSE], binstart[SORT_MAX_COARSE], gbase[SORT_MAX_COARSE];
    __shared__ u32 wtot[DIGITS_THREADS / 64];
    extern __shared__ __align__(16) unsigned char dg_smem[];
    u32* lkey = reinterpret_cast<u32*>(dg_smem);
    u32* lval = lkey + DIGITS_CHUNK;
    const u32 w = blockIdx.y;
    const u32 wtag = w << ENTRY_W_SHIFT;  // the entry names its window (n < 2^26, W <= 32: 26 and 5 bits)
    const u32 chunk_base = blockIdx.x * DIGITS_CHUNK;
    const u32 tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    u32 dig[DIGITS_PER_THREAD], keyb[DIGITS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DIGITS_PER_THREAD; j++) {
        const u32 i = chunk_base + j * DIGITS_THREADS + tid;
        const u32 code = i < N ? codes[(size_t)w * N + i] : 0xffffffffu;
        dig[j] = code;
        const bool act = code != 0xffffffffu;
        keyb[j] = act ? (i / n) * NB : 0u;
        lds_count(hist, act ? (keyb[j] + (code & 0x7fffffffu)) >> fb : 0u, act);
    }
    __syncthreads();
    // exclusive scan of the 1024 bins, one per thread; reserve each non-empty bin's run in its global region
    const u32 cnt = hist[tid];
    const u32 inc = wave_incl_scan(cnt);
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int q = 0; q < DIGITS_THREADS / 64; q++) {
        const u32 t = wtot[q];
        if (q < (int)(tid >> 6)) before += t;
        total += t;
    }
    const u32 ex = before + inc - cnt;
    __syncthreads();
    binstart[tid] = ex;
    hist[tid] = ex;  // now the bin's fill cursor
    gbase[tid] = cnt ? atomicAdd(&coarse_cur[tid], cnt) : 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DIGITS_PER_THREAD; j++) {
        const u32 code = dig[j];
        const bool act = code != 0xffffffffu;
        const u32 key = act ? keyb[j] + (code & 0x7fffffffu) : 0u;
        const u32 pos = lds_rank(hist, key >> fb, act);
        if (act) {
            const u32 i = chunk_base + j * DIGITS_THREADS + tid;
            lkey[pos] = key;
            lval[pos] = (i % n) | (code & 0x80000000u) | wtag;
        }
    }
    __syncthreads();
    for (u32 p = tid; p < total; p += DIGITS_THREADS) {
        const u32 key = lkey[p], b = key >> fb;
        const u32 dst = gbase[b] + (p - binstart[b]);
        part_key[dst] = (unsigned short)(key & ((1u << fb) - 1u));
        part_val[dst] = lval[p];
    }
}


// Horner over a member's W set sums (k_reduce_weights made them): acc = S_{W-1}, then acc = 2^c acc + S_w downwards.  One
// logical thread per member (a lane pair for G2): a serial chain of (W - 1) * c doublings and W - 1 additions, all members
// side by side.
template <class KF>
__global__ void __launch_bounds__(256, PS_TAIL_WAVES) k_batch_fold(const Xyzz<typename FieldTraits<KF>::Store>* __restrict__ sets, u32 members,
                                                       int W, int c, Xyzz<typename FieldTraits<KF>::Store>* __restrict__ out) {
    PS_TAIL_PRIO_HERE;
    const u32 m = logical_tid<KF>();
    if (m >= members) return;
    const Xyzz<typename FieldTraits<KF>::Store>* S = sets + (size_t)m * (u32)W;
    Xyzz<KF> acc = ld_xyzz<KF>(&S[W - 1]);
#pragma unroll 1
    for (int w = W - 2; w >= 0; w--) {
#pragma unroll 1
        for (int i = 0; i < c; i++) acc = xyzz_dbl_inl<KF>(acc);
        const Xyzz<KF> v = ld_xyzz<KF>(&S[w]);
        xyzz_add_inl<KF>(acc, v);
    }
    st_xyzz<KF>(&out[m], acc);
}

}  // namespace ps
