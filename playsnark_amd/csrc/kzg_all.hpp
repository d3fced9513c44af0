// The KZG proofs of EVERY node of the domain for a polynomial given by its n values on 1 .. n, over the Lagrange-form string
// (ps_kzg_all_key_lagrange, ps_kzg_open_all_lagrange; index arithmetic in kzg_all_plan.hpp, host side in kzg.inc).
//
// The quotient of node m, (p - v_m) / (X - m), has the values (v_m - v_i) / (m - i) at the nodes i != m and, at m itself, the
// value the degree bound forces: g_m = (s_m - v_m c_m) / w_m with the barycentric weights w_i = (-1)^(n-i) / ((i-1)! (n-i)!).
// Summed over the string L_i = [l_i(tau)] G1 this is
//     pi_m = v_m K_m - U_m + g_m L_m
//     U_m = sum_i kappa(m - i) (v_i L_i)     points, once per call          kappa(d) = 1 / d, kappa(0) = 0
//     K_m = sum_i kappa(m - i) L_i           points, once per string
//     s_m = sum_i kappa(m - i) w_i v_i       scalars                        c_m = sum_i kappa(m - i) w_i
// -- four Toeplitz products with ONE multiplier, run as cyclic convolutions of size S = 2^p >= 2n - 1 against kappa's stored
// transform: the two over points by the NTT over points of lagrange.hpp (k_ec_ntt_stage, k_ec_scale), the two over scalars as a
// batch of two through ntt_conv.  The kernels here are what surrounds the transforms:
//   k_kzg_all_kappa     the wrapped multiplier: 1 / d = (d-1)! / d! from the domain's factorial tables, no inversion
//   k_kzg_all_weights   [w.v | w] zero-padded to 2 S, and the values in Montgomery form for the kernels below
//   k_kzg_all_finish    g_m, with 1 / w_m = (-1)^(n-m) (m-1)! (n-m)!
//   k_kzg_all_load      P_i = v_i L_i from the affine string into S XYZZ points, the identity beyond n
//   k_kzg_all_combine   v_m K_m - U_m + g_m L_m in place of U_m
// The two point kernels multiply by full-width scalars (ec_mul_fr: the points must lie in the subgroup of order r).  Each runs
// ONE multiplication at a time and keeps nothing but indices live across it -- the combine kernel parks its partial sum in the
// point buffer between its two products -- so that they need the registers and the scratch of k_ec_scale (the window table of
// ec_mul_glv) and no more (tests/test_code_object_kzg_all.py).
#pragma once
#include "kzg_all_plan.hpp"
#include "lagrange.hpp"

namespace ps {

static_assert(sizeof(Xyzz<Fp>) == KZG_ALL_XYZZ_BYTES && sizeof(Fp) == KZG_ALL_FP_BYTES, "the plan's buffer sizes are those of the G1 point types");

// dst[t] = kappa(d) for the offset d that the index t of the wrapped sequence holds, t < S = 2^p; 0 where it holds none
__global__ void __launch_bounds__(256) k_kzg_all_kappa(Fr* __restrict__ dst, const Fr* __restrict__ fact, const Fr* __restrict__ invfact, u64 n, int p) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1ull << p)) return;
    const int64_t d = kzg_all_kappa_offset(t, n, p);
    if (d == 0) { dst[t] = fr_zero(); return; }
    const u64 a = d < 0 ? (u64)(-d) : (u64)d;
    const Fr inv = fr_mul(fact[a - 1], invfact[a]);
    dst[t] = d < 0 ? fr_neg(inv) : inv;
}

// x[j] = w_{j+1} v_{j+1}, x[S + j] = w_{j+1} for j < n, zero up to S in both halves; vm[j] = v_{j+1} in Montgomery form.
// v: the values as plain 8 x 32-bit words.
__global__ void __launch_bounds__(256) k_kzg_all_weights(Fr* __restrict__ x, Fr* __restrict__ vm, const u32* __restrict__ v,
                                                         const Fr* __restrict__ invfact, u64 n, int p) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ((u64)KZG_ALL_SCALAR_BATCH << p)) return;
    const u64 j = idx & ((1ull << p) - 1);
    if (j >= n) { x[idx] = fr_zero(); return; }
    Fr w = fr_mul(invfact[j], invfact[n - 1 - j]);
    if ((idx >> p) == 0) {
        u32 words[8];
#pragma unroll
        for (int k = 0; k < 8; k++) words[k] = v[8 * j + k];
        const Fr val = fr_to_mont(fr_from_words8(words));
        vm[j] = val;
        w = fr_mul(w, val);
    }
    x[idx] = ((n - 1 - j) & 1) ? fr_neg(w) : w;
}

// g[j] = (s - v c) / w for node j + 1: s = conv[j], c = conv[S + j] (the two convolutions), 1 / w = (-1)^(n-1-j) j! (n-1-j)!
__global__ void __launch_bounds__(256) k_kzg_all_finish(Fr* __restrict__ g, const Fr* __restrict__ conv, const Fr* __restrict__ vm,
                                                        const Fr* __restrict__ fact, u64 n, int p) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const Fr num = fr_norm(fr_sub(conv[j], fr_mul(vm[j], conv[(1ull << p) + j])));
    const Fr r = fr_mul(num, fr_mul(fact[j], fact[n - 1 - j]));
    g[j] = ((n - 1 - j) & 1) ? fr_neg(r) : r;
}

// an affine point of an array as XYZZ ((0, 0) is the identity)
template <class KF>
__device__ inline Xyzz<KF> kzg_all_ld_point(const Affine<typename FieldTraits<KF>::Store>* p) {
    const Affine<KF> a = ld_affine<KF>(p);
    return affine_is_identity<KF>(a) ? xyzz_identity<KF>() : xyzz_from_affine<KF>(a.x, a.y);
}

// buf[i] = i < n ? vm[i] * lag[i] : O, i < total
template <class KF>
__global__ void __launch_bounds__(256, PS_EC_WAVES(KF)) k_kzg_all_load(const Affine<typename FieldTraits<KF>::Store>* __restrict__ lag,
                                                                       const Fr* __restrict__ vm, u32 n, u32 total,
                                                                       Xyzz<typename FieldTraits<KF>::Store>* __restrict__ buf) {
    const u32 i = logical_tid<KF>();
    if (i >= total) return;
    if (i >= n) { st_xyzz<KF>(&buf[i], xyzz_identity<KF>()); return; }
    st_xyzz<KF>(&buf[i], ec_mul_fr<KF>(kzg_all_ld_point<KF>(&lag[i]), vm[i]));
}

// buf[i] = vm[i] * key[i] - buf[i] + g[i] * lag[i], i < n: step 0 leaves vm[i] key[i] - U in buf[i], step 1 adds g[i] lag[i]
template <class KF>
__global__ void __launch_bounds__(256, PS_EC_WAVES(KF)) k_kzg_all_combine(Xyzz<typename FieldTraits<KF>::Store>* __restrict__ buf,
                                                                          const Affine<typename FieldTraits<KF>::Store>* __restrict__ key,
                                                                          const Affine<typename FieldTraits<KF>::Store>* __restrict__ lag,
                                                                          const Fr* __restrict__ vm, const Fr* __restrict__ g, u32 n) {
    const u32 i = logical_tid<KF>();
    if (i >= n) return;
#pragma unroll 1
    for (int step = 0; step < 2; step++) {
        const Xyzz<KF> t = ec_mul_fr<KF>(kzg_all_ld_point<KF>(step ? &lag[i] : &key[i]), step ? g[i] : vm[i]);
        Xyzz<KF> acc = ld_xyzz<KF>(&buf[i]);
        if (step == 0) acc = xyzz_neg<KF>(acc);
        xyzz_add<KF>(acc, t);
        st_xyzz<KF>(&buf[i], acc);
    }
}

}  // namespace ps
