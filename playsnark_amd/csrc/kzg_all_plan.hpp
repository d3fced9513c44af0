// Index arithmetic of the openings at EVERY node of the domain (kzg_all.hpp): the transform size of an n, the wrapped index of
// an offset, buffer sizes and the size limit.  Nothing of HIP in here: tests/host_kzg_all_plan.cpp compiles it for the host under
// ASan + UBSan and sweeps it against literal loops.
//
// One polynomial given by its n values v_i on the nodes 1 .. n and the Lagrange-form string L_i: the proofs of all n nodes are
//     pi_m = v_m K_m - U_m + g_m L_m,    U_m = sum_i kappa(m - i) (v_i L_i),   K_m = sum_i kappa(m - i) L_i,
//     kappa(d) = 1 / d for d != 0 and kappa(0) = 0
// -- Toeplitz products, run as cyclic convolutions of size S = 2^p >= 2n - 1:
//   x        the n inputs sit at the indices 0 .. n - 1 (node i at i - 1), zeros (identity points) up to S
//   kappa    kappa(d) sits at the index d mod S, d = -(n - 1) .. n - 1; since 2 (n - 1) < S the positive offsets (indices
//            1 .. n - 1) and the negative ones (indices S - n + 1 .. S - 1) never meet, and what lies between is zero
//   result   node m at the index m - 1
// kappa is antisymmetric: the sequence read backwards gives the NEGATED sums, so the sign of an index is what this header is for.
#pragma once
#include <cstdint>

#ifndef PS_HD  // (field.hpp's, where a kernel header comes first; nothing on the host)
#define PS_HD
#endif

namespace ps {

// n at most this: the transform over points indexes its S <= 2^31 points with 32 bits, so 2n - 1 <= 2^31
constexpr uint64_t KZG_ALL_MAX_N = (uint64_t)1 << 30;
constexpr int KZG_ALL_MAX_LOG = 31;
constexpr int KZG_ALL_SCALAR_BATCH = 2;        // the scalar side convolves w.v and w as one batch of two transforms
constexpr uint64_t KZG_ALL_XYZZ_BYTES = 224;   // a G1 point between the stages: four coordinates of 14 limbs (kzg_all.hpp asserts it)
constexpr uint64_t KZG_ALL_FP_BYTES = 56;      // a chain product of the batch normalisation

PS_HD constexpr bool kzg_all_size_ok(uint64_t n) { return n >= 1 && n <= KZG_ALL_MAX_N; }
// p: the smallest with 2^p >= 2n - 1 (n >= 1); 0 for n = 1
PS_HD constexpr int kzg_all_log(uint64_t n) {
    int p = 0;
    while (((uint64_t)1 << p) < 2 * n - 1) p++;
    return p;
}
PS_HD constexpr uint64_t kzg_all_size(uint64_t n) { return (uint64_t)1 << kzg_all_log(n); }

// the index of kappa(d) in the wrapped sequence of S = 2^p entries, |d| <= n - 1
PS_HD constexpr uint64_t kzg_all_kappa_index(int64_t d, int p) { return (uint64_t)d & (((uint64_t)1 << p) - 1); }
// ... and back: what an index t < S of the wrapped sequence holds -- kappa(+d) (returns d > 0), kappa(-d) (returns -d < 0), or
// nothing (returns 0: the entry is zero, as kappa(0) is)
PS_HD constexpr int64_t kzg_all_kappa_offset(uint64_t t, uint64_t n, int p) {
    const uint64_t S = (uint64_t)1 << p;
    if (t >= 1 && t <= n - 1) return (int64_t)t;
    if (t < S && S - t <= n - 1) return -(int64_t)(S - t);
    return 0;
}
// where the input of node i (1-based) goes and the result of node m comes from
PS_HD constexpr uint64_t kzg_all_node_index(uint64_t node) { return node - 1; }

// the buffers of a call, in elements: S points (the n results are normalised in place: their n chain products go behind the first
// n points, inside the S - n points the results do not use), S scalars of kappa's stored transform, 2 S of the scalar batch, and
// n each for the values in Montgomery form and for g
PS_HD constexpr uint64_t kzg_all_point_elems(uint64_t n) { return kzg_all_size(n); }
PS_HD constexpr uint64_t kzg_all_kappa_elems(uint64_t n) { return kzg_all_size(n); }
PS_HD constexpr uint64_t kzg_all_scalar_elems(uint64_t n) { return KZG_ALL_SCALAR_BATCH * kzg_all_size(n); }
PS_HD constexpr uint64_t kzg_all_value_elems(uint64_t n) { return n; }
// the normalisation fits the point buffer: n points and n chain products within S points (n >= 2; n = 1 runs no transform)
PS_HD constexpr bool kzg_all_normalise_fits(uint64_t n) {
    return n * (KZG_ALL_XYZZ_BYTES + KZG_ALL_FP_BYTES) <= kzg_all_point_elems(n) * KZG_ALL_XYZZ_BYTES;
}

}  // namespace ps
