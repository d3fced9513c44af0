// Pass arithmetic of ps_msm_batch_multi: K scalar vectors over A point arrays, one sort per pass shared by all arrays.  The
// passes are those of ps_msm_batch (msm_batch_plan.hpp) under two more conditions.  No HIP in here:
// tests/host_msm_batch_multi_plan.cpp compiles it for the host alone.
//
//   groups    the arrays of a call may mix G1 and G2 and share ONE Kc, so the byte limit is applied with the point size of
//             the largest group present: every array's buckets and partial slots then fit what was planned.
//   stride    member j of a pass reads its n scalars at scalar index j * stride + t (t < n) from a base advanced to the
//             pass's first member; k_sort_count_batch holds that index in 32 bits, so (Kc - 1) * stride + n - 1 < 2^32.
//             A packed batch (stride == n) is bound more tightly by the entry limit already: the stride limit never shortens
//             a pass of ps_msm_batch.
// The caller has checked first + n <= stride, so a member never reads into its neighbour.
#pragma once
#include "msm_batch_plan.hpp"

// point size a mixed call is planned with
static inline uint64_t batch_multi_point_bytes(bool any_g1, bool any_g2, uint64_t g1_bytes, uint64_t g2_bytes) {
    if (any_g2) return g2_bytes;
    return any_g1 ? g1_bytes : 0;
}

// The largest number of members one pass may hold under member stride `stride` (>= s.n); 0: not even one member fits.
static inline uint64_t batch_multi_members(const BatchShape& s, const BatchLimits& l, uint64_t stride) {
    uint64_t kc = batch_pass_members(s, l);
    if (kc == 0 || stride < s.n || s.n > (1ull << 32)) return 0;
    const uint64_t room = (1ull << 32) - s.n;  // (kc - 1) * stride <= room
    if (stride) kc = std::min(kc, room / stride + 1);
    return kc;
}

// The passes of K members: as batch_passes, with the stride limit.
static inline bool batch_multi_passes(uint64_t K, const BatchShape& s, const BatchLimits& l, uint64_t stride, std::vector<BatchPass>* out) {
    out->clear();
    if (K == 0) return true;
    const uint64_t kc = batch_multi_members(s, l, stride);
    if (kc == 0) return false;
    for (uint64_t first = 0; first < K; first += kc) out->push_back({first, std::min(kc, K - first)});
    return true;
}
