// Index arithmetic of the set apply pass (poly_scan_set.hpp): point groups, the quotient's length and the store predicate that
// cuts its zero top, buffer sizes, the reduction step and the size limits.  Nothing of HIP in here:
// tests/host_poly_scan_set_plan.cpp compiles it for the host under ASan + UBSan and sweeps it against a literal loop.
//
// One polynomial p of n coefficients and a set S of k distinct points:  q = (p - r) / Z_S, Z_S = prod_j (X - z_j), r the
// interpolant of (z_j, p(z_j)).  By partial fractions 1 / Z_S = sum_j w_j / (X - z_j), w_j = 1 / prod_{l != j} (z_j - z_l), so
//     q = sum_j w_j q_j,   q_j = (p - p(z_j)) / (X - z_j)      (the rows of the linear scan, poly_scan_plan.hpp)
// whose top k - 1 coefficients cancel: q has n - k coefficients (none for n <= k).
//   group g     the points [g G, min(k, (g + 1) G)); the last group may be partial.  A workgroup owns one tile of one group
//               (blockIdx.x the tile, blockIdx.y the group) and writes partial row g: sum over ITS points of w_j q_j
//   partial     ceil(k / G) rows of n - k scalars; with one group the partial row is q, otherwise the rows are summed
//   stored      index i of the recurrence (q_{i-1} = h_i) is stored iff 1 <= i and i - 1 < n - k
#pragma once
#include "poly_scan_plan.hpp"

namespace ps {

constexpr int POLY_SCAN_SET_GROUP = 8;                    // G: points a workgroup folds into its accumulators
constexpr int POLY_SCAN_SET_REDUCE_EVERY = 32;            // points of a group between two fr_reduce of the accumulators
constexpr uint64_t PS_KZG_SET_MAX = 1024;                 // k at most this: weights and interpolation on the host are O(k^2)
static_assert((POLY_SCAN_SET_REDUCE_EVERY & (POLY_SCAN_SET_REDUCE_EVERY - 1)) == 0, "the kernel tests l & (EVERY - 1)");
static_assert(PS_KZG_SET_MAX < (uint64_t)POLY_SCAN_TILE, "the cut of the top k - 1 coefficients stays inside the last two tiles");

inline uint64_t poly_scan_set_groups(uint64_t k) { return (k + POLY_SCAN_SET_GROUP - 1) / POLY_SCAN_SET_GROUP; }
// points of group g (g < poly_scan_set_groups(k))
inline uint64_t poly_scan_set_group_len(uint64_t k, uint64_t g) {
    const uint64_t start = g * POLY_SCAN_SET_GROUP;
    return k - start < (uint64_t)POLY_SCAN_SET_GROUP ? k - start : (uint64_t)POLY_SCAN_SET_GROUP;
}
inline uint64_t poly_scan_set_last_group_len(uint64_t k) { return poly_scan_set_group_len(k, poly_scan_set_groups(k) - 1); }
// coefficients of the quotient by Z_S
inline uint64_t poly_scan_set_quotient_len(uint64_t n, uint64_t k) { return n > k ? n - k : 0; }
// is h_i stored (as q_{i-1})?  nq = poly_scan_set_quotient_len(n, k)
constexpr bool poly_scan_set_stored(uint64_t i, uint64_t nq) { return i >= 1 && i - 1 < nq; }
// does tile b store anything?  (its first index is b T)
constexpr bool poly_scan_set_tile_stores(uint64_t b, uint64_t nq) { return b * (uint64_t)POLY_SCAN_TILE <= nq && nq != 0; }
// is the accumulator reduced behind point l of its group?
constexpr bool poly_scan_set_reduce_after(uint64_t l) {
    return (l & (POLY_SCAN_SET_REDUCE_EVERY - 1)) == (uint64_t)POLY_SCAN_SET_REDUCE_EVERY - 1;
}

// elements of the buffers: the weights (k field elements), the partial rows (ceil(k / G) rows of n - k scalars of 8 words);
// totals and carries are the linear scan's (poly_scan_total_elems(n, k) field elements each)
inline uint64_t poly_scan_set_weight_elems(uint64_t k) { return k; }
inline uint64_t poly_scan_set_partial_words(uint64_t n, uint64_t k) { return 8 * poly_scan_set_groups(k) * poly_scan_set_quotient_len(n, k); }
// first word of entry i of partial row g
inline uint64_t poly_scan_set_partial_word(uint64_t g, uint64_t i, uint64_t nq) { return 8 * (g * nq + i); }

// 1 <= k <= PS_KZG_SET_MAX
inline bool poly_scan_set_points_ok(uint64_t k) { return k >= 1 && k <= PS_KZG_SET_MAX; }
// ... and k * n below 2^32, the scan's limit
inline bool poly_scan_set_size_ok(uint64_t n, uint64_t k) { return poly_scan_set_points_ok(k) && poly_scan_total_ok(n, k); }

}  // namespace ps
