// Index arithmetic of the value-form set quotient (poly_lagrange_set.hpp): point groups, (tile, group, thread, item) <-> (node,
// point), the thread-private LDS slots of the fold, partial-row offsets, buffer sizes and the size limits.  Nothing of HIP in
// here: tests/host_poly_lagrange_set_plan.cpp compiles it for the host under ASan + UBSan and sweeps it against literal loops.
//
// One polynomial given by its n values on the nodes 1 .. n (poly_lagrange_plan.hpp) and a set S of k distinct points:
//     q = (p - r) / Z_S = sum_j c_j (p - y_j) / (X - z_j),   c_j = 1 / prod_{l != j} (z_j - z_l)
// as its n values on the same nodes (all zero for k >= n).
//   group g     the points [g G, min(k, (g + 1) G)); the last group may be partial.  A workgroup owns one tile of one group
//               (blockIdx.x the tile, blockIdx.y the group) and writes partial row g: sum over ITS points of c_j q_j(i)
//   partial     ceil(k / G) rows of n scalars; with one group the partial row is the result and nothing else is allocated,
//               otherwise the rows are summed into it
//   slot        a thread keeps, per point of its group but the first, the product of its own differences over the points before
//               it: G - 1 arrays of 256 field elements in LDS, element [l - 1][t], read and written by thread t alone
#pragma once
#include "poly_lagrange_plan.hpp"
#include "poly_scan_set_plan.hpp"

namespace ps {

#ifdef PS_LAGR_SET_GROUP
constexpr int POLY_LAGR_SET_GROUP = PS_LAGR_SET_GROUP;    // an A/B build (tools/kzg_set_lagrange_sweep.py)
#else
constexpr int POLY_LAGR_SET_GROUP = 4;                    // G: points that share one inversion per tile
#endif
constexpr uint64_t POLY_LAGR_SET_MAX = PS_KZG_SET_MAX;    // k at most this: the weights on the host are O(k^2)
constexpr int POLY_LAGR_SET_FR_BYTES = 40;                // a field element in LDS: ten 32-bit limbs
constexpr int POLY_LAGR_SET_LDS_MAX = 64 * 1024;          // static LDS of a workgroup
static_assert(POLY_LAGR_SET_GROUP >= 1 && POLY_LAGR_SET_GROUP <= 32, "a node's sum of G products is reduced once, behind the group");
static_assert(POLY_LAGR_SET_MAX / POLY_LAGR_SET_GROUP + 1 <= POLY_LAGR_MAX_POINTS_PER_LAUNCH, "blockIdx.y picks the group");

inline uint64_t poly_lagr_set_groups(uint64_t k) { return (k + POLY_LAGR_SET_GROUP - 1) / POLY_LAGR_SET_GROUP; }
// points of group g (g < poly_lagr_set_groups(k))
inline uint64_t poly_lagr_set_group_len(uint64_t k, uint64_t g) {
    const uint64_t start = g * POLY_LAGR_SET_GROUP;
    return k - start < (uint64_t)POLY_LAGR_SET_GROUP ? k - start : (uint64_t)POLY_LAGR_SET_GROUP;
}
// the point that is number l of group g, and back
constexpr uint64_t poly_lagr_set_point(uint64_t g, uint64_t l) { return g * POLY_LAGR_SET_GROUP + l; }
constexpr uint64_t poly_lagr_set_point_group(uint64_t j) { return j / POLY_LAGR_SET_GROUP; }
constexpr uint64_t poly_lagr_set_point_slot(uint64_t j) { return j % POLY_LAGR_SET_GROUP; }
// (tile b, group g, thread t, item m, number l in the group) is the pair (node, point); nodes above n and points from k on
// take no part
constexpr uint64_t poly_lagr_set_node(uint64_t b, uint64_t t, uint64_t m) { return poly_lagr_node(b, t, m); }

// A thread unwinds its I nodes as two halves of H, over H - 1 products of either half
constexpr int POLY_LAGR_SET_HALF = POLY_LAGR_ITEMS / 2;
static_assert(POLY_LAGR_ITEMS == 2 * POLY_LAGR_SET_HALF && POLY_LAGR_SET_HALF >= 2, "two halves of two nodes at least");
// LDS of the fold, in arrays of 256 field elements: the prefix and the suffix products of the scan (one array each: a step
// reads, waits, writes, waits), which are the thread's own H - 1 half products afterwards; the G - 1 slot arrays; and the inverse
constexpr uint64_t POLY_LAGR_SET_SCRATCH_ARRAYS = POLY_LAGR_SET_HALF - 1 > 2 ? POLY_LAGR_SET_HALF - 1 : 2;
constexpr uint64_t POLY_LAGR_SET_SLOT_ARRAYS = POLY_LAGR_SET_GROUP > 1 ? POLY_LAGR_SET_GROUP - 1 : 1;  // (no array of none)
constexpr uint64_t POLY_LAGR_SET_LDS_ELEMS = (POLY_LAGR_SET_SCRATCH_ARRAYS + POLY_LAGR_SET_SLOT_ARRAYS) * POLY_LAGR_THREADS + 1;
static_assert(POLY_LAGR_SET_LDS_ELEMS * POLY_LAGR_SET_FR_BYTES <= (uint64_t)POLY_LAGR_SET_LDS_MAX,
              "the slots of G points and the half products of I nodes fit a workgroup's LDS (I = 16 does not: G = 4 is for I <= 8)");
// the slot of point number l >= 1 of a group, for thread t: element of the slot arrays
constexpr uint64_t poly_lagr_set_slot_elem(uint64_t l, uint64_t t) { return (l - 1) * POLY_LAGR_THREADS + t; }

// the partial rows: none beside the result for one group
inline uint64_t poly_lagr_set_partial_rows(uint64_t k) { return poly_lagr_set_groups(k) > 1 ? poly_lagr_set_groups(k) : 0; }
inline uint64_t poly_lagr_set_partial_words(uint64_t n, uint64_t k) { return 8 * poly_lagr_set_partial_rows(k) * n; }
// first word of node i (1-based) of partial row g
constexpr uint64_t poly_lagr_set_partial_word(uint64_t g, uint64_t i, uint64_t n) { return 8 * (g * n + (i - 1)); }
// the weights c_j: k field elements
inline uint64_t poly_lagr_set_weight_elems(uint64_t k) { return k; }

// 1 <= k <= POLY_LAGR_SET_MAX
inline bool poly_lagr_set_points_ok(uint64_t k) { return k >= 1 && k <= POLY_LAGR_SET_MAX; }
// ... and n >= 1 and k * n below 2^32, the limit of phase 1
inline bool poly_lagr_set_size_ok(uint64_t n, uint64_t k) { return poly_lagr_set_points_ok(k) && poly_lagr_total_ok(n, k); }
// the quotient is identically zero: no fold
inline bool poly_lagr_set_zero(uint64_t n, uint64_t k) { return k >= n; }

}  // namespace ps
