// Pass arithmetic of ps_msm_batch: how many of the K member sums (K scalar vectors over ONE point array) run as one pass,
// i.e. as one sort, one accumulation and one tail over Kc * W bucket sets.  No HIP in here: tests/host_msm_batch_plan.cpp
// compiles it for the host alone.
//
// A pass of Kc members, each of n scalars cut into W windows of NB = 2^(c-1) buckets, must respect five limits:
//   buckets   Kc * W * NB <= max_buckets   the two-level sort (k_sort_*) handles at most SORT_MAX_BUCKETS bucket keys
//   entries   Kc * n * W  <  max_entries   entry offsets, ranks and totals are 32-bit, and an entry keeps bit 31 for its sign
//   bytes     bucket array + partial slots <= max_bytes   (Kc * W * NB buckets, two slots per slice of >= min_slice entries)
//   sets      Kc * W <= max_sets           the per-set launches of the reduction: every grid is sets x (at most NB or c + 4)
//                                          workgroups and every u32 product (segments, roles, results) is at most
//                                          sets x NB, so with the bucket limit they stay far inside 2^31; the cap bounds the
//                                          one-workgroup-per-set kernels (k_reduce_weights) and the fold's member count
//   chunk     Kc <= chunk                  ps_msm_batch_set_chunk (0: no such limit)
// The members of a batch are taken in order, full passes first: K = 5 under a limit of 2 runs passes of 2, 2 and 1.
//
// Over a window table (BatchShape::table) all W windows of a member share ONE bucket set: a member still has n * W entries,
// but NB buckets and one set, so the limits read
//   buckets   Kc * NB          entries   Kc * n * W          bytes   Kc * (NB + 2 * slices) * point_bytes
//   sets      Kc               chunk     Kc
// A five-value BatchShape{n, W, NB, point_bytes, min_slice} is the plain shape, as it always was.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct BatchShape {
    uint64_t n;            // scalars per member = points
    uint64_t W;            // windows per scalar
    uint64_t NB;           // buckets per window
    uint64_t point_bytes;  // one XYZZ point of the group (a bucket, a partial slot)
    uint64_t min_slice;    // fewest entries an accumulation slice may hold (each slice owns two partial slots)
    uint64_t table = 0;    // nonzero: the points carry a window table, a member is one bucket set of NB buckets
};
struct BatchLimits {
    uint64_t max_buckets, max_entries, max_bytes, max_sets, chunk;
};
struct BatchPass { uint64_t first, count; };

// buckets and bucket sets of ONE member
static inline uint64_t batch_member_buckets(const BatchShape& s) { return s.table ? s.NB : s.W * s.NB; }
static inline uint64_t batch_member_sets(const BatchShape& s) { return s.table ? 1 : s.W; }

// bytes of the bucket array and the partial slots of a pass of kc members (an upper bound: slices counted per member)
static inline uint64_t batch_pass_bytes(const BatchShape& s, uint64_t kc) {
    const uint64_t slices = (s.n * s.W + s.min_slice - 1) / s.min_slice;
    return kc * (batch_member_buckets(s) + 2 * slices) * s.point_bytes;
}

// The largest number of members one pass may hold; 0: not even one member fits (the caller sums member by member).
static inline uint64_t batch_pass_members(const BatchShape& s, const BatchLimits& l) {
    if (s.n == 0 || s.W == 0 || s.NB == 0 || s.min_slice == 0) return 0;
    const uint64_t gb = batch_member_buckets(s), e = s.n * s.W;
    uint64_t kc = l.max_buckets / gb;
    kc = std::min(kc, (l.max_entries - 1) / e);
    kc = std::min(kc, l.max_sets / batch_member_sets(s));
    kc = std::min(kc, l.max_bytes / batch_pass_bytes(s, 1));
    if (l.chunk) kc = std::min(kc, l.chunk);
    return kc;
}

// The passes of a batch of K members: [first, first + count) in order, a partition of 0..K.  Returns false when K > 0 and
// no pass of even one member exists (`out` is left empty); K == 0 gives true and no pass.
static inline bool batch_passes(uint64_t K, const BatchShape& s, const BatchLimits& l, std::vector<BatchPass>* out) {
    out->clear();
    if (K == 0) return true;
    const uint64_t kc = batch_pass_members(s, l);
    if (kc == 0) return false;
    for (uint64_t first = 0; first < K; first += kc) out->push_back({first, std::min(kc, K - first)});
    return true;
}
