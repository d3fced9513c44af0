// Buckets in order of size: the index arithmetic of the whole-bucket point pass (msm.hpp section 4b), kept apart from the
// kernels so that it also compiles for the host -- tests/host_bucket_order.cpp runs exactly these functions over generated
// offs[] arrays and checks that perm[] is a permutation in non-increasing size classes and that the verdict is what a direct
// computation gives.
//
// k_bucket_sum gives every bucket to ONE lane.  A wave runs as long as its largest bucket, so the lanes of a wave must hold
// buckets of (nearly) one size: a counting sort of the G bucket sizes, largest first, over BO_CLASSES size classes
// (k_bo_count: histogram; k_bo_scan: class starts and the verdict; k_bo_place: perm[pos] = g).  Sizes of BO_CLASSES - 1 and
// more share the first class: an evenly filled sum has none, and a sum that has some is not summed this way unless forced.
#pragma once
#include "field.hpp"

namespace ps {

constexpr u32 BO_CLASSES = 256;
constexpr u32 BO_PLACE_ITEMS = 4;                       // buckets per thread of k_bo_place
constexpr u32 BO_PLACE_TILE = 256 * BO_PLACE_ITEMS;     // ... and per workgroup: one cursor reservation per (tile, class)

// which point pass a sum takes (ps_msm_set_accumulate / ps_msm_last_accumulate; the verdict word holds one of the last two)
enum AccumulatePath : u32 { ACC_AUTO = 0, ACC_SLICES = 1, ACC_BUCKETS = 2 };

// The host's part of the automatic choice (tuning values: profiles/bucket_order_ab.txt).  Whole buckets can pay only for a
// long sum with enough buckets for several rounds of the chip's 2 048 wave slots, and a lane must not hold a wave slot for
// longer than BO_MAX_MEAN additions or the tails of the other sums in flight starve (the reason slices of 96 and 128 lost).
// Scalars of at most BO_SHORT_BITS bits are the int64 wire values of a circuit -- zeros, ones, small numbers: a few buckets
// hold most of the entries, the device would say "slices" anyway, and the ordering kernels are not spent on them.
constexpr u64 BO_MIN_BUCKETS = 1ull << 18;
constexpr u64 BO_MAX_MEAN = 64;
constexpr int BO_SHORT_BITS = 64;
inline bool bo_host_admits(bool shortsum, u64 G, u64 digits, int max_bits) {
    return !shortsum && max_bits > BO_SHORT_BITS && G >= BO_MIN_BUCKETS && digits <= BO_MAX_MEAN * G;
}
// ... and the device's: "even" when the largest bucket is within BO_EVEN_MULT x mean + BO_EVEN_ADD of the non-empty buckets' mean
constexpr u32 BO_EVEN_MULT = 4;
constexpr u32 BO_EVEN_ADD = 32;

PS_HD inline u32 bo_class(u32 lo, u32 hi) {
    const u32 s = hi - lo;
    return s < BO_CLASSES - 1 ? s : BO_CLASSES - 1;
}

// Exclusive scan of the class histogram in DESCENDING size: start[k] = number of buckets in classes above k.  Returns the
// largest non-empty class (0 when every bucket is empty).
PS_HD inline u32 bo_scan_desc(const u32* hist, u32* start) {
    u32 run = 0, maxc = 0;
    for (u32 k = BO_CLASSES; k-- > 0;) {
        start[k] = run;
        run += hist[k];
        if (hist[k] && k > maxc) maxc = k;
    }
    return maxc;
}

// The verdict of a sum of E entries whose largest size class is maxc, with `nonempty` non-empty buckets: whole buckets when the
// fill is even, slices otherwise (the capped first class counts as uneven: its buckets may be of any size).
PS_HD inline u32 bo_verdict(u32 maxc, u32 nonempty, u32 E) {
    if (nonempty == 0 || maxc >= BO_CLASSES - 1) return ACC_SLICES;
    return (u64)maxc * nonempty <= (u64)BO_EVEN_MULT * E + (u64)BO_EVEN_ADD * nonempty ? ACC_BUCKETS : ACC_SLICES;
}

}  // namespace ps
