// Who writes a bucket, and who reads a partial slot: the index arithmetic of the fix-up (msm.hpp section 5), kept apart from
// the kernels so that it also compiles for the host -- tests/host_fixup_ownership.cpp runs exactly these functions over
// generated offs[] arrays and checks that every bucket has one writer and every partial slot one reader.
//
// The accumulation cuts the sorted list into slices of M entries.  A bucket [lo, hi) that lies inside one slice is written by
// the accumulation itself; one that a slice boundary cuts leaves a partial sum per slice it touches (slot 2t for a run that
// starts slice t, slot 2t + 1 for one that ends it) and is written by the kernel its class names.
#pragma once
#include "field.hpp"

namespace ps {

// Slice length a sum actually uses.  The plan is made before the sort has run, for W digits per scalar; a witness of bits or
// small values leaves one digit per scalar, and 2^19 entries in slices of 32 are 256 waves on a chip that holds 2 048 (the
// accumulation of Groth16's A over 2^20 booleanity gates: 0.46-0.60 ms for 0.06 ms of work).  So every kernel that walks the
// slices derives their length from the length of the sorted list E = offs[G], the planned slice count T and the planned M:
// M again as soon as the list is a quarter of the plan, shorter below, never under 4 (or a shorter planned M).
PS_HD inline int eff_slice(u32 E, u32 T, int M) {
#if defined(PS_NO_EFF_SLICE)  // measurement builds: the planned length throughout
    return M;
#endif
    const u64 m = (4ull * E + T - 1) / (T ? T : 1u);
    const u64 lo = M < 4 ? (u64)M : 4ull;
    return m >= (u64)M ? M : (int)(m < lo ? lo : m);
}

constexpr u32 HEAVY_SPAN = 8;  // buckets cut into more slices than this go to the heavy-bucket kernels

enum BucketClass : int {
    BUCKET_EMPTY = 0,  // no entries: the classification writes the identity (the bucket array is never cleared)
    BUCKET_WHOLE = 1,  // inside one slice: the accumulation's flush wrote it
    BUCKET_PAIR = 2,   // cut once, two partial slots: the thread of that slice boundary adds them (k_fixup_pair)
    BUCKET_CHAIN = 3,  // three to heavy_span slots: chain_list, a lane quad each (k_qfixup_chain)
    BUCKET_HEAVY = 4   // more: heavy_list, two levels of quad trees (k_heavy_jobs, k_qfixup_heavy*)
};
PS_HD inline int bucket_class(u32 lo, u32 hi, u32 M, u32 heavy_span) {
    if (lo == hi) return BUCKET_EMPTY;
    const u32 span = (hi - 1) / M - lo / M;  // slice boundaries inside the bucket
    return span == 0 ? BUCKET_WHOLE : span >= heavy_span ? BUCKET_HEAVY : span == 1 ? BUCKET_PAIR : BUCKET_CHAIN;
}

// Partial slot of the part of bucket [lo, ..) that lies in slice t: the head slot when the run starts the slice
PS_HD inline size_t part_slot(u32 lo, u32 t, u32 M) { return 2 * (size_t)t + (lo > t * M ? 1 : 0); }

// The bucket cut by slice boundary t (1 <= t, position t M of a sorted list of E entries), if adding its two slots is this
// boundary's job: false past the end of the list, where the boundary falls between two buckets, and where the bucket is cut
// more than once (its class sends it to a list).  offs[0 .. G]: bucket starts, offs[G] = E.
PS_HD inline bool pair_boundary_bucket(const u32* __restrict__ offs, u32 G, u32 E, u32 t, u32 M, u32 heavy_span, u32& g) {
    const u64 pos64 = (u64)t * M;
    if (pos64 >= E) return false;
    const u32 pos = (u32)pos64;
    u32 lo = 0, hi = G;  // invariant: offs[lo] <= pos < offs[hi]
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (offs[mid] <= pos) lo = mid; else hi = mid;
    }
    g = lo;
    const u32 b0 = offs[lo], b1 = offs[lo + 1];
    if (b0 == pos) return false;  // the slice starts a bucket: nothing is cut here
    return bucket_class(b0, b1, M, heavy_span) == BUCKET_PAIR;
}

}  // namespace ps
