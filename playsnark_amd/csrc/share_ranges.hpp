// Index arithmetic of the range-sharded provers: which part of an array, and which pieces of a sum, a rank takes.  No HIP in
// here: tests/host_share_ranges.cpp compiles it for the host alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

// Rank `rank` of `world` takes [first, first + cnt) of an array of `len`: contiguous, in order of rank, counts differ by at
// most one (the first len % world ranks have one more).  playsnark_amd.dist.shard_range is the same rule.
static inline void shard_range_c(size_t len, int rank, int world, size_t* first, size_t* cnt) {
    const size_t base = len / (size_t)world, extra = len % (size_t)world;
    *first = (size_t)rank * base + std::min<size_t>((size_t)rank, extra);
    *cnt = base + ((size_t)rank < extra ? 1 : 0);
}

struct SumSegment { size_t off, len; };

// A sum over `total` entries: the segments `segs` (each sharded over the ranks) and behind them `fixed` entries that are not.
// Returns the rank's pieces, in order: its range of every segment (empty ranges left out), and on the LAST rank the fixed
// entries.  There they continue its range of the last segment, so they ride in that piece instead of being a sum of their
// own (a 3-point sum is all latency: rank 0's share of a 2^20-constraint proof took 7.8 ms where the others took 6.5,
// tools/g16_shares.py).  One rank takes the sum whole.
static inline std::vector<SumSegment> share_pieces(const std::vector<SumSegment>& segs, size_t total, size_t fixed, int rank, int world) {
    std::vector<SumSegment> pieces;
    if (world == 1) {
        pieces.push_back({0, total});
        return pieces;
    }
    for (const SumSegment& sg : segs) {
        size_t f, cnt;
        shard_range_c(sg.len, rank, world, &f, &cnt);
        if (cnt) pieces.push_back({sg.off + f, cnt});
    }
    if (rank == world - 1 && fixed) {
        if (!pieces.empty() && pieces.back().off + pieces.back().len == total - fixed) pieces.back().len += fixed;
        else pieces.push_back({total - fixed, fixed});
    }
    return pieces;
}
