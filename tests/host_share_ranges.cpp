// host_share_ranges.cpp -- the index arithmetic of the range-sharded provers, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/share_ranges.hpp says which range of an array a rank takes (shard_range_c) and which pieces of a sum
// (share_pieces: its range of every segment, and on the last rank the fixed entries behind the last segment).  For every
// len in 0..70 and world in 1..9:
//   * the ranks' ranges partition [0, len) in order, and their counts differ by at most one;
//   * share_pieces over one, two and three segments (zero-length ones included) with 0..3 fixed entries: every entry of
//     the sum is in exactly one piece of exactly one rank -- a segment's entry in a piece of the rank whose range of that
//     segment holds it, a fixed entry in a piece of the last rank --, a rank's pieces are non-empty and ascending, and the
//     fixed tail is merged into the piece it continues.
// Prints the table "len world rank first cnt" for tests/test_share_ranges_host.py to compare with playsnark_amd.dist.shard_range.
#include <cstdio>
#include <vector>

#ifndef SHARE_RANGES_HEADER
#define SHARE_RANGES_HEADER "../playsnark_amd/csrc/share_ranges.hpp"
#endif
#include SHARE_RANGES_HEADER

static int failures = 0;
#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (failures++ < 20) {                                                   \
                std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                                   \
                std::fprintf(stderr, "\n");                                          \
            }                                                                        \
        }                                                                            \
    } while (0)

static void check_ranges(size_t len, int world) {
    size_t next = 0, lo = len, hi = 0;
    for (int rank = 0; rank < world; rank++) {
        size_t first = ~(size_t)0, cnt = ~(size_t)0;
        shard_range_c(len, rank, world, &first, &cnt);
        std::printf("%zu %d %d %zu %zu\n", len, world, rank, first, cnt);
        CHECK(first == next, "len %zu world %d rank %d: first %zu, want %zu", len, world, rank, first, next);
        CHECK(cnt <= len - next, "len %zu world %d rank %d: cnt %zu runs past the end", len, world, rank, cnt);
        next = first + cnt;
        lo = cnt < lo ? cnt : lo;
        hi = cnt > hi ? cnt : hi;
    }
    CHECK(next == len, "len %zu world %d: the ranges end at %zu", len, world, next);
    CHECK(hi - lo <= 1, "len %zu world %d: counts from %zu to %zu", len, world, lo, hi);
}

static void check_pieces(const std::vector<size_t>& lens, size_t fixed, int world) {
    std::vector<SumSegment> segs;
    size_t total = 0;
    for (size_t l : lens) { segs.push_back({total, l}); total += l; }
    total += fixed;
    // who must take each entry: the rank whose shard_range_c of the entry's segment holds it; the last rank for the fixed tail
    std::vector<int> want(total, world - 1), got(total, -1);
    for (const SumSegment& sg : segs)
        for (int rank = 0; rank < world; rank++) {
            size_t first, cnt;
            shard_range_c(sg.len, rank, world, &first, &cnt);
            for (size_t i = 0; i < cnt; i++) want[sg.off + first + i] = rank;
        }
    for (int rank = 0; rank < world; rank++) {
        const std::vector<SumSegment> pieces = share_pieces(segs, total, fixed, rank, world);
        if (world == 1) CHECK(pieces.size() == 1 && pieces[0].off == 0 && pieces[0].len == total, "one rank takes the sum whole (total %zu)", total);
        size_t end = 0;
        for (size_t k = 0; k < pieces.size(); k++) {
            const SumSegment& pc = pieces[k];
            CHECK(pc.len > 0 || world == 1, "total %zu fixed %zu world %d rank %d: empty piece %zu", total, fixed, world, rank, k);
            CHECK(pc.off >= end && pc.off <= total && pc.len <= total - pc.off, "total %zu fixed %zu world %d rank %d: piece %zu [%zu, +%zu) out of order or range",
                  total, fixed, world, rank, k, pc.off, pc.len);
            if (pc.off > total || pc.len > total - pc.off) continue;
            // the fixed tail rides in the piece it continues: it never starts a piece of its own right behind one
            CHECK(!(k > 0 && fixed && pc.off == total - fixed && pc.off == end), "total %zu fixed %zu world %d rank %d: the fixed tail is not merged", total,
                  fixed, world, rank);
            for (size_t i = pc.off; i < pc.off + pc.len; i++) {
                CHECK(got[i] == -1, "total %zu fixed %zu world %d: entry %zu is in two pieces (ranks %d and %d)", total, fixed, world, i, got[i], rank);
                got[i] = rank;
            }
            end = pc.off + pc.len;
        }
    }
    for (size_t i = 0; i < total; i++)
        CHECK(got[i] == want[i], "total %zu fixed %zu world %d: entry %zu is rank %d's, want rank %d's", total, fixed, world, i, got[i], want[i]);
}

int main() {
    for (size_t len = 0; len <= 70; len++)
        for (int world = 1; world <= 9; world++) {
            check_ranges(len, world);
            const size_t len2 = (7 * len + 3) % 23, len3 = (5 * len + 1) % 11;  // other lengths, 0 among them
            for (size_t fixed = 0; fixed <= 3; fixed++) {
                check_pieces({len}, fixed, world);
                check_pieces({len, len2}, fixed, world);
                check_pieces({len2, len}, fixed, world);
                check_pieces({len, 0}, fixed, world);
                check_pieces({len, len2, len3}, fixed, world);
                check_pieces({len3, 0, len}, fixed, world);
                check_pieces({0, len, 0}, fixed, world);
            }
        }
    if (failures) {
        std::fprintf(stderr, "host_share_ranges: %d failures\n", failures);
        return 1;
    }
    std::printf("host_share_ranges ok\n");
    return 0;
}
