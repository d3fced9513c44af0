// Index arithmetic of the polynomial scan (poly_scan.hpp): tiles, chunks of tiles, the exponent every carry is multiplied by,
// buffer sizes and the size limit.  Nothing of HIP in here: tests/host_poly_scan_plan.cpp compiles it for the host under
// ASan + UBSan and sweeps it against a literal loop.
//
// The recurrence h_n = 0, h_i = p_i + z h_{i+1} over the n coefficients p_0 .. p_{n-1} of one polynomial and one point z:
// h_0 = p(z), and q_{i-1} = h_i, 1 <= i < n, is the quotient (p(X) - p(z)) / (X - z), lowest degree first.
//   tile b      the coefficients [b T, min(n, (b + 1) T)), T = 256 threads x POLY_SCAN_ITEMS; the last tile may be partial
//   H_b         the tile's total sum_i p_i z^(i - b T) over its own coefficients
//   carry_b     h at the first index behind tile b: carry_b = H_{b+1} + z^T carry_{b+1}, 0 behind the last tile
//   h_i         local_i + z^(end_b - i) carry_b for i in tile b, local_i the suffix sum inside the tile, end_b = (b + 1) T
// A thread owns POLY_SCAN_ITEMS consecutive coefficients, so every multiplier of the scans is z^(I 2^s) (threads of a tile)
// or z^(T 2^s) (tiles of a chunk): entries of the table {z^(2^k)} with k = log2(I) + s and log2(T) + s, s < 8.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

constexpr int POLY_SCAN_THREADS = 256;
constexpr int POLY_SCAN_LOG_ITEMS = 3;
constexpr int POLY_SCAN_ITEMS = 1 << POLY_SCAN_LOG_ITEMS;                 // I: coefficients per thread
constexpr int POLY_SCAN_LOG_TILE = 8 + POLY_SCAN_LOG_ITEMS;
constexpr int POLY_SCAN_TILE = POLY_SCAN_THREADS * POLY_SCAN_ITEMS;       // T
constexpr int POLY_SCAN_CHUNK = 256;                                      // tiles the carry walk scans at once
constexpr int POLY_SCAN_POWERS = POLY_SCAN_LOG_TILE + 8;                  // table entries z^(2^k) the kernels read: k < 19
constexpr uint64_t POLY_SCAN_MAX_TOTAL = 1ull << 32;                      // k * n must stay below this
static_assert(POLY_SCAN_THREADS == 256 && POLY_SCAN_CHUNK == 256, "both scans run eight doubling steps over 256 values");
static_assert(POLY_SCAN_POWERS <= 32, "the table has 32 entries");

// tiles of a polynomial of n coefficients (n >= 1)
inline uint64_t poly_scan_tiles(uint64_t n) { return (n + POLY_SCAN_TILE - 1) / POLY_SCAN_TILE; }
// coefficients of tile b
inline uint64_t poly_scan_tile_len(uint64_t n, uint64_t b) {
    const uint64_t start = b * POLY_SCAN_TILE;
    return n - start < (uint64_t)POLY_SCAN_TILE ? n - start : (uint64_t)POLY_SCAN_TILE;
}
inline uint64_t poly_scan_last_tile_len(uint64_t n) { return poly_scan_tile_len(n, poly_scan_tiles(n) - 1); }
// chunks of the carry walk, and the tiles of chunk c (the walk starts at the LAST chunk)
inline uint64_t poly_scan_chunks(uint64_t tiles) { return (tiles + POLY_SCAN_CHUNK - 1) / POLY_SCAN_CHUNK; }
inline uint64_t poly_scan_chunk_len(uint64_t tiles, uint64_t c) {
    const uint64_t start = c * POLY_SCAN_CHUNK;
    return tiles - start < (uint64_t)POLY_SCAN_CHUNK ? tiles - start : (uint64_t)POLY_SCAN_CHUNK;
}
// the exponent of z that carry_b meets at coefficient i of tile b = i / T: the distance to the tile's nominal end (the carry
// behind a partial last tile is zero, so its nominal end serves as well as n)
inline uint64_t poly_scan_carry_exponent(uint64_t i) { return (i / POLY_SCAN_TILE + 1) * POLY_SCAN_TILE - i; }
// index into {z^(2^k)} of the multiplier of doubling step s (s < 8): threads of a tile, tiles of a chunk
inline int poly_scan_thread_power(int s) { return POLY_SCAN_LOG_ITEMS + s; }
inline int poly_scan_tile_power(int s) { return POLY_SCAN_LOG_TILE + s; }

// k polynomials' worth of work in one call: false when k * n reaches 2^32 (or overflows)
inline bool poly_scan_total_ok(uint64_t n, uint64_t k) {
    if (n == 0 || k == 0) return true;
    return k <= (POLY_SCAN_MAX_TOTAL - 1) / n;
}
// elements of the buffers: tile totals and carries (k rows of `tiles` field elements each), the quotient rows (k rows of
// n - 1 scalars of 8 words) and the values (k scalars of 8 words)
inline uint64_t poly_scan_total_elems(uint64_t n, uint64_t k) { return k * poly_scan_tiles(n); }
inline uint64_t poly_scan_quotient_words(uint64_t n, uint64_t k) { return 8 * k * (n - 1); }
inline uint64_t poly_scan_value_words(uint64_t k) { return 8 * k; }
// points of one launch (blockIdx.y): a grid's second dimension holds at most 65 535 blocks
constexpr uint64_t POLY_SCAN_MAX_POINTS_PER_LAUNCH = 65535;

}  // namespace ps
