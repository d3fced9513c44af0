// Index arithmetic of the value-form (Lagrange-form) evaluation and linear quotient (poly_lagrange.hpp): tiles, the node of
// (tile, thread, item) and back, where node m of an on-domain point lies, row offsets, chunks of the walk, buffer sizes and the
// size limit.  Nothing of HIP in here: tests/host_poly_lagrange_plan.cpp compiles it for the host under ASan + UBSan and sweeps
// it against literal loops.
//
// A polynomial of degree < n is given by its n values v_1 .. v_n on the NODES 1 .. n (the QAP domain, not a subgroup); node i is
// element i - 1 of every array.
//   tile b        the nodes [b T + 1, min(n, (b + 1) T)], T = 256 threads x POLY_LAGR_ITEMS; the last tile may be partial
//   thread t      owns POLY_LAGR_ITEMS consecutive nodes of its tile: b T + t I + 1 + m, m < I
//   A_b, B_b, P_b the tile's partial sums sum w_i v_i e_i and sum w_i e_i and its partial product prod (z - i), per (point, tile)
//   row j         the n quotient values (or the n inverses e_i) of point j: elements [j n, (j + 1) n) of the output
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

constexpr int POLY_LAGR_THREADS = 256;
#ifdef PS_LAGR_LOG_ITEMS
constexpr int POLY_LAGR_LOG_ITEMS = PS_LAGR_LOG_ITEMS;                     // an A/B build (tools/kzg_lagrange_sweep.py)
#else
constexpr int POLY_LAGR_LOG_ITEMS = 3;
#endif
constexpr int POLY_LAGR_ITEMS = 1 << POLY_LAGR_LOG_ITEMS;                 // I: nodes per thread
constexpr int POLY_LAGR_TILE = POLY_LAGR_THREADS * POLY_LAGR_ITEMS;       // T_L
constexpr int POLY_LAGR_CHUNK = 256;                                      // tiles the walk folds at once: one per thread
constexpr int POLY_LAGR_REDUCE_EVERY = 32;                                // the walk reduces its sums behind every 32nd chunk
constexpr int POLY_LAGR_PARTS = 3;                                        // A_b, B_b, P_b
constexpr uint64_t POLY_LAGR_MAX_TOTAL = 1ull << 32;                      // k * n must stay below this
constexpr uint64_t POLY_LAGR_MAX_POINTS_PER_LAUNCH = 65535;               // blockIdx.y picks the point
static_assert(POLY_LAGR_ITEMS >= 2 && POLY_LAGR_ITEMS <= 16, "a thread keeps I - 1 prefix products in registers");
static_assert(POLY_LAGR_THREADS == 256 && POLY_LAGR_CHUNK == 256, "the scans run eight doubling steps over 256 values");

// tiles of n nodes (n >= 1)
inline uint64_t poly_lagr_tiles(uint64_t n) { return (n + POLY_LAGR_TILE - 1) / POLY_LAGR_TILE; }
// nodes of tile b
inline uint64_t poly_lagr_tile_len(uint64_t n, uint64_t b) {
    const uint64_t start = b * POLY_LAGR_TILE;
    return n - start < (uint64_t)POLY_LAGR_TILE ? n - start : (uint64_t)POLY_LAGR_TILE;
}
// the node (1-based) of item m of thread t of tile b; a node above n is behind the end and takes no part
constexpr uint64_t poly_lagr_node(uint64_t b, uint64_t t, uint64_t m) { return b * POLY_LAGR_TILE + t * POLY_LAGR_ITEMS + m + 1; }
// ... and back: the tile, thread and item that hold node i >= 1
inline uint64_t poly_lagr_node_tile(uint64_t i) { return (i - 1) / POLY_LAGR_TILE; }
inline uint64_t poly_lagr_node_thread(uint64_t i) { return (i - 1) % POLY_LAGR_TILE / POLY_LAGR_ITEMS; }
inline uint64_t poly_lagr_node_item(uint64_t i) { return (i - 1) % POLY_LAGR_ITEMS; }
// A point z is ON the domain when it is one of the nodes: its canonical value as eight little-endian words is in [1, n].
// Returns that node m, or 0 for a point off the domain (n < 2^32 by the size limit, so a node fits one word).
inline uint64_t poly_lagr_hit(const uint32_t* z_words8, uint64_t n) {
    for (int i = 1; i < 8; i++)
        if (z_words8[i]) return 0;
    return z_words8[0] >= 1 && z_words8[0] <= n ? z_words8[0] : 0;
}
// element (of 8 words) of node i in row j
inline uint64_t poly_lagr_row_elem(uint64_t j, uint64_t i, uint64_t n) { return j * n + (i - 1); }
// chunks of the walk over `tiles` partials, and the tiles of chunk c
constexpr uint64_t poly_lagr_chunks(uint64_t tiles) { return (tiles + POLY_LAGR_CHUNK - 1) / POLY_LAGR_CHUNK; }
inline uint64_t poly_lagr_chunk_len(uint64_t tiles, uint64_t c) {
    const uint64_t start = c * POLY_LAGR_CHUNK;
    return tiles - start < (uint64_t)POLY_LAGR_CHUNK ? tiles - start : (uint64_t)POLY_LAGR_CHUNK;
}
// the walk's sums are reduced behind chunk c (counted from 0) when this holds: never more than 32 additions between two
constexpr bool poly_lagr_reduce_after(uint64_t c) { return (c + 1) % POLY_LAGR_REDUCE_EVERY == 0; }
// blocks of the elementwise apply pass: one node per thread
inline uint64_t poly_lagr_apply_blocks(uint64_t n) { return (n + POLY_LAGR_THREADS - 1) / POLY_LAGR_THREADS; }

// k points' worth of work in one call: false when n == 0 or k * n reaches 2^32 (or overflows)
inline bool poly_lagr_total_ok(uint64_t n, uint64_t k) {
    if (n == 0) return false;
    if (k == 0) return true;
    return k <= (POLY_LAGR_MAX_TOTAL - 1) / n;
}
// elements of the buffers: the partials (three planes of k rows of `tiles` field elements; plane p starts at p * k * tiles),
// the rows (k rows of n scalars of 8 words), the values (k scalars of 8 words) and the walk's y and q_m (two per point)
inline uint64_t poly_lagr_plane_elems(uint64_t n, uint64_t k) { return k * poly_lagr_tiles(n); }
inline uint64_t poly_lagr_part_elems(uint64_t n, uint64_t k) { return POLY_LAGR_PARTS * poly_lagr_plane_elems(n, k); }
inline uint64_t poly_lagr_part_elem(uint64_t plane, uint64_t j, uint64_t b, uint64_t n, uint64_t k) {
    return plane * poly_lagr_plane_elems(n, k) + j * poly_lagr_tiles(n) + b;
}
inline uint64_t poly_lagr_row_words(uint64_t n, uint64_t k) { return 8 * k * n; }
inline uint64_t poly_lagr_value_words(uint64_t k) { return 8 * k; }
inline uint64_t poly_lagr_yq_elems(uint64_t k) { return 2 * k; }

}  // namespace ps
