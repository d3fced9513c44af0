// Index arithmetic of the linear combination of scalar vectors (fr_lincomb.hpp): row groups, grid sizes, the layout of the
// two tables the kernel reads from device memory, the output layout and the size limits.  Nothing of HIP in here:
// tests/host_fr_lincomb_plan.cpp compiles it for the host under ASan + UBSan and sweeps it against a literal loop.
//
// m inputs v_0 .. v_{m-1} of len_l scalars each, a coefficient matrix c of m x t entries (entry [l * t + j]) and t output rows
// of N = max_l len_l scalars:  out[j * N + i] = sum_l c_lj v_l[i], every v_l zero behind its end.
//   thread      one index i (blockIdx.x * 256 + threadIdx.x) of one group of FR_LINCOMB_ROWS consecutive rows (blockIdx.y)
//   group g     the rows [g R, min(t, (g + 1) R)); the last group may be partial
//   launch      at most 65 535 groups (a grid's second dimension); the first group of a launch is a kernel argument
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

constexpr int FR_LINCOMB_THREADS = 256;
constexpr int FR_LINCOMB_ROWS = 4;                                 // R: accumulators a thread keeps
constexpr int FR_LINCOMB_REDUCE_EVERY = 32;                        // inputs between two fr_reduce of the accumulators
constexpr uint64_t FR_LINCOMB_MAX_TOTAL = 1ull << 32;              // t * N must stay below this (the scan's limit on what reads the rows)
constexpr uint64_t FR_LINCOMB_MAX_ENTRIES = 1ull << 20;            // m * t at most this: one upload of the coefficient table (48 MiB)
constexpr uint64_t FR_LINCOMB_MAX_GROUPS_PER_LAUNCH = 65535;       // blockIdx.y
static_assert((FR_LINCOMB_REDUCE_EVERY & (FR_LINCOMB_REDUCE_EVERY - 1)) == 0, "the kernel tests l & (EVERY - 1)");

// The two tables in device memory, read through uniform loads.
struct FrLincombInput {  // one per input
    const uint32_t* p;   // its plain canonical words, 8 per scalar
    uint64_t n;          // its length, >= 1
};
struct FrLincombCoef {   // one per matrix entry, at [l * t + j]
    int32_t l[10];       // c_lj in Montgomery form, canonical 28-bit limbs
    uint32_t nonzero;    // 0: the entry is zero and the kernel skips the product
    uint32_t pad;
};
static_assert(sizeof(FrLincombInput) == 16 && sizeof(FrLincombCoef) == 48, "table layout");

inline uint64_t fr_lincomb_blocks(uint64_t N) { return (N + FR_LINCOMB_THREADS - 1) / FR_LINCOMB_THREADS; }
inline uint64_t fr_lincomb_groups(uint64_t t) { return (t + FR_LINCOMB_ROWS - 1) / FR_LINCOMB_ROWS; }
// rows of group g (g < fr_lincomb_groups(t))
inline uint64_t fr_lincomb_group_rows(uint64_t t, uint64_t g) {
    const uint64_t start = g * FR_LINCOMB_ROWS;
    return t - start < (uint64_t)FR_LINCOMB_ROWS ? t - start : (uint64_t)FR_LINCOMB_ROWS;
}
// launches over the groups, and the groups of launch k
inline uint64_t fr_lincomb_launches(uint64_t groups) { return (groups + FR_LINCOMB_MAX_GROUPS_PER_LAUNCH - 1) / FR_LINCOMB_MAX_GROUPS_PER_LAUNCH; }
inline uint64_t fr_lincomb_launch_groups(uint64_t groups, uint64_t k) {
    const uint64_t start = k * FR_LINCOMB_MAX_GROUPS_PER_LAUNCH;
    return groups - start < FR_LINCOMB_MAX_GROUPS_PER_LAUNCH ? groups - start : FR_LINCOMB_MAX_GROUPS_PER_LAUNCH;
}
inline uint64_t fr_lincomb_coef_index(uint64_t l, uint64_t j, uint64_t t) { return l * t + j; }
// first word of out[j * N + i]
inline uint64_t fr_lincomb_out_word(uint64_t j, uint64_t i, uint64_t N) { return 8 * (j * N + i); }
// is the accumulator reduced behind input l?
constexpr bool fr_lincomb_reduce_after(uint64_t l) { return (l & (FR_LINCOMB_REDUCE_EVERY - 1)) == (uint64_t)FR_LINCOMB_REDUCE_EVERY - 1; }

// false when t * N reaches 2^32 or m * t exceeds 2^20 (or either overflows); m, t, N >= 1
inline bool fr_lincomb_size_ok(uint64_t m, uint64_t t, uint64_t N) {
    if (m == 0 || t == 0 || N == 0) return true;
    return t <= (FR_LINCOMB_MAX_TOTAL - 1) / N && m <= FR_LINCOMB_MAX_ENTRIES / t;
}

}  // namespace ps
