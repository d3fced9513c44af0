// Device side of ps_phgr13_verify_batch_locate (verify_phgr13_locate.inc): what the bisection of a rejected PHGR13 batch
// reads beyond the trees of locate_dev.hpp.  Included by capi.hip after locate_dev.hpp; its PS_HD part alone (which trees an
// equation reads, where a node lies; PS_LOCATE_INDEX_ONLY) by tests/host_phgr13_locate_index.cpp, which runs it on the host
// under ASan + UBSan together with the descent itself, locate_bisect of locate_descent.hpp, which both locators share;
// tests/device_phgr13_locate_check.hip includes it whole and launches k_g2_pair_sums and k_f12_segment_products directly
// (tests/test_device_phgr13_locate.py: every node against the oracle's G2 addition, every product against Python integers).
//
// The trees have the layout of locate_dev.hpp (node (l, i) covers the proofs [i 2^l, min((i + 1) 2^l, N)), all levels kept):
//   element trees  rho_i X_i in XYZZ form for the G1 elements the failed equations read, LEVEL-major: level l holds one
//                  segment of size[l] nodes per tree, side by side -- one k_g1_pair_sums launch per level for all of them
//   P trees        diff more G1 trees, leaves io_ik (rho_i gv_i), same layout
//   wss tree       rho_i wss_i in G2, one k_g2_pair_sums per level
//   F tree         miller(rho_i gv_i, wss_i): level 0 is the first N values of the batch's k_miller_batch launch, whose
//                  diff loops with the key's ws_k follow it; the levels above lie behind those (f_level_base), then the
//                  batch's product and the levels of the small product tree over the key's loops
//   scalar tree    k_fr_locate_rows, k_fr_row_pair_sums as they are
#pragma once
#include "locate_dev.hpp"

namespace ps {
namespace phgr13_locate {

constexpr int EQUATIONS = 5;
constexpr u32 ALL_EQUATIONS = (1u << EQUATIONS) - 1;
// the G1 elements in the order of the batch call's element-major upload
enum Element { VSS, VASS, WASS, YSS, YASS, HS, GZ, G1_ELEMENTS };

// Equations that read G1 element e: E0 reads hs and yss, E1 vass and vss, E2 wass (and wss), E3 yass and yss, E4 gz, vss,
// yss (and wss)
PS_HD inline u32 element_equations(int e) {
    return e == VSS ? 0b10010u : e == VASS ? 0b00010u : e == WASS ? 0b00100u : e == YSS ? 0b11001u : e == YASS ? 0b01000u : e == HS ? 0b00001u
         : e == GZ ? 0b10000u : 0u;
}
constexpr u32 WSS_EQUATIONS = 0b10100u;  // ... and the G2 element
// The G1 elements a descent under the root mask `mask` needs a tree of, in ascending order: slot[e] = the tree's segment or
// -1; returns their number
PS_HD inline int element_slots(u32 mask, int* slot) {
    int n = 0;
    for (int e = 0; e < G1_ELEMENTS; e++) slot[e] = (element_equations(e) & mask) ? n++ : -1;
    return n;
}
// First node of segment `seg` of level l of `segs` trees kept level-major (size, off: locate::tree_levels)
PS_HD inline u64 segment_node(const u64* size, const u64* off, int l, u64 segs, u64 seg) { return segs * off[l] + seg * size[l]; }
// First value of level l of the F tree over N proofs whose level 0 is followed by the `diff` loops of the key
using locate::f_level_base;
// The batch's product lies behind the levels and the key's loops, and behind it the levels of the product tree over the
// key's loops (ceil(diff / 2) values, then half of that ..: fewer than diff + MAX_LEVELS in all)
PS_HD inline u64 f_product_at(const u64* off, int levels, u64 diff) { return off[levels] + diff; }
PS_HD inline u64 f_key_levels_at(const u64* off, int levels, u64 diff) { return off[levels] + diff + 1; }
// Values of the whole F buffer
PS_HD inline u64 f_tree_values(const u64* off, int levels, u64 diff) { return off[levels] + 2 * diff + 1 + locate::MAX_LEVELS; }
// Host Miller loops of equation c of one set (the device ran the others of E0)
PS_HD inline int host_loops(int c) { return c == 4 ? 3 : 2; }

}  // namespace phgr13_locate
}  // namespace ps

#ifndef PS_LOCATE_INDEX_ONLY  // (the host check of the index arithmetic above takes it alone, without the tower)
namespace pairing_dev {
// out[s] = first[s] * prod_{j < len} in[s * len + j] (first == nullptr: the product alone; nothing to multiply: one).  The
// running product lives in out[s] and every factor is read from memory, as f12_mul_mem wants them: what f12_mul_mem stores
// is below 4 p at limb class <= 2 whatever went in at that class (f12_coeff above), so a chain of any length stays where
// the product tree stays.  out must not overlap first or in.
PS_HD static inline void f12_segment_product(Fp12* out, const Fp12* first, const Fp12* in, u32 len, u32 s) {
    const Fp12* seg = in + (size_t)s * len;
    u32 j = 0;
    if (first) out[s] = first[s];
    else if (len) out[s] = seg[j++];
    else out[s] = f12_one();
    for (; j < len; j++) {
        Fp12 t;
        f12_mul_mem(t, out[s], seg[j]);
        out[s] = t;
    }
}
}  // namespace pairing_dev
#endif

#if !defined(PS_LOCATE_INDEX_ONLY) && (defined(__HIPCC__) || defined(__HIP__))
namespace ps {

// The G2 twin of k_g1_pair_sums, same segmented contract: segment s reads n nodes at in + s * in_stride and writes
// ceil(n / 2) at out + s * out_stride; out[i] = in[2i] + in[2i + 1], or in[2i] for the carried node.  The complete addition
// of curve.hpp: identity operands, equal operands and P + (-P) are ordinary inputs.  One LANE PAIR per output node (Fp2s: the
// even lane holds c0, the odd lane c1 of every coordinate, as in every G2 kernel of the sums), so 2 * segs * ceil(n / 2)
// threads, below 2^32 (the host keeps segs * ceil(n / 2) below 2^20).  Both lanes of a pair take every branch together.
__global__ void __launch_bounds__(256, PS_TAIL_WAVES) k_g2_pair_sums(const Xyzz<Fp2>* __restrict__ in, u32 n, u32 segs, u32 in_stride,
                                                                     Xyzz<Fp2>* __restrict__ out, u32 out_stride) {
    const u32 t = logical_tid<Fp2s>(), h = (n + 1) / 2;
    if (t >= segs * h) return;
    const u32 seg = t / h, i = t - seg * h;
    const Xyzz<Fp2>* src = in + (size_t)seg * in_stride;
    Xyzz<Fp2s> acc = ld_xyzz<Fp2s>(&src[2 * i]);
    if (2 * i + 1 < n) {
        const Xyzz<Fp2s> right = ld_xyzz<Fp2s>(&src[2 * i + 1]);
        xyzz_add_inl<Fp2s>(acc, right);
    }
    st_xyzz<Fp2s>(&out[(size_t)seg * out_stride + i], acc);
}

// The Miller values of K sets reduced to one each: out[s] = first[s] * prod_{j < len} in[s * len + j], s < segs.  Lanes
// placed as k_f12_product places them (spread_index: `lpw` active lanes per wave).
__global__ void __launch_bounds__(64, 1) k_f12_segment_products(const pairing_dev::Fp12* __restrict__ first, const pairing_dev::Fp12* __restrict__ in,
                                                                u32 segs, u32 len, u32 lpw, pairing_dev::Fp12* __restrict__ out) {
    u32 s;
    if (!pairing_dev::spread_index(blockIdx.x * blockDim.x + threadIdx.x, lpw, segs, s)) return;
    pairing_dev::f12_segment_product(out, first, in, len, s);
}

}  // namespace ps
#endif
