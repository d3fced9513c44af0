// How wide an R1CS coefficient is, as the column sums over points see it (ec_spmv.hpp).  A canonical value v < r enters
// a sum as a signed magnitude: v itself while v <= (r - 1) / 2, else r - v with the point negated.  An entry is NARROW when
// that magnitude is below 2^64 -- every value that came from an int64 is, 2^63 included -- and WIDE otherwise.  Narrow
// matrices take the 64-plane kernels, matrices with a wide entry the four-word ones.
//
// No HIP in here: ps_qap_create_fr counts the wide entries on the host with these functions, k_colsum_coef_wide classifies
// with them on the device, and tests/host_coef_width.cpp compiles them for the host alone.
#pragma once
#include <stdint.h>

#include "bls12_381_constants.h"

#ifndef PS_HD
#define PS_HD
#endif

namespace ps {

// r as eight 32-bit words, least significant first
PS_HD inline uint32_t coef_r_word(int i) {
    constexpr uint32_t r[8] = PS_FR_MOD;
    return r[i];
}

// Is the 32-byte big-endian value below r (a canonical encoding)?
inline bool coef_be32_is_canonical(const uint8_t* be) {
    for (int i = 7; i >= 0; i--) {
        const uint8_t* p = be + 4 * (7 - i);
        const uint32_t w = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
        if (w != coef_r_word(i)) return w < coef_r_word(i);
    }
    return false;  // r itself
}

// v: a canonical value (v < r), eight 32-bit words, least significant first.  Writes min(v, r - v) to mag and returns the
// sign: true when the magnitude is r - v, that is when v >= (r + 1) / 2.  mag may not alias v.
PS_HD inline bool coef_signed_magnitude(uint32_t mag[8], const uint32_t v[8]) {
    uint32_t d[8];  // r - v, in 1 .. r
    uint64_t borrow = 0;
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)coef_r_word(i) - v[i] - borrow;
        d[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
    bool neg = false;  // r - v < v ?
    for (int i = 7; i >= 0; i--)
        if (d[i] != v[i]) { neg = d[i] < v[i]; break; }
    for (int i = 0; i < 8; i++) mag[i] = neg ? d[i] : v[i];
    return neg;
}

// the number of 64-bit words the magnitude needs: 0 (zero) .. 4
PS_HD inline int coef_words64(const uint32_t mag[8]) {
    for (int k = 3; k >= 0; k--)
        if (mag[2 * k] | mag[2 * k + 1]) return k + 1;
    return 0;
}

PS_HD inline bool coef_is_wide(const uint32_t mag[8]) { return coef_words64(mag) > 1; }

}  // namespace ps
