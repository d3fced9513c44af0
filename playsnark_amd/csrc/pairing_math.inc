// Host-side BLS12-381 ate pairing: tower arithmetic, Miller loop, final exponentiation (see pairing.inc for the
// verifiers built on it).  Needs field.hpp, curve.hpp, Affine<F> and affine_is_identity<F>() in scope; included by
// pairing.inc (the library) and by tests/host_limb_check.cpp (the sanitizer build of the host arithmetic).
namespace pairing_dev {
typedef Fp Base;
typedef Fp2 Base2;
// The running twist point is carried from step to step WITHOUT passing through a multiplication
// (x' = lam^2 - 2x), so with the lazy field representation its value would double every step;
// bring it back to [0, p) each time.  Input in (-3p, 2p).
static inline Fp canon_wide(const Fp& a) {
    Fp t;
    for (int i = 0; i < FP_L; i++) t.l[i] = a.l[i] + fp_mod28(i);
    return fp_canon(t);
}
static inline Fp2 canon_wide(const Fp2& a) { return Fp2{canon_wide(a.c0), canon_wide(a.c1)}; }

// This instance is also what the batch verifier's kernels run (pairing_dev.hpp): the tower functions the projective
// miller() and f12_mul() are made of compile for the device too.  Empty on a host-only build and for the Fq instance.
// PS_MILLER_F6_CALL: the Fp6 products of the tower as out-of-line device functions (operands and results through the
// lane's private memory) instead of inlined over registers -- the A/B of k_miller_batch's layout (pairing_dev.hpp).
#ifndef PS_MILLER_F6_CALL
#define PS_MILLER_F6_CALL 0
#endif
#define PS_TOWER_HD PS_HD
#if defined(__HIP_DEVICE_COMPILE__) && PS_MILLER_F6_CALL
#define PS_TOWER_F6 __attribute__((noinline))
#else
#define PS_TOWER_F6
#endif
#include "pairing_body.inc"
#undef PS_TOWER_HD
#undef PS_TOWER_F6
}  // namespace pairing_dev

#if defined(PS_HOSTFIELD)
namespace pairing {
typedef Fq Base;
typedef Fq2 Base2;
static inline Fq canon_wide(const Fq& a) { return a; }  // always reduced
static inline Fq2 canon_wide(const Fq2& a) { return a; }
#define PS_TOWER_HD
#define PS_TOWER_F6
#include "pairing_body.inc"
#undef PS_TOWER_HD
#undef PS_TOWER_F6
}  // namespace pairing
#endif
