// C++ host mirror of the reference's Go surface for the prover hot path, header-only over the C
// ABI (include/playsnark_hip.h).  The reference is compiled code (Go) whose toolchain is absent
// from the build image, so this is the host side "in the reference's shape": same names,
// argument meaning and error behaviour as algebra.go / qap.go / groth16.go / pinochio.go.
//
//   playsnark::Poly::BlindEval(points)          algebra.go:348-359
//   playsnark::Poly::Mul(p2)                    algebra.go:92-105
//   playsnark::QAP::Quotient(sol)               qap.go:151-162   (throws Apocalypse)
//   playsnark::Groth16Prove(tr, q, sol, r, s)   groth16.go:122-211
//   playsnark::PHGR13Prove(ek, qap, solution)   pinochio.go:207-254
//
// The reference panics; here the same conditions throw LengthMismatch (message of
// algebra.go:351) and Apocalypse ("apocalypse", qap.go:159).  No arithmetic in this file.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/playsnark_hip.h"

namespace playsnark {

struct LengthMismatch : std::runtime_error { using std::runtime_error::runtime_error; };
struct Apocalypse : std::runtime_error { Apocalypse() : std::runtime_error("apocalypse") {} };
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc) {
    if (rc == PS_OK) return;
    if (rc == PS_ERR_LENGTH) throw LengthMismatch(ps_last_error());
    if (rc == PS_ERR_NOT_DIVISIBLE) throw Apocalypse();
    throw Error(rc, ps_last_error());
}

using Bytes = std::vector<uint8_t>;
using Scalar = std::array<uint8_t, 32>;  // Element: 32-byte big-endian

class Context {
  public:
    explicit Context(int device = 0) { check(ps_ctx_create(device, &h_)); }
    ~Context() { ps_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ps_ctx* get() const { return h_; }
    void sync() { check(ps_ctx_sync(h_)); }

  private:
    ps_ctx* h_ = nullptr;
};

// []G1 / []G2 resident on the device (Groth16Setup.Xi, PHGR13EvalKey.vs, ...)
class Points {
  public:
    Points(Context& c, int group, const Bytes& affine) : ctx_(&c) {
        const size_t wb = group == PS_G1 ? 96 : 192;
        check(ps_points_upload(c.get(), group, affine.data(), affine.size() / wb, PS_FMT_AFFINE, &h_));
    }
    Points(Points&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    ~Points() { ps_points_free(h_); }
    Points(const Points&) = delete;
    Points& operator=(const Points&) = delete;
    const ps_points* get() const { return h_; }
    size_t size() const { return ps_points_len(h_); }
    int group() const { return ps_points_group(h_); }
    // This array read as {x^i P} (Xi, Xi2: nodes = 0; XiT, gsi: nodes = 1) -> {l_j(x) P} on the QAP's nodes, without the
    // secret point: the one-time conversion of a reference-made key (groth16.go:79-97) onto the prover's fast route.
    template <class Q>
    Points ToLagrange(const Q& qap, int nodes) const {
        ps_points* h = nullptr;
        check(ps_points_monomial_to_lagrange(ctx_->get(), qap.get(), h_, nodes, &h));
        return Points(*ctx_, h);
    }
    // Is `lagr` what ToLagrange(qap, nodes) makes of this array, without making it?  rho_be32: nrho x 32 bytes drawn after both
    // arrays are fixed, at least as many as the arrays are long (ps_points_lagrange_check)
    template <class Q>
    bool LagrangeCheck(const Q& qap, const Points& lagr, int nodes, const uint8_t* rho_be32, size_t nrho) const {
        int ok = 0;
        check(ps_points_lagrange_check(ctx_->get(), qap.get(), h_, lagr.h_, nodes, rho_be32, nrho, &ok));
        return ok != 0;
    }
    Bytes Download() const {
        Bytes out(size() * (group() == PS_G1 ? 96 : 192));
        if (!out.empty()) check(ps_points_download(ctx_->get(), h_, 0, size(), out.data()));
        return out;
    }

  private:
    friend class QAP;
    Points(Context& c, ps_points* h) : ctx_(&c), h_(h) {}
    Context* ctx_;
    ps_points* h_ = nullptr;
};

// type Poly []Element (algebra.go:89); also Vector via FromValues (Value.ToFieldElement, curve.go:17-19)
class Poly {
  public:
    Poly(Context& c, const std::vector<Scalar>& coeffs) : ctx_(&c) {
        check(ps_scalars_upload(c.get(), coeffs.empty() ? nullptr : coeffs[0].data(), coeffs.size(), &h_));
    }
    static Poly FromValues(Context& c, const std::vector<int64_t>& v) {
        ps_scalars* h = nullptr;
        check(ps_scalars_upload_i64(c.get(), v.data(), v.size(), &h));
        return Poly(c, h);
    }
    Poly(Poly&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    ~Poly() { ps_scalars_free(h_); }
    Poly(const Poly&) = delete;
    Poly& operator=(const Poly&) = delete;
    const ps_scalars* get() const { return h_; }
    size_t size() const { return ps_scalars_len(h_); }

    // func (p Poly) BlindEval(zero Commit, blindedPoint []Commit) Commit
    Bytes BlindEval(const Points& blindedPoint) const {
        Bytes out(blindedPoint.group() == PS_G1 ? 96 : 192);
        check(ps_msm(ctx_->get(), blindedPoint.get(), h_, out.data()));
        return out;
    }
    // func (p Poly) Mul(p2 Poly) Poly
    Poly Mul(const Poly& p2) const {
        ps_scalars* h = nullptr;
        check(ps_poly_mul(ctx_->get(), h_, p2.h_, &h));
        return Poly(*ctx_, h);
    }
    std::vector<Scalar> Download() const {
        std::vector<Scalar> out(size());
        if (!out.empty()) check(ps_scalars_download(ctx_->get(), h_, 0, out.size(), out[0].data()));
        return out;
    }
    // t rows of N = max size() coefficients, row j = sum_i coef[i * t + j] polys[i] (ps_scalars_lincomb); Poly.Add / Poly.Sub
    // (algebra.go:161-196) are the coefficients (1, 1) and (1, r - 1).  The result is not normalised.
    static Poly LinComb(Context& c, const std::vector<const Poly*>& polys, const std::vector<Scalar>& coef, size_t t) {
        if (polys.empty() || coef.size() != polys.size() * t) throw LengthMismatch("Poly::LinComb: polys.size() * t coefficients");
        std::vector<const ps_scalars*> hs;
        for (auto* p : polys) hs.push_back(p->get());
        ps_scalars* h = nullptr;
        check(ps_scalars_lincomb(c.get(), hs.data(), hs.size(), coef.empty() ? nullptr : coef[0].data(), t, &h));
        return Poly(c, h);
    }
    // func (p Poly) Div(p2 Poly) (algebra.go:119-137) by Z_S = prod (X - z), z in zs, at least one point and all distinct
    // (ps_poly_div_roots): the size() - zs.size() quotient coefficients, lowest degree first (none for size() <= zs.size()), the
    // values p(z), and the zs.size() coefficients of the remainder -- the interpolant of (z, p(z))
    struct RootsDivision;
    RootsDivision DivRoots(const std::vector<Scalar>& zs) const;

  private:
    friend class QAP;
    Poly(Context& c, ps_scalars* h) : ctx_(&c), h_(h) {}
    Context* ctx_;
    ps_scalars* h_ = nullptr;
};

struct Poly::RootsDivision {
    Poly q;
    std::vector<Scalar> ys, rem;
};
inline Poly::RootsDivision Poly::DivRoots(const std::vector<Scalar>& zs) const {
    const size_t k = zs.size();
    ps_scalars* h = nullptr;
    std::vector<Scalar> ys(k), rem(k);
    check(ps_poly_div_roots(ctx_->get(), h_, k ? zs[0].data() : nullptr, k, &h, k ? ys[0].data() : nullptr, k ? rem[0].data() : nullptr));
    return RootsDivision{Poly(*ctx_, h), std::move(ys), std::move(rem)};
}

// type QAP (qap.go:10-27) in sparse evaluation form on the reference's domain {1..n}
class QAP {
  public:
    struct Csr {
        std::vector<uint32_t> row_ptr, col;
        std::vector<int64_t> val;
    };
    QAP(Context& c, size_t nbVars, size_t nbIO, const Csr& left, const Csr& right, const Csr& out) : ctx_(&c) {
        ps_csr l{left.row_ptr.data(), left.col.data(), left.val.data()};
        ps_csr r{right.row_ptr.data(), right.col.data(), right.val.data()};
        ps_csr o{out.row_ptr.data(), out.col.data(), out.val.data()};
        check(ps_qap_create(c.get(), left.row_ptr.size() - 1, nbVars, nbIO, &l, &r, &o, &h_));
    }
    // The same circuit with coefficients that are field elements (ps_qap_create_fr): val holds one canonical big-endian
    // Scalar per entry.  A coefficient not below r throws (PS_ERR_ENCODING).
    struct CsrFr {
        std::vector<uint32_t> row_ptr, col;
        std::vector<Scalar> val;
    };
    QAP(Context& c, size_t nbVars, size_t nbIO, const CsrFr& left, const CsrFr& right, const CsrFr& out) : ctx_(&c) {
        static_assert(sizeof(Scalar) == 32, "a Scalar is 32 bytes, so a vector of them is the val_be32 array");
        auto bytes = [](const CsrFr& m) { return m.val.empty() ? nullptr : m.val[0].data(); };
        ps_csr_fr l{left.row_ptr.data(), left.col.data(), bytes(left)};
        ps_csr_fr r{right.row_ptr.data(), right.col.data(), bytes(right)};
        ps_csr_fr o{out.row_ptr.data(), out.col.data(), bytes(out)};
        check(ps_qap_create_fr(c.get(), left.row_ptr.size() - 1, nbVars, nbIO, &l, &r, &o, &h_));
    }
    // entries of left, right, out whose signed magnitude min(v, r - v) needs more than 64 bits (ps_qap_wide_entries)
    std::array<size_t, 3> wide_entries() const {
        std::array<size_t, 3> out{};
        check(ps_qap_wide_entries(h_, out.data()));
        return out;
    }
    ~QAP() { ps_qap_free(h_); }
    QAP(const QAP&) = delete;
    QAP& operator=(const QAP&) = delete;
    const ps_qap* get() const { return h_; }
    // func (q QAP) Quotient(sol Vector) Poly -- throws Apocalypse on a non-zero remainder
    Poly Quotient(const Poly& sol) const {
        ps_scalars* h = nullptr;
        check(ps_qap_quotient(ctx_->get(), h_, sol.get(), nullptr, nullptr, nullptr, &h));
        return Poly(*ctx_, h);
    }
    // out[i] = sum_j M[j][i] * points[j] over the variables i; M = left, right, out for which = 0, 1, 2, one point per gate
    // (ps_qap_column_sums): the per-variable sums of fullLinearPoly (groth16.go:254-264) over group elements
    Points column_sums(int which, const Points& points) const {
        ps_points* h = nullptr;
        check(ps_qap_column_sums(ctx_->get(), h_, which, points.get(), &h));
        return Points(*ctx_, h);
    }
    // The n values of (L|R|O).sol on the domain 1..n, which = 0, 1, 2: what computeAggregatePoly (qap.go:164-175) interpolates,
    // uninterpolated (ps_qap_gate_values) -- the form KZGCommitLagrange and KZGOpenLagrange take
    Poly GateValues(const Poly& sol, int which) const {
        ps_scalars* h = nullptr;
        check(ps_qap_gate_values(ctx_->get(), h_, sol.get(), which, &h));
        return Poly(*ctx_, h);
    }
    // K_m = sum_i lag_g1[i-1] / (m - i), m = 1..n: the part of the proofs of all nodes that depends on this domain and the
    // string alone (ps_kzg_all_key_lagrange); computed once, it halves the work of every KZGOpenAllLagrange
    Points KZGAllKeyLagrange(const Points& lag_g1) const {
        ps_points* h = nullptr;
        check(ps_kzg_all_key_lagrange(ctx_->get(), h_, lag_g1.get(), &h));
        return Points(*ctx_, h);
    }
    // the proofs of EVERY node of this domain, element m - 1 = [((p - v_m) / (X - m))(tau)] G1, on the device, from the n values and
    // the Lagrange-form string (ps_kzg_open_all_lagrange): KZGOpenLagrange's bytes at z = m.  all_key: KZGAllKeyLagrange(lag_g1)
    // or nullptr (computed inside the call and dropped)
    Points KZGOpenAllLagrange(const Points& lag_g1, const Poly& values, const Points* all_key = nullptr) const {
        ps_points* h = nullptr;
        check(ps_kzg_open_all_lagrange(ctx_->get(), h_, lag_g1.get(), all_key ? all_key->get() : nullptr, values.get(), &h));
        return Points(*ctx_, h);
    }
    // p(z), z in zs, for the polynomial with the given n values on this domain, with no interpolation (ps_poly_eval_lagrange)
    std::vector<Scalar> EvalLagrange(const Poly& values, const std::vector<Scalar>& zs) const {
        const size_t k = zs.size();
        std::vector<Scalar> ys(k);
        check(ps_poly_eval_lagrange(ctx_->get(), h_, values.get(), k ? zs[0].data() : nullptr, k, k ? ys[0].data() : nullptr));
        return ys;
    }
    // zs.size() rows of n scalars, row j = the VALUES on 1..n of (p - p(z_j)) / (X - z_j), and the values p(z_j)
    // (ps_poly_div_linear_lagrange)
    struct LagrangeDivision {
        Poly rows;
        std::vector<Scalar> ys;
    };
    LagrangeDivision DivLinearLagrange(const Poly& values, const std::vector<Scalar>& zs) const {
        const size_t k = zs.size();
        ps_scalars* h = nullptr;
        std::vector<Scalar> ys(k);
        check(ps_poly_div_linear_lagrange(ctx_->get(), h_, values.get(), k ? zs[0].data() : nullptr, k, &h, k ? ys[0].data() : nullptr));
        return LagrangeDivision{Poly(*ctx_, h), std::move(ys)};
    }
    // the n VALUES on 1..n of (p - r) / prod (X - z), z in zs (all zero for zs.size() >= n), the values p(z), and -- unless
    // remainder is false -- the zs.size() coefficients of r, as Poly::DivRoots gives them (ps_poly_div_roots_lagrange); at least
    // one point, all distinct, on the domain or off it
    Poly::RootsDivision DivRootsLagrange(const Poly& values, const std::vector<Scalar>& zs, bool remainder = true) const {
        const size_t k = zs.size();
        ps_scalars* h = nullptr;
        std::vector<Scalar> ys(k), rem(remainder ? k : 0);
        check(ps_poly_div_roots_lagrange(ctx_->get(), h_, values.get(), k ? zs[0].data() : nullptr, k, &h, k ? ys[0].data() : nullptr,
                                         remainder && k ? rem[0].data() : nullptr));
        return Poly::RootsDivision{Poly(*ctx_, h), std::move(ys), std::move(rem)};
    }

  private:
    Context* ctx_;
    ps_qap* h_ = nullptr;
};

struct Groth16Proof {  // groth16.go:106-118
    Scalar R, S;
    std::array<uint8_t, 96> A;
    std::array<uint8_t, 192> B;
    std::array<uint8_t, 96> C;
};

// func Groth16Prove(tr Groth16Setup, q QAP, sol Vector) Groth16Proof; r, s drawn by the caller
inline Groth16Proof Groth16Prove(Context& c, const ps_groth16_pk& tr, const QAP& q, const Poly& sol, const Scalar& r,
                                 const Scalar& s) {
    Groth16Proof p{r, s, {}, {}, {}};
    check(ps_groth16_prove(c.get(), &tr, q.get(), sol.get(), r.data(), s.data(), p.A.data(), p.B.data(), p.C.data()));
    return p;
}

// Groth16Prove for every witness of `sols` (rs.size() solution vectors of q's variables back to back) under one Lagrange-form
// key, in one call (ps_groth16_prove_batch); proof j is byte for byte Groth16Prove of witness j with (rs[j], ss[j]).
// valid == nullptr: a witness that violates a gate throws Apocalypse; otherwise (*valid)[j] == 0 and proof j is all zero bytes
inline std::vector<Groth16Proof> Groth16ProveBatch(Context& c, const ps_groth16_pk& tr, const QAP& q, const Poly& sols,
                                                   const std::vector<Scalar>& rs, const std::vector<Scalar>& ss,
                                                   std::vector<int>* valid = nullptr) {
    const size_t k = rs.size();
    if (ss.size() != k) throw std::invalid_argument("Groth16ProveBatch: as many s as r");
    std::vector<uint8_t> r(32 * k + 1), s(32 * k + 1), A(96 * k + 1), B(192 * k + 1), C(96 * k + 1);
    for (size_t j = 0; j < k; j++) {
        std::copy(rs[j].begin(), rs[j].end(), r.begin() + 32 * j);
        std::copy(ss[j].begin(), ss[j].end(), s.begin() + 32 * j);
    }
    if (valid) valid->assign(k, 0);
    check(ps_groth16_prove_batch(c.get(), &tr, q.get(), sols.get(), k, r.data(), s.data(), A.data(), B.data(), C.data(),
                                 valid && k ? valid->data() : nullptr));
    std::vector<Groth16Proof> out(k);
    for (size_t j = 0; j < k; j++) {
        out[j].R = rs[j];
        out[j].S = ss[j];
        std::copy(A.begin() + 96 * j, A.begin() + 96 * (j + 1), out[j].A.begin());
        std::copy(B.begin() + 192 * j, B.begin() + 192 * (j + 1), out[j].B.begin());
        std::copy(C.begin() + 96 * j, C.begin() + 96 * (j + 1), out[j].C.begin());
    }
    return out;
}

// One rank's share of Groth16Prove when the sums are split over `world` GPUs; the ranks' A, B, C add up
// (ps_points_sum after an all_gather) to the proof
inline Groth16Proof Groth16ProveShard(Context& c, const ps_groth16_pk& tr, const QAP& q, const Poly& sol, const Scalar& r,
                                      const Scalar& s, int rank, int world) {
    Groth16Proof p{r, s, {}, {}, {}};
    check(ps_groth16_prove_shard(c.get(), &tr, q.get(), sol.get(), r.data(), s.data(), rank, world, p.A.data(), p.B.data(),
                                 p.C.data()));
    return p;
}

// One rank's share when the rank holds ONLY its index ranges of a Lagrange-form key (tr_local: lxi / lxi2 / lxi_t / nio_lp cut
// for (rank, world); ps_groth16_prove_local); the ranks' A, B, C add up to the proof, the last rank adds the fixed points
inline Groth16Proof Groth16ProveLocal(Context& c, const ps_groth16_pk& tr_local, const QAP& q, const Poly& sol, const Scalar& r,
                                      const Scalar& s, int rank, int world) {
    Groth16Proof p{r, s, {}, {}, {}};
    check(ps_groth16_prove_local(c.get(), &tr_local, q.get(), sol.get(), r.data(), s.data(), rank, world, p.A.data(), p.B.data(),
                                 p.C.data()));
    return p;
}

// Groth16Prove over the devices of this process, dev[d].pk holding only device d's index ranges (ps_groth16_prove_multi): with
// lxi / lxi2 / lxi_t on every device the route without coefficient vectors, with the monomial arrays alone the other one
inline Groth16Proof Groth16ProveMulti(const std::vector<ps_groth16_device>& dev, const Scalar& r, const Scalar& s) {
    Groth16Proof p{r, s, {}, {}, {}};
    check(ps_groth16_prove_multi(dev.data(), dev.size(), r.data(), s.data(), p.A.data(), p.B.data(), p.C.data()));
    return p;
}

// func PHGR13Prove(ek PHGR13EvalKey, qap QAP, solution Vector) PHGR13Proof
inline ps_phgr13_proof PHGR13Prove(Context& c, const ps_phgr13_ek& ek, const QAP& qap, const Poly& solution) {
    ps_phgr13_proof out;
    check(ps_phgr13_prove(c.get(), &ek, qap.get(), solution.get(), &out));
    return out;
}

// PHGR13Prove for each of the k witnesses of `sols` (k solution vectors of qap's variables back to back) under one evaluation key
// that carries lgsi, in one call (ps_phgr13_prove_batch); proof j is byte for byte PHGR13Prove of witness j.
// valid == nullptr: a witness that violates a gate throws Apocalypse; otherwise (*valid)[j] == 0 and proof j is all zero bytes
inline std::vector<ps_phgr13_proof> PHGR13ProveBatch(Context& c, const ps_phgr13_ek& ek, const QAP& qap, const Poly& sols, size_t k,
                                                     std::vector<int>* valid = nullptr) {
    std::vector<ps_phgr13_proof> out(k + 1);
    if (valid) valid->assign(k, 0);
    check(ps_phgr13_prove_batch(c.get(), &ek, qap.get(), sols.get(), k, out.data(), valid && k ? valid->data() : nullptr));
    out.resize(k);
    return out;
}

// One rank's share of PHGR13Prove over the whole key; the ranks' eight elements add up (ps_points_sum) to the proof
inline ps_phgr13_proof PHGR13ProveShard(Context& c, const ps_phgr13_ek& ek, const QAP& qap, const Poly& solution, int rank,
                                        int world) {
    ps_phgr13_proof out;
    check(ps_phgr13_prove_shard(c.get(), &ek, qap.get(), solution.get(), rank, world, &out));
    return out;
}

// PHGR13Prove over the devices of this process, dev[d].ek holding only device d's index ranges (ps_phgr13_prove_multi)
inline ps_phgr13_proof PHGR13ProveMulti(const std::vector<ps_phgr13_device>& dev) {
    ps_phgr13_proof out;
    check(ps_phgr13_prove_multi(dev.data(), dev.size(), &out));
    return out;
}

// func Groth16Verify(tr Groth16Setup, q QAP, p Groth16Proof, io Vector) bool (groth16.go:214)
inline bool Groth16Verify(Context& c, const ps_groth16_vk& vk, const Groth16Proof& p, const Poly& io) {
    int ok = 0;
    check(ps_groth16_verify(c.get(), &vk, io.get(), p.A.data(), p.B.data(), p.C.data(), &ok));
    return ok != 0;
}
// prod_i e(g1[i], g2[i]) == 1, Miller loops and their product on the device (check: subgroup tests first)
inline bool pairing_product_is_one(Context& c, const ps_points* g1, const ps_points* g2, bool check_subgroup = true) {
    int one = 0;
    check(ps_pairing_product_is_one(c.get(), g1, g2, check_subgroup ? 1 : 0, &one));
    return one != 0;
}
// Groth16Verify for nproofs proofs under one key by a random linear combination: proofs = nproofs x (A || B || C), io =
// nproofs x diff scalars (proof-major), rho_be32 = nproofs x 32 bytes drawn after the proofs are fixed
inline bool Groth16VerifyBatch(Context& c, const ps_groth16_vk& vk, const Poly& io, const uint8_t* proofs, size_t nproofs,
                               const uint8_t* rho_be32) {
    int ok = 0;
    check(ps_groth16_verify_batch(c.get(), &vk, io.get(), proofs, nproofs, rho_be32, &ok));
    return ok != 0;
}
// The invalid proofs of a batch, by bisection over partial results kept on the device (ps_groth16_verify_batch_locate):
// their indices in ascending order, empty for an accepted batch; *info (optional): checks, depth, count of the call
inline std::vector<size_t> Groth16VerifyBatchLocate(Context& c, const ps_groth16_vk& vk, const Poly& io, const uint8_t* proofs, size_t nproofs,
                                                    const uint8_t* rho_be32, ps_verify_locate_info* info = nullptr) {
    std::vector<uint8_t> valid(nproofs ? nproofs : 1, 1);
    size_t ninvalid = 0;
    check(ps_groth16_verify_batch_locate(c.get(), &vk, io.get(), proofs, nproofs, rho_be32, valid.data(), &ninvalid));
    if (info) check(ps_groth16_verify_batch_locate_info(c.get(), info));
    std::vector<size_t> bad;
    for (size_t i = 0; i < nproofs; i++)
        if (!valid[i]) bad.push_back(i);
    return bad;
}
// func PHGR13Verify(vk PHGR13VerifKey, qap QAP, p PHGR13Proof, io Vector) bool (pinochio.go:281)
inline bool PHGR13Verify(Context& c, const ps_phgr13_vk& vk, const ps_phgr13_proof& p, const Poly& io) {
    int ok = 0;
    check(ps_phgr13_verify(c.get(), &vk, io.get(), &p, &ok));
    return ok != 0;
}
// PHGR13Verify for proofs.size() proofs under one key (ps_phgr13_verify_batch): the five pairing products of the single
// verifier, each weighted by rho and each checked on its own.  io = proofs.size() x diff scalars (proof-major), rho_be32 =
// proofs.size() x 32 bytes drawn after the proofs are fixed.  *info (optional): which equations failed, device Miller loops
inline bool PHGR13VerifyBatch(Context& c, const ps_phgr13_vk& vk, const Poly& io, const std::vector<ps_phgr13_proof>& proofs,
                              const uint8_t* rho_be32, ps_phgr13_batch_info* info = nullptr) {
    int ok = 0;
    check(ps_phgr13_verify_batch(c.get(), &vk, io.get(), proofs.data(), proofs.size(), rho_be32, &ok));
    if (info) check(ps_phgr13_verify_batch_info(c.get(), info));
    return ok != 0;
}
// The invalid proofs of a PHGR13 batch, by bisection over partial results kept on the device (ps_phgr13_verify_batch_locate):
// their indices in ascending order, empty for an accepted batch.  *masks (optional): per proof the equations it violates
// (bit c = E_c, 0 for a valid proof); *info (optional): checks, products, depth, count and the batch's mask
inline std::vector<size_t> PHGR13VerifyBatchLocate(Context& c, const ps_phgr13_vk& vk, const Poly& io, const std::vector<ps_phgr13_proof>& proofs,
                                                   const uint8_t* rho_be32, std::vector<uint8_t>* masks = nullptr, ps_phgr13_locate_info* info = nullptr) {
    const size_t n = proofs.size();
    std::vector<uint8_t> valid(n ? n : 1, 1), failed(n ? n : 1, 0);
    size_t ninvalid = 0;
    check(ps_phgr13_verify_batch_locate(c.get(), &vk, io.get(), proofs.data(), n, rho_be32, valid.data(), failed.data(), &ninvalid));
    if (info) check(ps_phgr13_verify_batch_locate_info(c.get(), info));
    std::vector<size_t> bad;
    for (size_t i = 0; i < n; i++)
        if (!valid[i]) bad.push_back(i);
    if (masks) masks->assign(failed.begin(), failed.begin() + n);
    return bad;
}
// func NewGroth16TrustedSetup(qap QAP) Groth16Setup (groth16.go:64), toxic waste drawn by the caller
inline ps_groth16_crs NewGroth16TrustedSetup(Context& c, const QAP& q, const ps_groth16_toxic& tw) {
    ps_groth16_crs out;
    check(ps_groth16_setup(c.get(), q.get(), &tw, &out));
    return out;
}

// Phase-1 output (a powers-of-tau string): x^i G1 (2n-1), x^i G2 (n), alpha x^i G1 (n), beta x^i G1 (n), beta G2
using Groth16SRS = ps_groth16_srs;
// The key of NewGroth16TrustedSetup (groth16.go:64-101) for delta = gamma = 1 from the string alone: no toxic waste.  The
// caller frees the eight arrays of the result with ps_points_free, as with NewGroth16TrustedSetup.
inline ps_groth16_crs NewGroth16SetupFromSRS(Context& c, const QAP& q, const Groth16SRS& srs) {
    ps_groth16_crs out;
    check(ps_groth16_setup_from_srs(c.get(), q.get(), &srs, &out));
    return out;
}
// `in` with delta multiplied by d and gamma by g (ps_groth16_crs_contribute); xi, xi2, lxi, lxi2 of the result are views of
// in's storage (reference counted): both keys are freed array by array, in either order
inline ps_groth16_crs Groth16Contribute(Context& c, const ps_groth16_crs& in, const Scalar& d, const Scalar& g) {
    ps_groth16_crs out;
    check(ps_groth16_crs_contribute(c.get(), &in, d.data(), g.data(), &out));
    return out;
}
// Was `after` made from `before` by folding in SOME shares?  rho_be32: nrho x 32 bytes drawn after both keys are fixed, at
// least as many as the longest of nio_lp, xi_t, io_lp (ps_groth16_crs_check_update)
inline bool Groth16CheckUpdate(Context& c, const ps_groth16_crs& before, const ps_groth16_crs& after, const uint8_t* rho_be32,
                               size_t nrho) {
    int ok = 0;
    check(ps_groth16_crs_check_update(c.get(), &before, &after, rho_be32, nrho, &ok));
    return ok != 0;
}
// Is `key` what NewGroth16SetupFromSRS(q, srs) makes, with SOME shares folded in -- without deriving it again?  rho_be32: nrho x
// 32 bytes drawn after string and key are fixed, at least max(n_vars, n_gates) of them (ps_groth16_crs_check_from_srs)
inline bool Groth16CheckFromSRS(Context& c, const QAP& q, const Groth16SRS& srs, const ps_groth16_crs& key, const uint8_t* rho_be32,
                                size_t nrho, bool check_subgroup = true) {
    int ok = 0;
    check(ps_groth16_crs_check_from_srs(c.get(), q.get(), &srs, &key, rho_be32, nrho, check_subgroup ? 1 : 0, &ok));
    return ok != 0;
}

// Phase 1, the making of the string itself.  [c, c s, .., c s^(n-1)] on the device (ps_scalars_powers); the caller frees it
// with ps_scalars_free
inline ps_scalars* Powers(Context& c, const Scalar& s, size_t n, const Scalar& coeff) {
    ps_scalars* out = nullptr;
    check(ps_scalars_powers(c.get(), s.data(), coeff.data(), n, &out));
    return out;
}
using Groth16SRSShare = ps_groth16_srs_share;  // a contributor's public values: t G2, a G2, b G2
// `in` with tau multiplied by t, alpha by a, beta by b (ps_groth16_srs_contribute), and the public share.  The caller frees the
// four arrays of the result with ps_points_free; t, a, b are its to draw and to delete.
inline Groth16SRS Groth16SRSContribute(Context& c, const Groth16SRS& in, const Scalar& t, const Scalar& a, const Scalar& b,
                                       Groth16SRSShare* share) {
    Groth16SRS out;
    check(ps_groth16_srs_contribute(c.get(), &in, t.data(), a.data(), b.data(), &out, share));
    return out;
}
// Is the string well formed?  rho_be32: nrho x 32 bytes drawn after the string is fixed, at least (longest array - 1) of them
// (ps_groth16_srs_check)
inline bool Groth16SRSCheck(Context& c, const Groth16SRS& srs, const uint8_t* rho_be32, size_t nrho, bool check_subgroup = true) {
    int ok = 0;
    check(ps_groth16_srs_check(c.get(), &srs, rho_be32, nrho, check_subgroup ? 1 : 0, &ok));
    return ok != 0;
}
// Is `after` well formed and `before` with the (t, a, b) behind `share` folded in (ps_groth16_srs_check_update)?
inline bool Groth16SRSCheckUpdate(Context& c, const Groth16SRS& before, const Groth16SRS& after, const Groth16SRSShare& share,
                                  const uint8_t* rho_be32, size_t nrho) {
    int ok = 0;
    check(ps_groth16_srs_check_update(c.get(), &before, &after, &share, rho_be32, nrho, &ok));
    return ok != 0;
}

// func NewPHGR13TrustedSetup(qap QAP) PHGR13Setup (pinochio.go:93), toxic waste drawn by the caller;
// release the arrays with ps_phgr13_crs_free
inline ps_phgr13_crs NewPHGR13TrustedSetup(Context& c, const QAP& q, const ps_phgr13_toxic& tw) {
    ps_phgr13_crs out;
    check(ps_phgr13_setup(c.get(), q.get(), &tw, &out));
    return out;
}
// computeSolCommit for several evaluation-key arrays at once (pinochio.go:222-241): one digit sort
inline std::vector<Bytes> SolCommits(Context& c, const std::vector<const Points*>& arrays, const Poly& sol) {
    std::vector<const ps_points*> pts;
    std::vector<Bytes> out;
    std::vector<uint8_t*> dst;
    for (auto* a : arrays) {
        pts.push_back(a->get());
        out.emplace_back(a->group() == PS_G1 ? 96 : 192);
    }
    for (auto& o : out) dst.push_back(o.data());
    check(ps_msm_multi(c.get(), pts.data(), pts.size(), sol.get(), dst.data()));
    return out;
}

// k scalar vectors (back to back in `scalars`) over ONE point array, as one bucket problem on the device (ps_msm_batch): the dual
// of SolCommits.  out[j] = the sum of member j, 96 / 192 bytes
inline std::vector<Bytes> BlindEvalBatch(Context& c, const Points& points, const Poly& scalars, size_t k) {
    const size_t wb = points.group() == PS_G1 ? 96 : 192;
    std::vector<uint8_t> flat(wb * k + 1);
    check(ps_msm_batch(c.get(), points.get(), scalars.get(), k, flat.data()));
    std::vector<Bytes> out;
    for (size_t j = 0; j < k; j++) out.emplace_back(flat.begin() + wb * j, flat.begin() + wb * (j + 1));
    return out;
}
// k scalar vectors over several point arrays (ps_msm_batch_multi): member j is scalars[j * stride + first, + n), n the arrays'
// common length -- computeSolCommit (pinochio.go:222-241) for k solutions back to back with stride = the number of variables
// and first = diff.  One digit sort per pass serves every array.  out[i][j] = the sum of member j over arrays[i]
inline std::vector<std::vector<Bytes>> SolCommitsBatch(Context& c, const std::vector<const Points*>& arrays, const Poly& scalars, size_t k,
                                                       size_t stride, size_t first = 0) {
    std::vector<const ps_points*> pts;
    std::vector<std::vector<uint8_t>> flat;
    std::vector<uint8_t*> dst;
    for (auto* a : arrays) {
        pts.push_back(a->get());
        flat.emplace_back((a->group() == PS_G1 ? 96 : 192) * k + 1);
    }
    for (auto& f : flat) dst.push_back(f.data());
    check(ps_msm_batch_multi(c.get(), pts.data(), pts.size(), scalars.get(), k, stride, first, dst.data()));
    std::vector<std::vector<Bytes>> out(arrays.size());
    for (size_t i = 0; i < arrays.size(); i++) {
        const size_t wb = arrays[i]->group() == PS_G1 ? 96 : 192;
        for (size_t j = 0; j < k; j++) out[i].emplace_back(flat[i].begin() + wb * j, flat[i].begin() + wb * (j + 1));
    }
    return out;
}
// polys.size() polynomials opened at zs.size() points with ONE proof per point (ps_kzg_open_multi): coef[i * t + j] != 0 means
// "polynomial i is opened at point j, with this weight" (powers of a challenge drawn after commitments and values are fixed).
// ys[i * t + j] = p_i(z_j) there, zero elsewhere; proofs[j]: 96 bytes
struct KZGMultiOpening {
    std::vector<Scalar> ys;
    std::vector<Bytes> proofs;
};
inline KZGMultiOpening KZGOpenMulti(Context& c, const Points& tau_g1, const std::vector<const Poly*>& polys, const std::vector<Scalar>& zs,
                                    const std::vector<Scalar>& coef) {
    const size_t m = polys.size(), t = zs.size();
    if (m == 0 || coef.size() != m * t) throw LengthMismatch("KZGOpenMulti: polys.size() * zs.size() coefficients");
    std::vector<const ps_scalars*> hs;
    for (auto* p : polys) hs.push_back(p->get());
    KZGMultiOpening out;
    out.ys.resize(m * t);
    std::vector<uint8_t> flat(96 * t + 1);
    check(ps_kzg_open_multi(c.get(), tau_g1.get(), hs.data(), m, t ? zs[0].data() : nullptr, t, t ? coef[0].data() : nullptr,
                            t ? out.ys[0].data() : nullptr, flat.data()));
    for (size_t j = 0; j < t; j++) out.proofs.emplace_back(flat.begin() + 96 * j, flat.begin() + 96 * (j + 1));
    return out;
}
// the check of such an opening in one weighted equation (ps_kzg_verify_multi): commits m x 96 bytes, one non-zero rho per point
// drawn after everything else is fixed
inline bool KZGVerifyMulti(Context& c, const uint8_t tau_g2_1[192], const Bytes& commits, const std::vector<Scalar>& zs,
                           const std::vector<Scalar>& coef, const KZGMultiOpening& opening, const std::vector<Scalar>& rhos,
                           bool check_subgroup = true) {
    const size_t m = commits.size() / 96, t = zs.size();
    if (coef.size() != m * t || opening.ys.size() != m * t || opening.proofs.size() != t || rhos.size() != t)
        throw LengthMismatch("KZGVerifyMulti: m x t coefficients and values, one proof and one rho per point");
    Bytes proofs;
    for (auto& p : opening.proofs) proofs.insert(proofs.end(), p.begin(), p.end());
    int ok = 0;
    check(ps_kzg_verify_multi(c.get(), tau_g2_1, commits.data(), m, t ? zs[0].data() : nullptr, t, t ? coef[0].data() : nullptr,
                              t ? opening.ys[0].data() : nullptr, proofs.data(), t ? rhos[0].data() : nullptr, check_subgroup ? 1 : 0, &ok));
    return ok != 0;
}
// the values p(z), z in zs, and ONE proof [q(tau)] G1 for the whole set, q = (p - r) / prod (X - z) with r the interpolant of
// the values (ps_kzg_open_set); at least one point, all distinct
struct KZGSetOpening {
    std::vector<Scalar> ys;
    Bytes proof;
};
inline KZGSetOpening KZGOpenSet(Context& c, const Points& tau_g1, const Poly& p, const std::vector<Scalar>& zs) {
    const size_t k = zs.size();
    KZGSetOpening out;
    out.ys.resize(k);
    out.proof.resize(96);
    check(ps_kzg_open_set(c.get(), tau_g1.get(), p.get(), k ? zs[0].data() : nullptr, k, k ? out.ys[0].data() : nullptr, out.proof.data()));
    return out;
}
// e(C - [r(tau)] G1, G2) e(-proof, [Z_S(tau)] G2) == 1 (ps_kzg_verify_set): tau_g1 holds at least zs.size() powers of the string
// and tau_g2 at least zs.size() + 1
inline bool KZGVerifySet(Context& c, const Points& tau_g1, const Points& tau_g2, const Bytes& commit, const std::vector<Scalar>& zs,
                         const KZGSetOpening& opening, bool check_subgroup = true) {
    const size_t k = zs.size();
    if (opening.ys.size() != k || commit.size() != 96 || opening.proof.size() != 96)
        throw LengthMismatch("KZGVerifySet: one value per point, a commitment and a proof of 96 bytes");
    int ok = 0;
    check(ps_kzg_verify_set(c.get(), tau_g1.get(), tau_g2.get(), commit.data(), k ? zs[0].data() : nullptr, k ? opening.ys[0].data() : nullptr, k,
                            opening.proof.data(), check_subgroup ? 1 : 0, &ok));
    return ok != 0;
}
// [p(tau)] G1 for a polynomial held as its n values on the domain, over the Lagrange form of the string on the same nodes
// (ps_kzg_commit_lagrange): the bytes of Poly.Commit for the interpolated coefficients
inline Bytes KZGCommitLagrange(Context& c, const Points& lag_g1, const Poly& values) {
    Bytes out(96);
    check(ps_kzg_commit_lagrange(c.get(), lag_g1.get(), values.get(), out.data()));
    return out;
}
// the values p(z) and the proofs [q_z(tau)] G1, z in zs, from the n values and the Lagrange-form string (ps_kzg_open_lagrange):
// no interpolation, no division; the bytes ps_kzg_open gives for the coefficients.  Points may lie on the domain.
struct KZGLagrangeOpening {
    std::vector<Scalar> ys;
    std::vector<Bytes> proofs;
};
inline KZGLagrangeOpening KZGOpenLagrange(Context& c, const QAP& qap, const Points& lag_g1, const Poly& values, const std::vector<Scalar>& zs) {
    const size_t k = zs.size();
    KZGLagrangeOpening out;
    out.ys.resize(k);
    std::vector<uint8_t> flat(96 * k + 1);
    check(ps_kzg_open_lagrange(c.get(), qap.get(), lag_g1.get(), values.get(), k ? zs[0].data() : nullptr, k, k ? out.ys[0].data() : nullptr,
                               flat.data()));
    for (size_t j = 0; j < k; j++) out.proofs.emplace_back(flat.begin() + 96 * j, flat.begin() + 96 * (j + 1));
    return out;
}
// the values p(z), z in zs, and ONE proof for the whole set from the n values and the Lagrange-form string
// (ps_kzg_open_set_lagrange): the bytes KZGOpenSet gives for the interpolated coefficients, and KZGVerifySet checks them
inline KZGSetOpening KZGOpenSetLagrange(Context& c, const QAP& qap, const Points& lag_g1, const Poly& values, const std::vector<Scalar>& zs) {
    const size_t k = zs.size();
    KZGSetOpening out;
    out.ys.resize(k);
    out.proof.resize(96);
    check(ps_kzg_open_set_lagrange(c.get(), qap.get(), lag_g1.get(), values.get(), k ? zs[0].data() : nullptr, k, k ? out.ys[0].data() : nullptr,
                                   out.proof.data()));
    return out;
}
// members per pass of BlindEvalBatch / SolCommitsBatch / the batch provers (ps_msm_batch_set_chunk); 0: automatic
inline void SetBatchChunk(Context& c, int members) { check(ps_msm_batch_set_chunk(c.get(), members)); }
// batched sums over the points' window tables (ps_msm_batch_set_table): 0 automatic, 1 never, 2 wherever the tables are usable
inline void SetBatchTable(Context& c, int mode) { check(ps_msm_batch_set_table(c.get(), mode)); }

}  // namespace playsnark
