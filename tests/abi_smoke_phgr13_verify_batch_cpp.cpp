// abi_smoke_phgr13_verify_batch_cpp.cpp -- playsnark::PHGR13VerifyBatch of host/playsnark.hpp on the device: the 7-gate tiling
// of the toy gate pattern (9 variables, nbIO = 3, diff = 6), two witnesses (x = 3, 5) proved by PHGR13ProveBatch, verified as
// one batch (accepted: failed = 0, 2 + diff device loops), then with the gz of proof 0 replaced by that of proof 1 (rejected:
// failed = {E4}); rho = 0 throws Error(PS_ERR_ARG).
//   g++ -std=c++17 -I. tests/abi_smoke_phgr13_verify_batch_cpp.cpp -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_phgr13_verify_batch_cpp
// Exit codes: 0 = all checks passed, 77 = no gfx950 device, 1 = failure.
#include <cstdio>
#include <cstring>

#include "playsnark_amd/host/playsnark.hpp"

using namespace playsnark;

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::fprintf(stderr, "abi_smoke_phgr13_verify_batch_cpp: line %d: %s failed\n", __LINE__, #cond); \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

static Scalar small(unsigned long v) {
    Scalar s{};
    for (int i = 0; i < 8; i++) s[31 - i] = (uint8_t)(v >> (8 * i));
    return s;
}

int main() {
    if (ps_device_count() == 0) { std::printf("no gfx950 device\n"); return 77; }
    try {
        Context ctx(0);
        const size_t M = 9, NIO = 3, DIFF = M - NIO, K = 2;
        QAP::Csr L{{0, 1, 2, 4, 6, 7, 8, 10}, {1, 3, 4, 1, 0, 5, 6, 7, 8, 6}, {1, 1, 1, 1, 5, 1, 1, 1, 1, 1}};
        QAP::Csr R{{0, 1, 2, 3, 4, 5, 6, 7}, {1, 1, 0, 0, 6, 6, 0}, {1, 1, 1, 1, 1, 1, 1}};
        QAP::Csr O{{0, 1, 2, 3, 4, 5, 6, 7}, {3, 4, 5, 6, 7, 8, 2}, {1, 1, 1, 1, 1, 1, 1}};
        QAP qap(ctx, M, NIO, L, R, O);
        std::vector<int64_t> wit;
        for (int64_t x : {3, 5}) {
            const int64_t u = x * x, v = u * x, w = v + x, x2 = w + 5, u2 = x2 * x2, v2 = u2 * x2;
            for (int64_t e : {(int64_t)1, x, v2 + x2, u, v, w, x2, u2, v2}) wit.push_back(e);
        }
        ps_phgr13_toxic tw;
        unsigned long draws[8] = {998877665ul, 1234577ul, 7654321ul, 424243ul, 31337ul, 271829ul, 3141593ul, 1618033ul};
        uint8_t* slots[8] = {tw.s, tw.av, tw.aw, tw.ay, tw.rv, tw.rw, tw.beta, tw.gamma};
        for (int i = 0; i < 8; i++) std::memcpy(slots[i], small(draws[i]).data(), 32);
        ps_phgr13_crs crs = NewPHGR13TrustedSetup(ctx, qap, tw);
        ps_phgr13_ek ek{};
        ek.vs = crs.vs; ek.ws = crs.ws; ek.ys = crs.ys; ek.vas = crs.vas; ek.was = crs.was; ek.yas = crs.yas;
        ek.gsi = crs.gsi; ek.vbs = crs.vbs; ek.wbs = crs.wbs; ek.ybs = crs.ybs; ek.lgsi = crs.lgsi;
        std::vector<ps_phgr13_proof> proofs = PHGR13ProveBatch(ctx, ek, qap, Poly::FromValues(ctx, wit), K, nullptr);
        CHECK(proofs.size() == K);

        ps_phgr13_vk vk{};
        std::memcpy(vk.av, crs.av, 192); std::memcpy(vk.aw, crs.aw, 96); std::memcpy(vk.ay, crs.ay, 192); std::memcpy(vk.gamma, crs.gamma, 192);
        std::memcpy(vk.bgamma, crs.bgamma, 96); std::memcpy(vk.bgamma2, crs.bgamma2, 192); std::memcpy(vk.yts, crs.yts, 192);
        ps_points *vs_io = nullptr, *ws_io = nullptr, *ys_io = nullptr;
        check(ps_points_slice(crs.vk_vs, 0, DIFF, &vs_io));
        check(ps_points_slice(crs.vk_ws, 0, DIFF, &ws_io));
        check(ps_points_slice(crs.vk_ys, 0, DIFF, &ys_io));
        vk.vs_io = vs_io; vk.ws_io = ws_io; vk.ys_io = ys_io;

        std::vector<Scalar> pub;
        for (size_t i = 0; i < K; i++)
            for (size_t j = 0; j < DIFF; j++) pub.push_back(small((unsigned long)wit[M * i + j]));
        Poly io(ctx, pub);
        std::vector<uint8_t> rho(32 * K, 0);
        for (size_t i = 0; i < K; i++)
            for (int k = 16; k < 32; k++) rho[32 * i + k] = (uint8_t)(41 * i + 7 * k + 3);

        ps_phgr13_batch_info info;
        CHECK(PHGR13VerifyBatch(ctx, vk, io, proofs, rho.data(), &info));
        CHECK(info.failed == 0 && info.device_loops == K + DIFF);
        CHECK(PHGR13Verify(ctx, vk, proofs[0], Poly(ctx, std::vector<Scalar>(pub.begin(), pub.begin() + DIFF))));
        std::vector<ps_phgr13_proof> bad = proofs;
        std::memcpy(bad[0].gz, proofs[1].gz, 96);
        CHECK(!PHGR13VerifyBatch(ctx, vk, io, bad, rho.data(), &info));
        CHECK(info.failed == (1u << 4));
        std::vector<uint8_t> zero(32 * K, 0);
        int code = 0;
        try { PHGR13VerifyBatch(ctx, vk, io, proofs, zero.data()); } catch (const Error& e) { code = e.code; }
        CHECK(code == PS_ERR_ARG);
        CHECK(PHGR13VerifyBatch(ctx, vk, io, proofs, rho.data()));

        ps_points_free(vs_io); ps_points_free(ws_io); ps_points_free(ys_io);
        ps_phgr13_crs_free(&crs);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "abi_smoke_phgr13_verify_batch_cpp: %s\n", e.what());
        return 1;
    }
    std::printf("abi_smoke_phgr13_verify_batch_cpp ok\n");
    return 0;
}
