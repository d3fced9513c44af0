// abi_smoke_qap_fr_cpp.cpp -- the C++ host mirror (playsnark_amd/host/playsnark.hpp) over a circuit with field-valued
// coefficients: the three MiMC-style rounds of tests/abi_smoke_qap_fr.c (constants 2^64, r - 1, 2^253 + 5) through
// QAP::CsrFr, QAP::wide_entries, QAP::Quotient on the witness and on a wrong one, and a coefficient equal to r.
//   g++ -std=c++17 -Wall -I. tests/abi_smoke_qap_fr_cpp.cpp -Lplaysnark_amd -lplaysnark_hip -o abi_smoke_qap_fr_cpp
// Exit codes: 0 ok, 77 no gfx950 device, 1 failure.
#include <cstdio>
#include <string>

#include "playsnark_amd/host/playsnark.hpp"

using namespace playsnark;

static Scalar hex(const std::string& h) {
    Scalar s{};
    for (size_t i = 0; i < 32; i++) s[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
    return s;
}
#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "abi_smoke_qap_fr_cpp: line %d: %s failed\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    const Scalar ONE = hex("0000000000000000000000000000000000000000000000000000000000000001");
    const Scalar C0 = hex("0000000000000000000000000000000000000000000000010000000000000000");  // 2^64
    const Scalar C1 = hex("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000");  // r - 1
    const Scalar C2 = hex("2000000000000000000000000000000000000000000000000000000000000005");  // 2^253 + 5
    const Scalar RR = hex("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001");  // r: not canonical
    const char* witness[8] = {  // [const, x, out, t0, x1, t1, x2, t2] for x = 3
        "0000000000000000000000000000000000000000000000000000000000000001",
        "0000000000000000000000000000000000000000000000000000000000000003",
        "1217d15b6d7965af30c9c946fa3a780103c5bcaca60ac48df61a92790c142da9",
        "0000000000000000000000000000000100000000000000060000000000000009",
        "00000000000000010000000000000009000000000000001b000000000000001b",
        "39a57377c968fcb99f9b9fc57bc15a7105f9a77cafca1e03fb2021460c7f8beb",
        "3c8cf6aa5c6e62511c892cf6fbb30b56336f5ffe1eb136e73f5e745bd05eb41e",
        "49914021ac8ff75410613b3d226b3974b0fdb4434ab4cb9d2085892b4523b65c",
    };
    try {
        Context ctx(0);
        QAP::CsrFr L{{0, 2, 3, 5, 6, 8, 9}, {1, 0, 3, 4, 0, 5, 6, 0, 7}, {ONE, C0, ONE, ONE, C1, ONE, ONE, C2, ONE}};
        QAP::CsrFr R{{0, 2, 4, 6, 8, 10, 12}, {1, 0, 1, 0, 4, 0, 4, 0, 6, 0, 6, 0}, {ONE, C0, ONE, C0, ONE, C1, ONE, C1, ONE, C2, ONE, C2}};
        QAP::CsrFr O{{0, 1, 2, 3, 4, 5, 6}, {3, 4, 5, 6, 7, 2}, {ONE, ONE, ONE, ONE, ONE, ONE}};
        QAP qap(ctx, 8, 3, L, R, O);
        const auto wide = qap.wide_entries();
        REQUIRE(wide[0] == 2 && wide[1] == 4 && wide[2] == 0);
        std::vector<Scalar> sol;
        for (const char* w : witness) sol.push_back(hex(w));
        Poly h = qap.Quotient(Poly(ctx, sol));
        REQUIRE(h.size() == 5);
        sol[7][31] ^= 1;
        bool threw = false;
        try { qap.Quotient(Poly(ctx, sol)); } catch (const Apocalypse&) { threw = true; }
        REQUIRE(threw);
        threw = false;
        QAP::CsrFr bad = R;
        bad.val[7] = RR;
        try { QAP q2(ctx, 8, 3, L, bad, O); } catch (const Error& e) { threw = e.code == PS_ERR_ENCODING; }
        REQUIRE(threw);
    } catch (const Error& e) {
        if (e.code == PS_ERR_NO_DEVICE) { std::printf("no gfx950 device: %s\n", e.what()); return 77; }
        std::fprintf(stderr, "abi_smoke_qap_fr_cpp: error %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("abi_smoke_qap_fr_cpp ok\n");
    return 0;
}
