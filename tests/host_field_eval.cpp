// host_field_eval.cpp -- the C++ forms of field.hpp's products compiled for the HOST (g++), with the same interface as
// device_field_check.hip (OP N IN OUT, int32 words).  tests/test_device_field.py uses it to anchor the Python emulation
// (tests/field_model.py) to the product's source before any GPU time is spent.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../playsnark_amd/csrc/field.hpp"

using namespace ps;

static Fp ld(const i32* p) { Fp r; for (int i = 0; i < FP_L; i++) r.l[i] = p[i]; return r; }
static void st(i32* o, const Fp& a) { for (int i = 0; i < FP_L; i++) o[i] = a.l[i]; }
static Fr ldr(const i32* p) { Fr r; for (int i = 0; i < FR_L; i++) r.l[i] = p[i]; return r; }
static void str(i32* o, const Fr& a) { for (int i = 0; i < FR_L; i++) o[i] = a.l[i]; }

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const char* op = argv[1];
    const long n = std::atol(argv[2]);
    int in = 0, out = FP_L;
    if (!std::strcmp(op, "fp_mul") || !std::strcmp(op, "fp_mul_ilp")) in = 28;
    else if (!std::strcmp(op, "fp_sqr") || !std::strcmp(op, "fp_norm")) in = 14;
    else if (!std::strcmp(op, "fp_mul2sub") || !std::strcmp(op, "fp_mul2add") || !std::strcmp(op, "fp_mul2sub_ilp")) in = 56;
    else if (!std::strcmp(op, "fp_mul2add2sub") || !std::strcmp(op, "fp_mulsum_ilp4")) in = 112;
    else if (!std::strcmp(op, "fr_mul")) { in = 20; out = FR_L; }
    else return 2;
    std::vector<i32> h(n * in), o(n * out);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f || std::fread(h.data(), 4, h.size(), f) != h.size()) return 2;
    std::fclose(f);
    for (long c = 0; c < n; c++) {
        const i32* x = h.data() + c * in;
        i32* y = o.data() + c * out;
        if (!std::strcmp(op, "fp_mul")) st(y, f_mul(ld(x), ld(x + 14)));
        else if (!std::strcmp(op, "fp_mul_ilp")) st(y, f_mul_ilp(ld(x), ld(x + 14)));
        else if (!std::strcmp(op, "fp_sqr")) st(y, f_sqr(ld(x)));
        else if (!std::strcmp(op, "fp_norm")) st(y, f_norm(ld(x)));
        else if (!std::strcmp(op, "fp_mul2sub")) st(y, f_mul2sub(ld(x), ld(x + 14), ld(x + 28), ld(x + 42)));
        else if (!std::strcmp(op, "fp_mul2add")) st(y, f_mul2add(ld(x), ld(x + 14), ld(x + 28), ld(x + 42)));
        else if (!std::strcmp(op, "fp_mul2sub_ilp")) st(y, f_mul2sub_ilp(ld(x), ld(x + 14), ld(x + 28), ld(x + 42)));
        else if (!std::strcmp(op, "fp_mul2add2sub"))
            st(y, f_mul2add2sub(ld(x), ld(x + 14), ld(x + 28), ld(x + 42), ld(x + 56), ld(x + 70), ld(x + 84), ld(x + 98)));
        else if (!std::strcmp(op, "fp_mulsum_ilp4")) {
            const Fp a[4] = {ld(x), ld(x + 28), ld(x + 56), ld(x + 84)}, b[4] = {ld(x + 14), ld(x + 42), ld(x + 70), ld(x + 98)};
            const bool neg[4] = {false, false, true, true};
            st(y, f_mulsum_ilp<4>(a, b, neg));
        } else str(y, fr_mul(ldr(x), ldr(x + 10)));
    }
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(o.data(), 4, o.size(), f) != o.size()) return 2;
    std::fclose(f);
    return 0;
}
