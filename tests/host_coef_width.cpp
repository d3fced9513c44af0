// host_coef_width.cpp -- how the column sums over points classify a coefficient, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// playsnark_amd/csrc/coef_width.hpp turns a canonical value v < r into the signed magnitude min(v, r - v) (negative above
// (r - 1) / 2), counts the 64-bit words it needs and calls it wide from two words on; coef_be32_is_canonical is the range
// test of ps_qap_create_fr.  Reads 64-digit hexadecimal values, one per line, from standard input and prints for each
//     <canonical 0|1> <negative 0|1> <wide 0|1> <words64> <magnitude, 64 hex digits>
// (the last four as 0 0 0 0 for a value that is not canonical) for tests/test_coef_width_host.py to compare with Python
// integers.
#include <cstdio>
#include <cstring>

#ifndef COEF_WIDTH_HEADER
#define COEF_WIDTH_HEADER "../playsnark_amd/csrc/coef_width.hpp"
#endif
#include COEF_WIDTH_HEADER

static int hexval(char ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    return -1;
}

int main() {
    char line[128];
    size_t count = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        size_t len = std::strlen(line);
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len == 0) continue;
        if (len != 64) { std::fprintf(stderr, "host_coef_width: line of %zu characters\n", len); return 1; }
        uint8_t be[32];
        for (int i = 0; i < 32; i++) {
            const int hi = hexval(line[2 * i]), lo = hexval(line[2 * i + 1]);
            if (hi < 0 || lo < 0) { std::fprintf(stderr, "host_coef_width: not a hexadecimal digit\n"); return 1; }
            be[i] = (uint8_t)(hi << 4 | lo);
        }
        count++;
        if (!ps::coef_be32_is_canonical(be)) {
            std::printf("0 0 0 0 %064d\n", 0);
            continue;
        }
        uint32_t v[8], mag[8];
        for (int i = 0; i < 8; i++) {
            const uint8_t* p = be + 4 * (7 - i);
            v[i] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
        }
        const bool neg = ps::coef_signed_magnitude(mag, v);
        std::printf("1 %d %d %d ", neg ? 1 : 0, ps::coef_is_wide(mag) ? 1 : 0, ps::coef_words64(mag));
        for (int i = 7; i >= 0; i--) std::printf("%08x", mag[i]);
        std::printf("\n");
    }
    std::printf("host_coef_width ok %zu\n", count);
    return 0;
}
