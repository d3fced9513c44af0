// host_point_pass_predict.cpp -- which point pass the host launches for an admitted sum, checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// Compiles playsnark_amd/csrc/point_pass_predict.hpp and drives sequences of (key, device verdict) through PassHistory in
// the two roles the library has for it: predict() when a sum is launched, observe() when it is finished -- one sum at a
// time, and with sums in flight, where the launches run ahead of the finishes.
#include <cstdio>
#include <deque>
#include <vector>

#include "../playsnark_amd/csrc/point_pass_predict.hpp"

using namespace ps;

static int failures = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (failures++ < 20) {                                                  \
                std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                                  \
                std::fprintf(stderr, "\n");                                         \
            }                                                                       \
        }                                                                           \
    } while (0)

static const u32 U = ACC_BUCKETS, B = ACC_SLICES, BOTH = ACC_AUTO;

static int storages[64];  // addresses to tell arrays apart
static PassKey key_of(int array, u64 n = 1 << 20, int c = 20, int W = 13, int width = 16) {
    PassKey k;
    k.storage = &storages[array];
    k.n = n;
    k.G = 1ull << (c - 1);
    k.group = 1;
    k.c = c;
    k.W = W;
    k.width = width;
    return k;
}

struct Step { u32 launched; bool redo; };
// the sums of `verdicts` over one key with at most `depth` in flight: launch until the queue is full, then finish one per launch
static std::vector<Step> run(PassHistory& h, const PassKey& k, const std::vector<u32>& verdicts, size_t depth) {
    std::vector<Step> out(verdicts.size());
    std::deque<size_t> pending;
    size_t next = 0;
    while (next < verdicts.size() || !pending.empty()) {
        if (next < verdicts.size() && pending.size() < depth) {
            out[next].launched = h.predict(k);
            pending.push_back(next++);
        } else {
            const size_t i = pending.front();
            pending.pop_front();
            out[i].redo = h.observe(k, out[i].launched, verdicts[i]);
            CHECK(out[i].redo == (out[i].launched != BOTH && out[i].launched != verdicts[i]), "sum %zu", i);
        }
    }
    return out;
}

int main() {
    {  // first sight launches both; a repeated verdict is predicted
        PassHistory h;
        const auto s = run(h, key_of(0), {U, U, U, U, U, U}, 1);
        CHECK(s[0].launched == BOTH, "first sight");
        for (size_t i = 1; i < s.size(); i++) CHECK(s[i].launched == U && !s[i].redo, "sum %zu launched %u", i, s[i].launched);
        CHECK(h.counts().both == 1 && h.counts().one == 5 && h.counts().redone == 0, "counts");
        CHECK(h.size() == 1, "size %d", h.size());
    }
    {  // four in flight: no history until the first finish, so the first queue-full launches both
        PassHistory h;
        const auto s = run(h, key_of(0), {U, U, U, U, U, U}, 4);
        for (size_t i = 0; i < 4; i++) CHECK(s[i].launched == BOTH, "sum %zu", i);
        for (size_t i = 4; i < 6; i++) CHECK(s[i].launched == U, "sum %zu", i);
        CHECK(h.counts().both == 4 && h.counts().one == 2 && h.counts().redone == 0, "counts");
    }
    {  // a flip: a redo, PP_HOLD launches of both, then the new verdict is predicted
        PassHistory h;
        std::vector<u32> v = {U, U, B};
        for (int i = 0; i < PP_HOLD + 3; i++) v.push_back(B);
        const auto s = run(h, key_of(0), v, 1);
        CHECK(s[1].launched == U && !s[1].redo, "before the flip");
        CHECK(s[2].launched == U && s[2].redo, "the flip");
        for (int i = 0; i < PP_HOLD; i++) CHECK(s[3 + i].launched == BOTH && !s[3 + i].redo, "hold %d: %u", i, s[3 + i].launched);
        for (size_t i = 3 + PP_HOLD; i < s.size(); i++) CHECK(s[i].launched == B && !s[i].redo, "after the hold %zu: %u", i, s[i].launched);
        CHECK(h.counts().redone == 1 && h.counts().both == 1 + (unsigned)PP_HOLD && h.counts().one == 2 + 3, "counts");
    }
    {  // the flip happens while predicted sums are pending behind it: they were launched for U, are U, and are not redone
        PassHistory h;
        const auto s = run(h, key_of(0), {U, U, U, U, B, U, U, U, U}, 4);
        for (size_t i = 0; i < 4; i++) CHECK(s[i].launched == BOTH, "sum %zu", i);
        for (size_t i = 4; i < 8; i++) CHECK(s[i].launched == U, "sum %zu: %u", i, s[i].launched);
        CHECK(s[4].redo, "the flip");
        CHECK(s[8].launched == BOTH, "launched after the flip was seen: %u", s[8].launched);
        CHECK(h.counts().both == 5 && h.counts().one == 4 && h.counts().redone == 1, "counts %llu %llu %llu", h.counts().both, h.counts().one, h.counts().redone);
    }
    {  // an alternating stream pays ONE redo: every change seen during the hold starts the hold again
        PassHistory h;
        std::vector<u32> v;
        for (int i = 0; i < 64; i++) v.push_back(i % 2 ? B : U);
        const auto s = run(h, key_of(0), v, 1);
        CHECK(s[0].launched == BOTH && s[1].launched == U && s[1].redo, "the first flip meets a prediction");
        for (size_t i = 2; i < s.size(); i++) CHECK(s[i].launched == BOTH && !s[i].redo, "sum %zu: %u", i, s[i].launched);
        CHECK(h.counts().redone == 1 && h.counts().one == 1 && h.counts().both == 63, "counts");
        PassHistory h4;  // ... and with four in flight no more than one either
        run(h4, key_of(0), v, 4);
        CHECK(h4.counts().redone <= 1, "redone %llu", h4.counts().redone);
    }
    {  // B B B U B B one at a time: both, B, B, U launched as B (redo), then the hold
        PassHistory h;
        const auto s = run(h, key_of(0), {B, B, B, U, B, B}, 1);
        CHECK(s[0].launched == BOTH && s[1].launched == B && s[2].launched == B, "warm-up");
        CHECK(s[3].launched == B && s[3].redo, "the flip");
        CHECK(s[4].launched == BOTH && s[5].launched == BOTH && !s[4].redo && !s[5].redo, "the hold");
        CHECK(h.counts().both == 3 && h.counts().one == 3 && h.counts().redone == 1, "counts");
    }
    {  // a different key does not inherit a verdict: every member of the key is told apart
        PassHistory h;
        run(h, key_of(0), {U, U}, 1);
        PassKey others[9] = {key_of(1), key_of(0, 1 << 19), key_of(0, 1 << 20, 16), key_of(0, 1 << 20, 20, 12), key_of(0, 1 << 20, 20, 13, 4),
                             key_of(0), key_of(0), key_of(0), key_of(0)};
        others[5].table = &storages[9];
        others[6].first = 128;
        others[7].group = 2;
        others[8].sums = 7;
        for (const PassKey& k : others) CHECK(h.predict(k) == BOTH, "a key that was never seen");
        CHECK(h.predict(key_of(0)) == U, "the key that was");
        CHECK(h.size() == 1, "predict alone makes no entry: %d", h.size());
        // ... and keys keep their own verdicts side by side
        h.observe(others[0], BOTH, B);
        CHECK(h.predict(others[0]) == B && h.predict(key_of(0)) == U, "two keys");
    }
    {  // eviction: the history stays at PP_SLOTS entries and the least recently used key goes
        PassHistory h;
        for (int a = 0; a < PP_SLOTS; a++) h.observe(key_of(a), BOTH, a % 2 ? B : U);
        CHECK(h.size() == PP_SLOTS, "size %d", h.size());
        CHECK(h.predict(key_of(0)) == U, "key 0 is used again");  // now key 1 is the oldest
        for (int a = PP_SLOTS; a < 40; a++) {
            h.observe(key_of(a), BOTH, U);
            CHECK(h.size() == PP_SLOTS, "size %d after %d keys", h.size(), a + 1);
            CHECK(h.predict(key_of(0)) == U, "a key in use stays");
        }
        CHECK(h.predict(key_of(1)) == BOTH, "the least recently used key went");
        CHECK(h.predict(key_of(39)) == U, "the newest key is there");
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("host_point_pass_predict ok (hold %d, slots %d)\n", PP_HOLD, PP_SLOTS);
    return 0;
}
