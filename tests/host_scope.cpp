// host_scope.cpp -- playsnark_amd/csrc/scope.hpp (the one owner of a library call's temporaries), checked on the host.
//     g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
// The header includes nothing of HIP and nothing of the library, so this file supplies counting stand-ins for the names it
// uses -- hipStream_t, hipError_t, hipMalloc, hipFree, hipStreamSynchronize, two handle types with their frees, g_last_error --
// and logs every call.  Device buffers and handles are real heap blocks: ASan's leak and double-free checks back the counters.
//   * a body that takes k handles and j device buffers and returns at each of its k + j + 1 points frees each acquired thing
//     exactly once;
//   * the stream is synchronised exactly once, before the first hipFree, when the scope holds scratch, and not at all otherwise
//     (in_flight(): once on every way out but finish(0));
//   * device buffers go in reverse order of allocation, then handles in reverse order;
//   * a registered result survives finish(0) untouched, is freed and nulled on every other way out, the code passed through;
//   * g_last_error is the same string after the scope as before it, even when a free overwrites it;
//   * a slot's address is unchanged after 1 000 more slots;
//   * a failed device<T>() records nothing and leaves the earlier buffers to be freed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

// ---- stand-ins ----
typedef int hipStream_t;
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static std::string g_last_error;

struct Event { char what; const void* p; };  // 'Y' sync, 'D' hipFree, 'P' ps_points_free, 'S' ps_scalars_free
static std::vector<Event> g_log;
static std::map<const void*, int> g_freed;   // frees per address
static int g_mallocs = 0, g_fail_malloc_at = -1, g_sync_stream = -1;
static size_t g_last_bytes = 0;

static hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_mallocs++ == g_fail_malloc_at) return hipErrorOutOfMemory;
    g_last_bytes = bytes;
    *p = std::malloc(bytes);
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    g_log.push_back({'D', p});
    g_freed[p]++;
    g_last_error = "overwritten by hipFree";
    std::free(p);
    return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t st) {
    g_log.push_back({'Y', nullptr});
    g_sync_stream = st;
    return hipSuccess;
}
struct ps_points { int id; };
struct ps_scalars { int id; };
static void ps_points_free(ps_points* p) {  // (null is a no-op, as in the library)
    if (!p) return;
    g_log.push_back({'P', p});
    g_freed[p]++;
    g_last_error = "overwritten by ps_points_free";
    delete p;
}
static void ps_scalars_free(ps_scalars* s) {
    if (!s) return;
    g_log.push_back({'S', s});
    g_freed[s]++;
    g_last_error = "overwritten by ps_scalars_free";
    delete s;
}

#ifndef SCOPE_HEADER
#define SCOPE_HEADER "../playsnark_amd/csrc/scope.hpp"
#endif
#include SCOPE_HEADER

static int failures = 0;
#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        if (!(cond)) {                                                               \
            if (failures++ < 20) {                                                   \
                std::fprintf(stderr, "FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); \
                std::fprintf(stderr, __VA_ARGS__);                                   \
                std::fprintf(stderr, "\n");                                          \
            }                                                                        \
        }                                                                            \
    } while (0)

static void reset() {
    g_log.clear();
    g_freed.clear();
    g_mallocs = 0;
    g_fail_malloc_at = -1;
    g_sync_stream = -1;
    g_last_error.clear();
}

// A function body in the library's style: acquisition i of `order` ('P' points, 'S' scalars, 'D' device scratch), a return
// after `stop` of them.  What it acquired goes to `got` in order.
static int body(const std::string& order, size_t stop, std::vector<Event>* got) {
    Scope scope(7);
    for (size_t i = 0; i < order.size(); i++) {
        if (i == stop) {
            g_last_error = "the error of this return";
            return 100 + (int)i;
        }
        if (order[i] == 'D') {
            double* d = nullptr;
            if (scope.device(&d, i) != hipSuccess) return -1;
            got->push_back({'D', d});
        } else if (order[i] == 'P') {
            ps_points** p = scope.points();
            *p = new ps_points{(int)i};
            got->push_back({'P', *p});
        } else {
            ps_scalars** s = scope.scalars();
            *s = new ps_scalars{(int)i};
            got->push_back({'S', *s});
        }
    }
    g_last_error = "the error of this return";
    return 0;
}

static void check_every_return(const std::string& order) {
    for (size_t stop = 0; stop <= order.size(); stop++) {
        reset();
        std::vector<Event> got;
        const int rc = body(order, stop, &got);
        CHECK(rc == (stop < order.size() ? 100 + (int)stop : 0), "%s stop %zu: rc %d", order.c_str(), stop, rc);
        CHECK(g_last_error == "the error of this return", "%s stop %zu: error text '%s'", order.c_str(), stop, g_last_error.c_str());
        // exactly once each, and nothing else
        for (const Event& e : got) CHECK(g_freed[e.p] == 1, "%s stop %zu: a '%c' freed %d times", order.c_str(), stop, e.what, g_freed[e.p]);
        size_t frees = 0, syncs = 0;
        for (const Event& e : g_log) (e.what == 'Y' ? syncs : frees)++;
        CHECK(frees == got.size(), "%s stop %zu: %zu frees of %zu things", order.c_str(), stop, frees, got.size());
        // the expected log: [sync] + device buffers in reverse + handles in reverse
        std::vector<Event> want;
        bool scratch = false;
        for (const Event& e : got) scratch = scratch || e.what == 'D';
        if (scratch) want.push_back({'Y', nullptr});
        for (size_t i = got.size(); i-- > 0;)
            if (got[i].what == 'D') want.push_back(got[i]);
        for (size_t i = got.size(); i-- > 0;)
            if (got[i].what != 'D') want.push_back(got[i]);
        CHECK(syncs == (scratch ? 1u : 0u), "%s stop %zu: %zu synchronisations", order.c_str(), stop, syncs);
        CHECK(!scratch || g_sync_stream == 7, "%s stop %zu: synchronised stream %d", order.c_str(), stop, g_sync_stream);
        bool same = want.size() == g_log.size();
        for (size_t i = 0; same && i < want.size(); i++) same = want[i].what == g_log[i].what && want[i].p == g_log[i].p;
        CHECK(same, "%s stop %zu: order of the %zu releases", order.c_str(), stop, g_log.size());
    }
}

// a call with two results: rc == 0 keeps them, every other way out frees and nulls them
static int makes_results(int rc, bool through_finish, ps_points** out_p, ps_scalars** out_s) {
    Scope scope;
    *scope.result(out_p) = new ps_points{1};
    *scope.result(out_s) = new ps_scalars{2};
    *scope.points() = new ps_points{3};  // a temporary beside them
    if (!through_finish) return rc;      // a return from the middle
    return scope.finish(rc);
}

int main() {
    // ---- every return point of bodies with k handles and j buffers, in several interleavings (k, j in 0..4) ----
    for (const char* order : {"", "P", "S", "D", "PS", "DD", "PDSD", "DPDSP", "PPSS", "DDDD", "SDPDSDPD", "DSSPPDDS"}) check_every_return(order);

    // ---- sizes: max(count, 1) elements ----
    {
        reset();
        Scope scope;
        double* a = nullptr;
        char* b = nullptr;
        CHECK(scope.device(&a, 5) == hipSuccess && g_last_bytes == 40, "%zu bytes for 5 doubles", g_last_bytes);
        CHECK(scope.device(&b, 0) == hipSuccess && g_last_bytes == 1 && b, "%zu bytes for no element", g_last_bytes);
    }

    // ---- results ----
    for (int through_finish = 0; through_finish < 2; through_finish++)
        for (int rc : {0, 7}) {
            reset();
            ps_points* p = (ps_points*)0x10;  // garbage on entry: registering nulls it
            ps_scalars* s = (ps_scalars*)0x10;
            g_last_error = "kept";
            const int got = makes_results(rc, through_finish != 0, &p, &s);
            CHECK(got == rc, "code %d came back as %d", rc, got);
            CHECK(g_last_error == "kept", "error text '%s'", g_last_error.c_str());
            if (rc == 0 && through_finish) {
                CHECK(p && s && p->id == 1 && s->id == 2, "results of a successful call");
                CHECK(g_log.size() == 1 && g_log[0].what == 'P' && g_freed[p] == 0 && g_freed[s] == 0, "only the temporary is freed: %zu releases", g_log.size());
                delete p;
                delete s;
            } else {
                CHECK(!p && !s, "results of a failed call are nulled");
                CHECK(g_log.size() == 3, "both results and the temporary are freed: %zu releases", g_log.size());
                for (auto& f : g_freed) CHECK(f.second == 1, "freed %d times", f.second);
            }
        }

    // ---- the error text, with nothing in the scope and with everything ----
    {
        reset();
        g_last_error = "before";
        { Scope scope; }
        CHECK(g_last_error == "before" && g_log.empty(), "an empty scope does nothing");
        {
            KeepError keep;
            g_last_error = "changed inside";
        }
        CHECK(g_last_error == "before", "KeepError: '%s'", g_last_error.c_str());
    }

    // ---- stable addresses ----
    {
        reset();
        Scope scope;
        ps_points** first_p = scope.points();
        ps_scalars** first_s = scope.scalars();
        *first_p = new ps_points{-1};
        *first_s = new ps_scalars{-2};
        ps_points* const was_p = *first_p;
        ps_scalars* const was_s = *first_s;
        std::vector<ps_points**> all;
        for (int i = 0; i < 1000; i++) {
            all.push_back(scope.points());
            *scope.scalars() = new ps_scalars{i};
        }
        CHECK(*first_p == was_p && *first_s == was_s && (*first_p)->id == -1 && (*first_s)->id == -2, "the first slots moved");
        for (size_t i = 1; i < all.size(); i++) CHECK(all[i] != all[i - 1] && *all[i] == nullptr, "slot %zu", i);
    }

    // ---- a failed allocation: nothing recorded, the earlier buffers still freed, once, after one synchronisation ----
    for (int fail_at = 0; fail_at < 3; fail_at++) {
        reset();
        g_fail_malloc_at = fail_at;
        std::vector<void*> made;
        {
            Scope scope(3);
            for (int i = 0; i < 3; i++) {
                int* d = (int*)0x10;
                const hipError_t e = scope.device(&d, 4);
                CHECK((e == hipSuccess) == (i != fail_at), "allocation %d of a run failing at %d", i, fail_at);
                if (e != hipSuccess) { CHECK(d == nullptr, "a failed allocation leaves a pointer"); break; }
                made.push_back(d);
            }
        }
        CHECK((int)made.size() == fail_at, "%zu buffers before the failure at %d", made.size(), fail_at);
        CHECK(g_log.size() == (made.empty() ? 0 : made.size() + 1), "%zu calls for %zu buffers", g_log.size(), made.size());
        for (size_t i = 0; i < made.size(); i++) CHECK(g_log[1 + i].what == 'D' && g_log[1 + i].p == made[made.size() - 1 - i], "release %zu", i);
        if (!made.empty()) CHECK(g_log[0].what == 'Y' && g_sync_stream == 3, "the synchronisation comes first");
    }

    // ---- in_flight(): waits without scratch on every way out but finish(0); never twice ----
    for (int how = 0; how < 3; how++) {  // 0: return from the middle, 1: finish(5), 2: finish(0)
        reset();
        {
            Scope scope(9);
            scope.in_flight();
            if (how) (void)scope.finish(how == 1 ? 5 : 0);
        }
        CHECK(g_log.size() == (how == 2 ? 0u : 1u) && (how == 2 || (g_log[0].what == 'Y' && g_sync_stream == 9)), "in_flight, way out %d: %zu calls", how, g_log.size());
        reset();
        {
            Scope scope(9);
            float* d = nullptr;
            scope.in_flight();
            (void)scope.device(&d, 1);
            if (how) (void)scope.finish(how == 1 ? 5 : 0);
        }
        CHECK(g_log.size() == 2 && g_log[0].what == 'Y' && g_log[1].what == 'D', "in_flight with scratch, way out %d: %zu calls", how, g_log.size());
    }

    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("host_scope ok");
    return 0;
}
