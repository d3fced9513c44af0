// What one library call makes along the way -- temporary handles, slices, device scratch -- lives in ONE Scope on its stack and
// is released on every way out, once, after the stream is idle, with the error text kept.  Long-lived owners ("Who
// frees what") do not go through it.
//
// Includes nothing of HIP and nothing of the library: the including file has declared hipStream_t, hipError_t, hipSuccess,
// hipMalloc, hipFree, hipStreamSynchronize, ps_points / ps_points_free, ps_scalars / ps_scalars_free and g_last_error
// (capi.hip does; tests/host_scope.cpp supplies counting stand-ins).
#pragma once
#include <algorithm>
#include <deque>
#include <string>
#include <vector>

// g_last_error as it was, put back at the end of the block: for frees and drains that run the library's own entry points
struct KeepError {
    std::string text = g_last_error;
    ~KeepError() { g_last_error = text; }
    KeepError() = default;
    KeepError(const KeepError&) = delete;
};

class Scope {
public:
    explicit Scope(hipStream_t stream = hipStream_t()) : st(stream) {}
    Scope(const Scope&) = delete;
    Scope& operator=(const Scope&) = delete;

    // A null slot for the out-parameter of ps_*_slice / *_alloc / ps_*_upload; its address holds while the scope lives (deque).
    ps_points** points() { slots.push_back({}); return &slots.back().p; }
    ps_scalars** scalars() { slots.push_back({}); return &slots.back().s; }
    // hipMalloc of max(count, 1) elements; a failure records nothing and leaves *p null
    template <class T>
    hipError_t device(T** p, size_t count) {
        void* raw = nullptr;
        *p = nullptr;
        const hipError_t e = hipMalloc(&raw, sizeof(T) * std::max<size_t>(count, 1));
        if (e != hipSuccess) return e;
        dev.push_back(raw);
        *p = (T*)raw;
        return e;
    }
    // The stream has work in flight on memory the caller takes back at return (a copy from a pageable buffer): every way out
    // but finish(0), which the call reaches with the stream idle, waits for it even without scratch.
    void in_flight() { wait = true; }
    // *out, nulled here, is the caller's once finish(0) has been called; on every other way out it is freed and nulled again.
    ps_points** result(ps_points** out) { *out = nullptr; rpt.push_back(out); return out; }
    ps_scalars** result(ps_scalars** out) { *out = nullptr; rsc.push_back(out); return out; }
    int finish(int rc) { ok = rc == 0; return rc; }

    ~Scope() {
        KeepError keep;
        if (!dev.empty() || (wait && !ok)) (void)hipStreamSynchronize(st);
        for (auto p = dev.rbegin(); p != dev.rend(); ++p) (void)hipFree(*p);
        for (auto h = slots.rbegin(); h != slots.rend(); ++h) { ps_points_free(h->p); ps_scalars_free(h->s); }
        if (ok) return;
        for (ps_scalars** r : rsc) { ps_scalars_free(*r); *r = nullptr; }
        for (ps_points** r : rpt) { ps_points_free(*r); *r = nullptr; }
    }

private:
    hipStream_t st;
    bool wait = false, ok = false;
    std::vector<void*> dev;
    struct Slot { ps_points* p = nullptr; ps_scalars* s = nullptr; };  // one of the two
    std::deque<Slot> slots;
    std::vector<ps_scalars**> rsc;
    std::vector<ps_points**> rpt;
};
