// host_locate_descent.hpp -- locate_bisect (playsnark_amd/csrc/locate_descent.hpp), the descent both locating batch verifiers
// ship, run on the host by host_locate_index.cpp and host_phgr13_locate_index.cpp, which define CHECK before including this.
// Its `check` is an oracle: mask_of(level, node) -> the equations that fail on the leaves under a node of a tree of n leaves.
#pragma once
#include "../playsnark_amd/csrc/locate_descent.hpp"

struct Descent {
    int rc = 0;
    std::vector<ps::u32> leaves;
    std::vector<uint8_t> masks;
    ps::u32 checks = 0, levels = 0;
    ps::u64 products = 0;  // (set, equation) pairs handed to `check`
    size_t calls = 0;
    bool same(const Descent& o) const {
        return rc == o.rc && leaves == o.leaves && masks == o.masks && checks == o.checks && levels == o.levels && products == o.products;
    }
};
constexpr int STOPPED = 77;
constexpr size_t UNBOUNDED = ~(size_t)0;

// stop_at: the call of `check` that returns STOPPED instead of an answer (0: none)
template <class MaskOf>
Descent descend(ps::u64 n, const MaskOf& mask_of, size_t per_pass, size_t stop_at = 0) {
    ps::u64 size[ps::locate::MAX_LEVELS], off[ps::locate::MAX_LEVELS + 1];
    const int nl = ps::locate::tree_levels(n, size, off);
    Descent d;
    auto check = [&](int l, const ps::u32* idx, const uint8_t* pmask, size_t K, uint8_t* fmask) {
        d.calls++;
        CHECK(K >= 1 && K <= per_pass && l >= 0 && l < nl - 1, "n = %llu: a pass of %zu sets of level %d, per_pass = %zu", (unsigned long long)n, K, l, per_pass);
        CHECK(!stop_at || d.calls <= stop_at, "n = %llu: call %zu after the one that stopped the descent", (unsigned long long)n, d.calls);
        if (d.calls == stop_at) return STOPPED;
        for (size_t k = 0; k < K; k++) {
            CHECK(idx[k] < size[l] && pmask[k], "n = %llu: node %u of level %d, mask %u", (unsigned long long)n, idx[k], l, pmask[k]);
            for (unsigned m = pmask[k]; m; m &= m - 1) d.products++;
            const unsigned m = mask_of(l, idx[k]);
            CHECK((m & ~(unsigned)pmask[k]) == 0, "a child fails an equation its parent passed");
            fmask[k] = (uint8_t)(m & pmask[k]);
        }
        return 0;
    };
    d.rc = ps::locate_bisect(n, (uint8_t)mask_of(nl - 1, 0), per_pass, check, &d.leaves, &d.masks, &d.checks, &d.levels);
    return d;
}

// The descent with every set of a level in one pass; cut into passes of 1 and of 3 sets it must report the same, and an error
// of its second pass must end it with that code (the oracle itself checks the passes' sizes and that nothing runs after it)
template <class MaskOf>
Descent descend_every_way(ps::u64 n, const MaskOf& mask_of) {
    const Descent d = descend(n, mask_of, UNBOUNDED);
    CHECK(d.rc == 0 && d.leaves.size() == d.masks.size() && std::is_sorted(d.leaves.begin(), d.leaves.end()), "n = %llu: rc %d", (unsigned long long)n, d.rc);
    for (size_t per_pass : {(size_t)1, (size_t)3})
        CHECK(descend(n, mask_of, per_pass).same(d), "n = %llu: per_pass = %zu differs", (unsigned long long)n, per_pass);
    if (n > 1) {  // (one leaf: no check is made)
        const Descent e = descend(n, mask_of, 1, 2);
        CHECK(e.rc == STOPPED && e.calls == 2 && e.leaves.empty() && e.masks.empty(), "n = %llu: rc %d after %zu calls", (unsigned long long)n, e.rc, e.calls);
    }
    return d;
}
