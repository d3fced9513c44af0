// The bisection of both locating batch verifiers (verify_locate.inc, verify_phgr13_locate.inc).  Plain C++17, no HIP, none of
// the library's types: tests/host_locate_index.cpp and tests/host_phgr13_locate_index.cpp run THIS loop under ASan + UBSan.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "locate_dev.hpp"

namespace ps {

// From the root (mask `root` of failed equations) down over a tree of N >= 1 leaves: both children of every failing node are
// tested on the equations of the parent's mask alone, all nodes of a level in one round, cut into passes of at most per_pass
// sets; a node with one (carried) child hands verdict and mask down without a check.  check(level, idx, pmask, K, fmask) -> rc
// fills fmask[k] with the failing subset of pmask[k] for the K nodes idx[] of `level`; a non-zero rc is returned at once.
// leaves / masks: the failing leaves in ascending order.  *checks grows by the sets tested, *levels is the levels walked
// (N == 1: the root is the leaf, no check is made and neither is touched).
template <class Check>
int locate_bisect(u64 N, uint8_t root, size_t per_pass, Check&& check, std::vector<u32>* leaves, std::vector<uint8_t>* masks, u32* checks, u32* levels) {
    u64 size[locate::MAX_LEVELS], off[locate::MAX_LEVELS + 1];
    const int nl = locate::tree_levels(N, size, off);
    std::vector<std::pair<u32, uint8_t>> failing{{0, root}};  // (node, mask), sorted by node
    for (int l = nl - 1; l > 0 && !failing.empty(); l--) {
        std::vector<std::pair<u32, uint8_t>> below;
        std::vector<u32> tests;
        std::vector<uint8_t> tmasks;
        for (const auto& node : failing) {
            const u32 i = node.first;
            if (locate::node_has_two_children(i, size[l - 1])) {
                for (u32 ch : {2 * i, 2 * i + 1}) { tests.push_back(ch); tmasks.push_back(node.second); }
            } else {
                below.push_back({2 * i, node.second});  // carried: the same set, the same verdict, the same mask
            }
        }
        std::vector<uint8_t> got(tests.size(), 0);
        for (size_t at = 0; at < tests.size(); at += per_pass)
            if (int rc = check(l - 1, tests.data() + at, tmasks.data() + at, std::min(per_pass, tests.size() - at), got.data() + at)) return rc;
        for (size_t k = 0; k < tests.size(); k++)
            if (got[k]) below.push_back({tests[k], got[k]});
        std::sort(below.begin(), below.end());
        failing.swap(below);
        *checks += (u32)tests.size();
        *levels = (u32)(nl - l);
    }
    for (const auto& leaf : failing) { leaves->push_back(leaf.first); masks->push_back(leaf.second); }
    return 0;
}

}  // namespace ps
