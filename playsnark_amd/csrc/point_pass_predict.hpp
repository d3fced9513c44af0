// Which point pass a sum will take, guessed on the host from the sums before it (msm.hpp section 4b, bucket_order.hpp).
//
// An admitted sum (ACC_AUTO) has both point passes to choose from and the device picks one at the end of the sort: the
// verdict word.  Enqueueing both families -- k_bucket_sum, and k_accumulate with its fix-up kernels -- costs the family not
// taken thousands of workgroups that must win a wave slot from another sum's accumulation only to return.  The verdict of a
// finished sum reaches the host ahead of its results, and the sums of one caller over one key look alike: the host
// launches only the family the last sum of the same shape took, and checks the guess when the sum finishes.
//
//   launch   PassHistory::predict(key)   ACC_AUTO: launch both families (no history, or the hold after a change)
//                                        ACC_SLICES / ACC_BUCKETS: launch that family only
//   finish   PassHistory::observe(key, launched, verdict)   true: the launched family was not the device's choice, the
//                                        buckets were never computed and the point pass must run again with `verdict`
//
// A change of the verdict (seen at a finish, whatever was launched) holds the key on "both" for PP_HOLD launches, and every
// further change during the hold starts it again: a stream of sums that alternates pays one redo, not one per sum.
// A wrong guess costs time only -- every kernel of both families reads the verdict word and returns when it names the
// other one -- so a stale entry (a freed array whose address is used again) is harmless.
//
// Pure logic: no HIP calls, compiles for the host (tests/host_point_pass_predict.cpp).  One history per context, used by
// the thread that owns the context: no lock.
#pragma once
#include "bucket_order.hpp"

namespace ps {

constexpr int PP_SLOTS = 8;  // keys remembered per context (a prover has three to seven arrays; the least recently used goes)
constexpr int PP_HOLD = 4;   // launches of both families after a change of the verdict: one queue-full (PS_MSM_QUEUE)

// What determines the plan of a sum and, with the caller's habits, its fill: the array (its storage, the table the entries
// index, the view's offset), the length, the window, the bucket sets, and the width class of the scalars.
struct PassKey {
    const void* storage = nullptr;  // the points' allocation
    const void* table = nullptr;    // base of the window table or view table the pass reads, nullptr: the plain plan
    u64 first = 0, n = 0, G = 0;
    int group = 0, c = 0, W = 0;
    int width = 0;                  // pp_width_class of the scalars
    int sums = 1;                   // point passes over the one sort (ps_msm_multi, the provers' solution sums: one verdict for all)
    bool operator==(const PassKey& o) const {
        return storage == o.storage && table == o.table && first == o.first && n == o.n && G == o.G && group == o.group && c == o.c &&
               W == o.W && width == o.width && sums == o.sums;
    }
};
// scalars of one width class have the same number of significant 32-bit words; int64 vectors with negative values (folded to
// r - |v| on the device) are a class of their own
inline int pp_width_class(int max_bits, bool neg_small) { return ((max_bits + 31) / 32) * 2 + (neg_small ? 1 : 0); }

struct PassCounts {
    unsigned long long both = 0, one = 0, redone = 0;  // admitted sums launched with both families, with one, and summed twice
};

class PassHistory {
public:
    // the families to launch for the next sum of `key`; counts the launch
    u32 predict(const PassKey& key) {
        Entry* e = find(key);
        u32 family = ACC_AUTO;
        if (e) {
            e->used = ++clock_;
            if (e->hold > 0) e->hold--;
            else family = e->verdict;
        }
        (family == ACC_AUTO ? counts_.both : counts_.one)++;
        return family;
    }
    // a sum of `key` launched with `launched` (what predict returned) finished with the device's `verdict`
    // (ACC_SLICES / ACC_BUCKETS).  Returns whether its point pass must be run again.
    bool observe(const PassKey& key, u32 launched, u32 verdict) {
        const bool redo = launched != ACC_AUTO && launched != verdict;
        if (redo) counts_.redone++;
        Entry* e = find(key);
        if (!e) {
            e = victim();
            e->key = key;
            e->live = true;
            e->hold = 0;
        } else if (e->verdict != verdict) {
            e->hold = PP_HOLD;
        }
        e->verdict = verdict;
        e->used = ++clock_;
        return redo;
    }
    const PassCounts& counts() const { return counts_; }
    int size() const {
        int k = 0;
        for (const Entry& e : slots_) k += e.live ? 1 : 0;
        return k;
    }

private:
    struct Entry {
        PassKey key;
        u32 verdict = ACC_AUTO;
        int hold = 0;  // launches of both families still to come
        unsigned long long used = 0;
        bool live = false;
    };
    Entry* find(const PassKey& key) {
        for (Entry& e : slots_)
            if (e.live && e.key == key) return &e;
        return nullptr;
    }
    Entry* victim() {  // a free slot, else the least recently used
        Entry* v = &slots_[0];
        for (Entry& e : slots_) {
            if (!e.live) return &e;
            if (e.used < v->used) v = &e;
        }
        return v;
    }
    Entry slots_[PP_SLOTS];
    unsigned long long clock_ = 0;
    PassCounts counts_;
};

}  // namespace ps
