// cm_pinned_ranges.h — PinnedRanges, the owner of the host ranges a run has page-locked (cm_host_register).
//
// cm_mapping_run registers the FASTQ parser's batch arrays and text blocks so that their copies are direct DMA.  The parser says
// (cm_fastq_set_release_hook, on whichever thread frees) before a block goes: no registration may outlive its block.  The list, its
// mutex, the cap, the overlap walk and the "unregister and erase" step are here, once.  The back end is two function pointers and a
// user pointer: the library passes cm_host_register / cm_host_unregister over its context, tests/diag/pinned_san_main.cpp fakes.
#ifndef CM_PINNED_RANGES_H
#define CM_PINNED_RANGES_H

#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

struct __attribute__((visibility("hidden"))) PinnedRanges {          // (internal to the library: no exported name)
    // Past this many live registrations nothing more is registered: the copies then go through pageable staging.  (The parser
    // reuses four generations of four arrays, 16 live ranges; only batches that keep growing could pile up more.)
    static constexpr size_t kMax = 64;
    int (*reg)(void *user, void *p, uint64_t bytes) = nullptr;        // 0: registered
    int (*unreg)(void *user, void *p, const char **msg) = nullptr;    // 0: unregistered; else *msg may say why (valid until the next call)
    void *user = nullptr;
    // Unregistrations the back end refused -- their entries are gone all the same -- and what it said of the first.  For the
    // thread that owns the object, once no other is in a call.
    uint64_t failed = 0;
    std::string first_message;

    // Page-lock [p, p + bytes).  Inside a live registration: nothing to do.  Otherwise every registration it overlaps (the same
    // block, handed out longer or at another offset) is dropped and their union is registered.  A refused registration is not an
    // error and is not recorded: the copy is then a staged pageable one.
    void cover(const void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        const char *lo = (const char *)p, *hi = lo + bytes;
        if (!bytes || sweep(lo, hi, true) || v.size() >= kMax) return;
        if (reg(user, (void *)lo, (uint64_t)(hi - lo)) == 0) v.emplace_back((char *)lo, (uint64_t)(hi - lo));
    }
    // The block [p, p + bytes) is about to be freed: every registration that overlaps it goes first.
    void release(const void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        const char *lo = (const char *)p, *hi = lo + bytes;
        (void)sweep(lo, hi, false);
    }
    void clear() {
        std::lock_guard<std::mutex> lk(mu);
        while (!v.empty()) drop(v.begin());
    }
    ~PinnedRanges() { clear(); }
private:
    typedef std::vector<std::pair<char *, uint64_t>> List;
    std::mutex mu;
    List v;
    // the one way an entry leaves the list: with the call, whose status is kept
    List::iterator drop(List::iterator it) {
        const char *msg = nullptr;
        if (unreg(user, it->first, &msg) != 0 && failed++ == 0) first_message = msg ? msg : "";
        return v.erase(it);
    }
    // the one overlap walk: drops every entry that overlaps [lo, hi).  With `widen` it stops, true, at an entry that holds the
    // whole range, and lo / hi grow to the union with what was dropped.
    bool sweep(const char *&lo, const char *&hi, bool widen) {
        for (auto it = v.begin(); it != v.end();) {
            const char *a0 = it->first, *a1 = a0 + it->second;
            if (widen && lo >= a0 && hi <= a1) return true;
            if (lo < a1 && hi > a0) {
                if (widen) lo = std::min(lo, a0), hi = std::max(hi, a1);
                it = drop(it);
            } else ++it;
        }
        return false;
    }
};

#endif /* CM_PINNED_RANGES_H */
