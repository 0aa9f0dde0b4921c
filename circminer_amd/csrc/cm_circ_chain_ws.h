// cm_circ_chain_ws.h — the device workspace of cm_circ_chain_run (cm_circ_chain.hip), owned by the context (cm_hot.hip).
//
// The two translation units stay separate: cm_hot.hip is compiled once per kernel build and holds one of these per context,
// cm_circ_chain.hip is compiled once and fills it.  Plain data: nothing here depends on CM_MAX_CHAIN_FRAGS.
//
// Every buffer is grow-only: a call that needs more than a buffer holds frees it and allocates what it needs, a call that needs
// less uses the front of what is there.  The per-wave slices (score / prev / log / seen) are sized by `workers` problems at a time;
// how many of those the device holds is decided from the free memory when the slices are first sized (`max_workers`), and again
// when CM_CIRC_LOG_CAP has changed the size of a slice.  The per-group buffers are reused from group to group inside a call (a
// group ends with a synchronisation of the stream).  cm_destroy releases everything through cc_ws_release.
//
// Two consequences of owning the memory.  `max_workers` is not looked at again while the slice size stays the same: a later, larger
// call grows the slices up to that figure, and if the context's free memory has shrunk since (more contigs, a larger batch) the
// growth fails with CM_ENOMEM where a per-call rule would have taken fewer waves.  And what the calls have grown -- about 1.8 GiB
// after a call of 1024 or more problems at the default log capacity -- stays held for the life of the context, the mapping
// rounds that follow included.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

enum CcWsBuf {
    // per call
    CCW_REQ, CCW_SEQS, CCW_GENEOF, CCW_FRAGBASE, CCW_RES, CCW_CSCORE, CCW_CLEN, CCW_RPOS, CCW_QPOS, CCW_CURSOR, CCW_COUNTERS,
    // per resident wave
    CCW_SCORE, CCW_PREV, CCW_LOG, CCW_SEEN,
    // per gene group
    CCW_GENES, CCW_OFF, CCW_CNT, CCW_LOC, CCW_ARENA, CCW_ORDER,
    CCW_COUNT
};
struct cm_circ_chain_ws {
    void *p[CCW_COUNT];
    size_t bytes[CCW_COUNT];
    uint32_t max_workers;        // the most the device holds slices for (a quarter of the free memory at first sizing, 1024 at the most); 0: not sized yet
    uint32_t log_cap, seen_cap;  // what a slice was sized with
    uint64_t allocations;        // hipMalloc calls so far, over the life of the workspace
    uint64_t held;               // bytes held now
};

// buffer `which` holds at least `need` bytes afterwards (what it held before is gone if it had to grow)
inline hipError_t cc_ws_ensure(cm_circ_chain_ws &w, int which, size_t need) {
    if (need == 0) need = 1;
    if (w.p[which] && w.bytes[which] >= need) return hipSuccess;
    if (w.p[which]) {
        (void)hipFree(w.p[which]);
        w.held -= w.bytes[which];
        w.p[which] = nullptr;
        w.bytes[which] = 0;
    }
    const hipError_t e = hipMalloc(&w.p[which], need);
    if (e != hipSuccess) {
        w.p[which] = nullptr;
        return e;
    }
    w.bytes[which] = need;
    w.held += need;
    ++w.allocations;
    return hipSuccess;
}
inline void cc_ws_drop(cm_circ_chain_ws &w, int which) {
    if (!w.p[which]) return;
    (void)hipFree(w.p[which]);
    w.held -= w.bytes[which];
    w.p[which] = nullptr;
    w.bytes[which] = 0;
}
// first error of the frees, hipSuccess if none
inline hipError_t cc_ws_release(cm_circ_chain_ws &w) {
    hipError_t first = hipSuccess;
    for (int i = 0; i < CCW_COUNT; ++i)
        if (w.p[i]) {
            const hipError_t e = hipFree(w.p[i]);
            if (e != hipSuccess && first == hipSuccess) first = e;
            w.p[i] = nullptr;
            w.bytes[i] = 0;
        }
    w.held = 0;
    w.max_workers = 0;
    return first;
}
