// The schedule a library issues, as text: force-included into a build of the library
//     CM_EXTRA_FLAGS="-include <this file>"  _build.build(tag="trace")
// it renames the HIP calls that order work (waits, records, host waits, memsets, copies, kernel launches) to wrappers that append one
// line each to the file named by CM_SCHED_TRACE (nothing is written when that is unset) and then make the call.  Streams, events
// and kernels (host-side function pointers) are numbered in order of first appearance, so two builds that issue the same schedule
// write the same file.  It touches no source, so it works on any commit: see sched_trace.py.
// Kernel arguments are logged too, one token each.  hipMalloc / hipFree are renamed as well, so that a word of an argument that
// points into a live device allocation is written as (allocation number, offset), which does not depend on the addresses of a run.
// An argument of up to 8 bytes is written as that value.  A larger one (a struct by value) as S<bytes>:<p>:<h>, p a hash of its
// words that point into allocations (with their offsets in the struct), h a hash of all of it -- h also covers padding bytes,
// which hold whatever the stack held: sched_trace.py --compare tells a difference in h alone apart from any other.
// Limits of the launch macro: the kernel needs at least one argument (an empty __VA_ARGS__ would leave a trailing comma), and
// `kernel`, `grid`, `block`, `lds`, `stream` and the arguments are evaluated twice, so they must be free of side effects.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <initializer_list>
#include <vector>

namespace sched_trace {
// one log per library: the inline function's statics are shared by every translation unit it is included into
struct Log {
    std::mutex m;
    FILE *f = nullptr;
    std::vector<const void *> streams, events, kernels;
    struct Alloc { uintptr_t base; size_t size; bool live; };
    std::vector<Alloc> allocs;
    // a word that points into a live allocation (its end included) -> 0xA... | allocation number << 40 | offset
    uint64_t norm(uint64_t w, bool &is_ptr) const {
        for (size_t i = allocs.size(); i-- > 0;)
            if (allocs[i].live && w >= allocs[i].base && w <= allocs[i].base + allocs[i].size) {
                is_ptr = true;
                return 0xA000000000000000ull | (uint64_t)i << 40 | (w - allocs[i].base);
            }
        return w;
    }
    uint64_t ptr(const void *p) const {
        bool is_ptr = false;
        const uint64_t n = norm((uint64_t)(uintptr_t)p, is_ptr);
        return is_ptr ? n : 0;          // 0: host memory (or null)
    }
    Log() {
        if (const char *p = getenv("CM_SCHED_TRACE")) f = fopen(p, "a");
    }
    static int id(std::vector<const void *> &v, const void *p) {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == p) return (int)i;
        v.push_back(p);
        return (int)v.size() - 1;
    }
    int s(hipStream_t p) { return id(streams, p); }
    int e(hipEvent_t p) { return id(events, p); }
    int k(const void *p) { return id(kernels, p); }
};
inline Log &log() {
    static Log l;
    return l;
}
#define SCHED_TRACE_LINE(...)                      \
    do {                                           \
        sched_trace::Log &l = sched_trace::log();  \
        if (l.f) {                                 \
            std::lock_guard<std::mutex> g(l.m);    \
            fprintf(l.f, __VA_ARGS__);             \
            fflush(l.f);                           \
        }                                          \
    } while (0)

inline hipError_t stream_wait_event(hipStream_t st, hipEvent_t ev, unsigned int flags = 0) {
    SCHED_TRACE_LINE("wait    s%d e%d\n", l.s(st), l.e(ev));
    return hipStreamWaitEvent(st, ev, flags);
}
inline hipError_t event_record(hipEvent_t ev, hipStream_t st = nullptr) {
    SCHED_TRACE_LINE("record  s%d e%d\n", l.s(st), l.e(ev));
    return hipEventRecord(ev, st);
}
inline hipError_t event_synchronize(hipEvent_t ev) {
    SCHED_TRACE_LINE("esync   e%d\n", l.e(ev));
    return hipEventSynchronize(ev);
}
inline hipError_t stream_synchronize(hipStream_t st) {
    SCHED_TRACE_LINE("ssync   s%d\n", l.s(st));
    return hipStreamSynchronize(st);
}
inline uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }
template <class T>
inline void arg(const Log &l, std::string &out, const T &a) {
    unsigned char buf[sizeof(T)];
    memcpy(buf, (const void *)&a, sizeof(T));
    uint64_t h = 0xcbf29ce484222325ull, hp = h, first = 0;
    size_t off = 0;
    for (; off + 8 <= sizeof(T); off += 8) {
        uint64_t w;
        memcpy(&w, buf + off, 8);
        bool is_ptr = false;
        const uint64_t n = l.norm(w, is_ptr);
        if (off == 0) first = n;
        h = mix(h, n);
        if (is_ptr) hp = mix(mix(hp, n), off);
    }
    for (; off < sizeof(T); ++off) first = first << 8 | buf[off], h = mix(h, buf[off]);
    char t[64];
    if (sizeof(T) <= 8) snprintf(t, sizeof t, " %llx", (unsigned long long)first);
    else snprintf(t, sizeof t, " S%zu:%llx:%llx", sizeof(T), (unsigned long long)hp, (unsigned long long)h);
    out += t;
}
template <class T>
inline hipError_t dev_malloc(T **p, size_t bytes) {
    const hipError_t e = hipMalloc((void **)p, bytes);
    Log &l = log();
    if (l.f && e == hipSuccess) {
        std::lock_guard<std::mutex> g(l.m);
        l.allocs.push_back({(uintptr_t)*p, bytes, true});
        fprintf(l.f, "malloc  a%zu %zu bytes\n", l.allocs.size() - 1, bytes);
    }
    return e;
}
inline hipError_t dev_free(void *p) {
    Log &l = log();
    if (l.f && p) {
        std::lock_guard<std::mutex> g(l.m);
        for (size_t i = l.allocs.size(); i-- > 0;)
            if (l.allocs[i].live && l.allocs[i].base == (uintptr_t)p) {
                l.allocs[i].live = false;
                fprintf(l.f, "free    a%zu\n", i);
                break;
            }
    }
    return hipFree(p);
}
inline hipError_t memset_async(void *dst, int value, size_t bytes, hipStream_t st = nullptr) {
    SCHED_TRACE_LINE("memset  s%d %zu bytes of %d at %llx\n", l.s(st), bytes, value, (unsigned long long)l.ptr(dst));
    return hipMemsetAsync(dst, value, bytes, st);
}
inline hipError_t memcpy_async(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st = nullptr) {
    SCHED_TRACE_LINE("memcpy  s%d %zu bytes kind %d to %llx from %llx\n", l.s(st), bytes, (int)kind, (unsigned long long)l.ptr(dst), (unsigned long long)l.ptr(src));
    return hipMemcpyAsync(dst, src, bytes, kind, st);
}
// (every argument converted to the type of the kernel's parameter first, as the launch itself does)
template <class... K, class... A>
inline void launch(void (*kernel)(K...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A &...a) {
    Log &l = log();
    if (!l.f) return;
    std::lock_guard<std::mutex> g(l.m);
    std::string args;
    (void)std::initializer_list<int>{(arg<K>(l, args, (K)a), 0)...};
    fprintf(l.f, "launch  s%d k%d grid %u %u %u block %u %u %u lds %zu args%s\n", l.s(st), l.k((const void *)kernel), grid.x, grid.y, grid.z, block.x, block.y, block.z, lds, args.c_str());
    fflush(l.f);
}
}  // namespace sched_trace

#define hipStreamWaitEvent(...) sched_trace::stream_wait_event(__VA_ARGS__)
#define hipEventRecord(...) sched_trace::event_record(__VA_ARGS__)
#define hipEventSynchronize(...) sched_trace::event_synchronize(__VA_ARGS__)
#define hipStreamSynchronize(...) sched_trace::stream_synchronize(__VA_ARGS__)
#define hipMemsetAsync(...) sched_trace::memset_async(__VA_ARGS__)
#define hipMemcpyAsync(...) sched_trace::memcpy_async(__VA_ARGS__)
#define hipMalloc(...) sched_trace::dev_malloc(__VA_ARGS__)
#define hipFree(...) sched_trace::dev_free(__VA_ARGS__)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...)                                         \
    do {                                                                                                  \
        sched_trace::launch((kernel), dim3(grid), dim3(block), (size_t)(lds), (stream), __VA_ARGS__); \
        hipLaunchKernelGGLInternal((kernel), (grid), (block), (lds), (stream), __VA_ARGS__);              \
    } while (0)
#endif
