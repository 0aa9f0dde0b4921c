// cm_index_dev.h — DevList, an owner for the device allocations of a contig load.
//
// Not used by the library yet.  It belongs to the translation unit that is to hold the index loaders (NOTES 60:
// tests/diag/patches/index_unit.patch adds the unit, its interface below this type, and the loaders of cm_hot.hip on top of both);
// what is checked in ahead of it is the part that runs without a device: tests/diag/devlist_san_main.cpp, tests/test_index_build_cpu.py.
#ifndef CM_INDEX_DEV_H
#define CM_INDEX_DEV_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

// Where DevList's memory comes from: an expression that is 0 on success.  (tests/diag/devlist_san_main.cpp puts malloc / free
// here and takes DevList alone, for the host sanitizers.)
#ifndef CMIX_DEV_MALLOC
#include <hip/hip_runtime.h>
#define CMIX_DEV_MALLOC(pp, bytes) ((int)hipMalloc((pp), (bytes)))
#define CMIX_DEV_FREE(p) ((int)hipFree(p))
#endif

// Device allocations with one owner: what the list holds is freed when the list goes, unless another list took it first.
struct DevList {
    std::vector<void *> v;
    DevList() = default;
    DevList(const DevList &) = delete;
    DevList &operator=(const DevList &) = delete;
    ~DevList() { (void)release(); }
    // `bytes` of device memory at *p, owned by the list; the allocator's status (0: done), *p null on failure
    template <class T>
    int alloc(T **p, size_t bytes) {
        void *d = nullptr;
        v.reserve(v.size() + 1);                   // (an allocation that succeeded is never lost to a failing push_back; a load makes about 15)
        const int e = CMIX_DEV_MALLOC(&d, bytes);
        if (e == 0) v.push_back(d);
        else d = nullptr;
        *p = (T *)d;
        return e;
    }
    // everything freed, the list empty (a second call finds nothing to do); the first failing status
    int release() {
        int first = 0;
        for (void *p : v) {
            const int e = CMIX_DEV_FREE(p);
            if (e != 0 && first == 0) first = e;
        }
        v.clear();
        return first;
    }
    // hand-over: `from`'s allocations become this list's, `from` is left empty
    void take(DevList &from) {
        if (&from == this) return;
        v.insert(v.end(), from.v.begin(), from.v.end());
        from.v.clear();
    }
};

#endif /* CM_INDEX_DEV_H */
