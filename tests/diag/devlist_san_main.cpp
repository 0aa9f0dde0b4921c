// devlist_san_main.cpp — DevList (circminer_amd/csrc/cm_index_dev.h), the owner of a contig's device allocations, over malloc / free
// as a program of its own, for the host sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I circminer_amd/csrc \
//       tests/diag/devlist_san_main.cpp -o tests/_hostemu/devlist_san && tests/_hostemu/devlist_san
// A leak, a double free or a use of freed memory is the sanitizer's report; the program's own count of live blocks says the same
// without one (tests/test_index_build_cpu.py builds it plain).  Exit status 0 = every case as expected and no report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

static long g_live = 0, g_fail_at = -1, g_calls = 0;
static int san_malloc(void **p, size_t bytes) {
    if (g_calls++ == g_fail_at) return 2;                  // (the allocator's "out of memory")
    *p = malloc(bytes ? bytes : 1);
    memset(*p, 0xa5, bytes);
    ++g_live;
    return 0;
}
static int san_free(void *p) {
    if (p) --g_live;
    free(p);
    return 0;
}
#define CMIX_DEV_MALLOC(pp, bytes) san_malloc((pp), (bytes))
#define CMIX_DEV_FREE(p) san_free(p)
#include "cm_index_dev.h"

static int g_bad = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);              \
            ++g_bad;                                                     \
        }                                                                \
    } while (0)

// a load as the loaders of cm_index_dev.hip make one: three arrays for keeps, two temporaries; the `fail_at`-th allocation fails
static int load(DevList &keep, long fail_at) {
    g_calls = 0;
    g_fail_at = fail_at;
    DevList tmp;
    uint32_t *off = nullptr, *pos = nullptr, *scratch = nullptr;
    uint16_t *cks = nullptr;
    uint8_t *table = nullptr;
    if (keep.alloc(&off, 1024 * sizeof(uint32_t))) return -3;
    if (tmp.alloc(&table, 4096)) return -3;
    if (tmp.alloc(&scratch, 64 * sizeof(uint32_t))) return -3;
    if (keep.alloc(&cks, 100 * sizeof(uint16_t))) return -3;
    if (keep.alloc(&pos, 100 * sizeof(uint32_t))) return -3;
    off[1023] = pos[99] = scratch[63] = 1;                 // the last item of each is the list's to give
    cks[99] = table[4095] = 1;
    return 0;
}

int main() {
    {   // hand-over on success: the slot's list owns the arrays, the call's list nothing; the temporaries went with the call
        DevList slot;
        {
            DevList keep;
            EXPECT(load(keep, -1) == 0 && keep.v.size() == 3 && g_live == 3);
            slot.take(keep);
            EXPECT(keep.v.empty() && slot.v.size() == 3);
        }
        EXPECT(g_live == 3);
        memset(slot.v[0], 0, 1024 * sizeof(uint32_t));     // still the slot's
        {   // a second load into the same slot: the old arrays are released first, as reset_index does
            DevList keep;
            EXPECT(slot.release() == 0 && g_live == 0);
            EXPECT(load(keep, -1) == 0);
            slot.take(keep);
        }
        EXPECT(g_live == 3 && slot.v.size() == 3);
    }
    EXPECT(g_live == 0);
    for (long at = 0; at < 5; ++at) {   // scope exit on failure, at every allocation of the call
        {
            DevList keep;
            void *was = (void *)&keep;
            EXPECT(load(keep, at) == -3 && (void *)&keep == was);
            EXPECT(g_live == (long)keep.v.size());             // the temporaries are gone, what the call kept is listed ...
        }
        EXPECT(g_live == 0);                                   // ... and goes with the list
    }
    {   // a failed allocation leaves a null pointer and the list as it was
        DevList l;
        int *p = (int *)&l;
        g_calls = 0;
        g_fail_at = 0;
        EXPECT(l.alloc(&p, 16) == 2 && p == nullptr && l.v.empty());
    }
    {   // double release, release after a hand-over, an empty list, a hand-over of an empty list and into a filled one
        g_fail_at = -1;
        DevList a, b, none;
        char *p = nullptr;
        EXPECT(none.release() == 0 && none.release() == 0);
        EXPECT(a.alloc(&p, 0) == 0 && a.alloc(&p, 7) == 0 && b.alloc(&p, 9) == 0 && g_live == 3);
        b.take(a);
        b.take(none);
        b.take(b);                                             // (its own: nothing moves, nothing is lost)
        EXPECT(a.v.empty() && b.v.size() == 3 && a.release() == 0 && g_live == 3);
        EXPECT(b.release() == 0 && g_live == 0 && b.release() == 0 && g_live == 0);
        EXPECT(b.alloc(&p, 5) == 0 && g_live == 1);            // a released list is a fresh one
    }
    EXPECT(g_live == 0);
    printf("devlist: %d mismatches, %ld blocks live\n", g_bad, g_live);
    return g_bad == 0 && g_live == 0 ? 0 : 1;
}
