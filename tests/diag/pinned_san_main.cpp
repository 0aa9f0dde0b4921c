// pinned_san_main.cpp — PinnedRanges (circminer_amd/csrc/cm_pinned_ranges.h), the owner of cm_mapping_run's page-locked host ranges,
// over a fake runtime that keeps its own set of live registrations, as a program of its own, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I circminer_amd/csrc
//       tests/diag/pinned_san_main.cpp -o tests/_hostemu/pinned_san && tests/_hostemu/pinned_san
// After every call: no two live registrations overlap, never more than 64, a covered range lies inside a live registration (unless
// the cap was reached or the fake refused), nothing live overlaps a released block, and after clear() nothing is live with every
// registration unregistered exactly once.  tests/test_index_build_cpu.py builds it plain.  Prints "0 mismatches"; exit status 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#include "cm_pinned_ranges.h"

static int g_bad = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);              \
            ++g_bad;                                                     \
        }                                                                \
    } while (0)

// the runtime's side: what is registered now, and how often it was asked
struct Fake {
    std::mutex mu;
    std::map<const char *, uint64_t> live;
    long n_reg = 0, n_unreg = 0, n_refused = 0;
    bool refuse_reg = false, fail_unreg = false;
    static int reg(void *u, void *p, uint64_t bytes) {
        Fake &f = *(Fake *)u;
        std::lock_guard<std::mutex> lk(f.mu);
        if (f.refuse_reg) return ++f.n_refused, 3;
        for (auto &e : f.live) EXPECT(!((const char *)p < e.first + e.second && (const char *)p + bytes > e.first));   // the runtime refuses an overlap
        EXPECT(p && bytes);
        f.live[(const char *)p] = bytes;
        ++f.n_reg;
        return 0;
    }
    static int unreg(void *u, void *p, const char **msg) {
        Fake &f = *(Fake *)u;
        std::lock_guard<std::mutex> lk(f.mu);
        EXPECT(f.live.erase((const char *)p) == 1);              // registered, and not unregistered before
        ++f.n_unreg;
        if (!f.fail_unreg) return 0;
        static char text[64];
        snprintf(text, sizeof text, "fake says no (%ld)", f.n_unreg);
        *msg = text;
        return 7;
    }
    bool overlaps(const void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &e : live)
            if ((const char *)p < e.first + e.second && (const char *)p + bytes > e.first) return true;
        return false;
    }
    bool holds(const void *p, uint64_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &e : live)
            if ((const char *)p >= e.first && (const char *)p + bytes <= e.first + e.second) return true;
        return false;
    }
    void check() {
        std::lock_guard<std::mutex> lk(mu);
        EXPECT(live.size() <= PinnedRanges::kMax);
        const char *end = nullptr;
        for (auto &e : live) {                                   // (sorted by address)
            EXPECT(!end || e.first >= end);
            end = e.first + e.second;
        }
    }
    size_t n_live() {
        std::lock_guard<std::mutex> lk(mu);
        return live.size();
    }
};

static void bind(PinnedRanges &P, Fake &F) {
    P.reg = Fake::reg;
    P.unreg = Fake::unreg;
    P.user = &F;
}
static void cover(PinnedRanges &P, Fake &F, const void *p, uint64_t bytes) {
    const bool full = F.n_live() >= PinnedRanges::kMax;
    P.cover(p, bytes);
    F.check();
    if (bytes && !full && !F.refuse_reg) EXPECT(F.holds(p, bytes));
}
static void release(PinnedRanges &P, Fake &F, const void *p, uint64_t bytes) {
    P.release(p, bytes);
    F.check();
    EXPECT(!F.overlaps(p, bytes));
}
static void clear(PinnedRanges &P, Fake &F) {
    P.clear();
    EXPECT(F.n_live() == 0 && F.n_unreg == F.n_reg);
}

// the parser's arrays: a block that has to grow is announced, freed and allocated anew; otherwise the pointer stays and more of it is used
struct Block {
    char *p = nullptr;
    uint64_t cap = 0;
    void need(PinnedRanges &P, Fake &F, uint64_t bytes) {
        if (bytes <= cap) return;
        if (p) release(P, F, p, cap);
        free(p);
        cap = bytes + bytes / 2;
        p = (char *)malloc(cap);
    }
};

static void generations() {
    Fake F;
    PinnedRanges P;
    bind(P, F);
    Block gen[4][4];
    for (int k = 0; k < 16; ++k) {                               // batch k in generation k & 3, sizes growing from batch to batch
        for (int j = 0; j < 4; ++j) {
            Block &b = gen[k & 3][j];
            const uint64_t bytes = (j < 2 ? 3000 : 400) + (uint64_t)k * (j < 2 ? 700 : 90);
            const char *before = b.p;
            b.need(P, F, bytes);
            cover(P, F, b.p, bytes);
            if (before == b.p) EXPECT(F.holds(b.p, bytes));      // pointer unchanged, bytes larger: one registration, from the block's start
        }
        EXPECT(F.n_live() == (size_t)(k < 4 ? 4 * (k + 1) : 16));
    }
    cover(P, F, gen[0][0].p, 10);                                // inside a live registration: no call
    const long n = F.n_reg;
    cover(P, F, gen[1][2].p + 8, 16);
    EXPECT(F.n_reg == n);
    cover(P, F, gen[1][2].p, 0);                                 // nothing to cover
    EXPECT(F.n_reg == n);
    for (auto &g : gen)
        for (Block &b : g) {
            release(P, F, b.p, b.cap);
            free(b.p);
        }
    EXPECT(F.n_live() == 0);
    clear(P, F);
}

static void text_blocks() {
    Fake F;
    PinnedRanges P;
    bind(P, F);
    const uint64_t cap = 1u << 20;
    char *buf = (char *)malloc(cap), *other = (char *)malloc(4096);
    uint64_t off = 300000;
    for (int k = 0; k < 12; ++k) {                               // a block = the unconsumed tail in head room + fresh bytes: the start moves
        const uint64_t len = 65536 + 1000 * k;
        cover(P, F, buf + off, len);
        EXPECT(F.n_live() == 1);                                 // widened to the union, never two
        off = k & 1 ? off + 30000 : off - 50000;
    }
    cover(P, F, buf, 100);                                       // apart from the rest: a second registration in the same block
    cover(P, F, other, 4096);
    EXPECT(F.n_live() == 3);
    release(P, F, buf, cap);                                     // one block, two registrations, released at once
    EXPECT(F.n_live() == 1 && F.holds(other, 4096));
    free(buf);
    clear(P, F);
    free(other);
}

static void past_the_cap() {
    Fake F;
    PinnedRanges P;
    bind(P, F);
    char *buf = (char *)malloc(70 * 256);
    for (int i = 0; i < 70; ++i) cover(P, F, buf + i * 256, 128);
    EXPECT(F.n_live() == 64 && F.n_reg == 64 && !F.overlaps(buf + 64 * 256, 6 * 256));
    cover(P, F, buf + 10 * 256, 64);                             // (held already)
    cover(P, F, buf + 3 * 256, 512);                             // two dropped, their union registered: 63 live
    EXPECT(F.n_live() == 63 && F.holds(buf + 3 * 256, 256 + 128));
    cover(P, F, buf + 69 * 256, 128);                            // room again
    EXPECT(F.n_live() == 64);
    clear(P, F);
    EXPECT(P.failed == 0);
    free(buf);
}

static void refusals() {
    char *buf = (char *)malloc(4096);
    {
        Fake F;
        PinnedRanges P;
        bind(P, F);
        F.refuse_reg = true;                                     // a refused registration: nothing recorded, no failure counted
        cover(P, F, buf, 1000);
        EXPECT(F.n_refused == 1 && F.n_live() == 0);
        release(P, F, buf, 4096);
        clear(P, F);
        EXPECT(F.n_unreg == 0 && P.failed == 0 && P.first_message.empty());
        F.refuse_reg = false;
        cover(P, F, buf, 1000);
        F.refuse_reg = true;                                     // refused after the overlapped one was dropped: that one is gone, as before
        cover(P, F, buf + 500, 1000);
        EXPECT(F.n_live() == 0 && F.n_unreg == 1);
        clear(P, F);
        EXPECT(F.n_unreg == 1 && P.failed == 0);
    }
    {
        Fake F;
        PinnedRanges P;
        bind(P, F);
        cover(P, F, buf, 1000);
        cover(P, F, buf + 2000, 1000);
        F.fail_unreg = true;                                     // a failed unregistration: entry gone, counted, first message kept
        P.release(buf, 1500);
        EXPECT(P.failed == 1 && P.first_message == "fake says no (1)" && F.n_unreg == 1);
        P.release(buf, 1500);                                    // (gone from the list: not asked again)
        EXPECT(F.n_unreg == 1);
        P.clear();
        EXPECT(P.failed == 2 && P.first_message == "fake says no (1)" && F.n_unreg == 2);
        P.clear();
        EXPECT(F.n_unreg == 2);
    }
    free(buf);
}

// the release hook's situation: the parser's thread announces blocks while the calling thread covers others
static void two_threads() {
    Fake F;
    PinnedRanges P;
    bind(P, F);
    const int n = 24, rounds = 400;
    char *buf = (char *)malloc(n * 1024);
    std::thread hook([&]() {
        for (int r = 0; r < rounds; ++r)
            for (int i = 0; i < n; ++i) {
                P.release(buf + i * 1024, 1024);
                F.check();
            }
    });
    for (int r = 0; r < rounds; ++r)
        for (int i = 0; i < n; ++i) {
            P.cover(buf + i * 1024 + (r & 3) * 100, 256 + (r & 7) * 64);
            F.check();
        }
    hook.join();
    for (int i = 0; i < n; i += 2) release(P, F, buf + i * 1024, 1024);
    EXPECT(F.n_live() <= (size_t)n / 2);
    clear(P, F);
    EXPECT(P.failed == 0);
    free(buf);
}

int main() {
    generations();
    text_blocks();
    past_the_cap();
    refusals();
    two_threads();
    printf("%d mismatches\n", g_bad);
    return g_bad ? 1 : 0;
}
