// row_ranges_san_main.cpp — format_ranges (circminer_amd/csrc/cm_row_ranges.h), the loop cm_mapping_run formats a batch's text
// with, over a formatter that only counts, as a program of its own, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc
//       tests/diag/row_ranges_san_main.cpp -o tests/_hostemu/row_ranges_san && tests/_hostemu/row_ranges_san
// The formatter knows the size of every record as a function of its index and reports sums: no byte is stored, so a file of 2^32
// bytes and more costs nothing, and the buffers are numbers (p stays null).  For one file and for two:
//   (a) a range whose bytes reach 2^32 is halved until it fits, down to one record, where the refusal is final;
//   (b) every record is formatted exactly once and in order across halvings and growths;
//   (c) a growth asks for what the loops of cm_mapping_run asked for before they were one, the expression written out below;
//   (d) a refusal that is neither of the two is passed through once, with no retry;
//   (e) an empty set of unknown size makes one call and ends, an empty set of known size makes none;
//   (f) a refusal that says nothing (a tie group above the cap) is told apart only for the first range.
// tests/test_row_ranges_cpu.py builds and runs it.  Prints "0 mismatches"; exit status 0.
#include <cstdio>
#include <functional>
#include <vector>

#include "cm_row_ranges.h"

static int g_bad = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);              \
            ++g_bad;                                                     \
        }                                                                \
    } while (0)

// the formatter's side and the caller's books
struct Fake {
    int files;
    uint64_t n;                                             // records of the set
    std::function<uint64_t(uint64_t, int)> size;            // bytes of record i in file m
    bool learn = false, append = true;                      // the size of the set is told by the first call; ranges are appended
    long fail_call = -1;                                    // this call (from 0) fails with fail_code, saying nothing
    int fail_code = CM_EHIP;
    RowBuf B[2];
    uint64_t total = 0, next = 0, bytes[2] = {0, 0};
    long calls = 0, halved = 0, grown = 0, taken_ranges = 0, refusals = 0, said_nothing = 0;
    uint64_t last_first = 0, last_c = 0, last_got[2] = {0, 0};

    // a call is for the range after the one that was served, or for the start of the one that was not
    int format(uint64_t first, uint64_t count, uint64_t got[2], uint64_t *tot) {
        const long call = calls++;
        if (learn) *tot = n;
        EXPECT(*tot == n && first <= n && (count == ~0ull || count <= n - first));
        EXPECT(first == next);                              // (b) no record skipped, none asked for again once it is done
        for (int m = 0; m < files; ++m) EXPECT(B[m].n == (append ? bytes[m] : 0));
        const uint64_t c = count == ~0ull ? n - first : count;
        last_first = first, last_c = c, last_got[0] = last_got[1] = 0;
        if (call == fail_call) return fail_code;
        bool over = false, small = false;
        for (int m = 0; m < files; ++m) {
            for (uint64_t i = first; i < first + c; ++i) got[m] += size(i, m);
            last_got[m] = got[m];
            over |= got[m] >= (1ull << 32);
            small |= got[m] > B[m].room();
        }
        if (over && c > 1) ++halved;
        if (over || small) return CM_ELIMIT;
        next = first + c;                                   // served: the bytes are in the buffers
        for (int m = 0; m < files; ++m) bytes[m] += got[m];
        return CM_OK;
    }
    int grow(RowBuf &b, uint64_t cap) {
        const int m = (int)(&b - B);
        ++grown;
        EXPECT(m >= 0 && m < files && last_got[m] > b.room() && last_got[m] < (1ull << 32));
        // (c) the parent's expression: what is held, the range, the records behind it at the range's bytes per record, 64 KB
        const uint64_t done = last_first, c = last_c, got = last_got[m];
        EXPECT(c && cap == b.n + got + got / c * (n - done - c) + (1u << 16));
        b.cap = cap;
        return CM_OK;
    }
    int taken(uint64_t c) {                                 // the caller takes the range away: the next one starts at byte 0 again
        ++taken_ranges;
        EXPECT(!append && c == last_c && next == last_first + c);
        for (int m = 0; m < files; ++m) {
            EXPECT(B[m].n == last_got[m]);
            B[m].n = 0;
        }
        return CM_OK;
    }
    int refused(int r, bool nothing) {
        ++refusals;
        said_nothing += nothing;
        return r;
    }
    int run(uint64_t step) {
        total = learn ? ~0ull : n;
        RowRanges back{[this](uint64_t f, uint64_t c, uint64_t got[2], uint64_t *t) { return format(f, c, got, t); }, [this](RowBuf &b, uint64_t cap) { return grow(b, cap); },
                       nullptr, [this](int r, bool nothing) { return refused(r, nothing); }};
        if (!append) back.appended = [this](uint64_t c) { return taken(c); };
        const int r = format_ranges(B, files, &total, step, back);
        for (int m = 0; m < files; ++m) EXPECT(B[m].n == (append ? bytes[m] : 0));
        return r;
    }
    uint64_t sum(int m) const {
        uint64_t s = 0;
        for (uint64_t i = 0; i < n; ++i) s += size(i, m);
        return s;
    }
};

static void scenarios(int files) {
    const int big = files - 1;                              // the file that decides: the only one, or the second of two
    {   // (a, b, c) records of half a gigabyte and a little: 37 -> 18 -> 9 -> 4 per range; the buffers start empty
        Fake f{files, 37, [&](uint64_t i, int m) { return m == big ? (1ull << 29) + 7 * i : 100 + i; }};
        f.learn = files == 2;
        EXPECT(f.run(~0ull) == CM_OK && f.next == 37 && f.total == 37);
        EXPECT(f.halved == 3 && f.grown >= files && f.refusals == 0);
        for (int m = 0; m < files; ++m) EXPECT(f.B[m].n == f.sum(m) && f.bytes[m] == f.sum(m) && f.B[m].cap >= f.B[m].n);
    }
    {   // (a) ... down to one record of 2^32 bytes: the refusal is final, nothing grows for it, the records before it are done
        Fake f{files, 9, [&](uint64_t i, int m) { return m == big && i == 6 ? 1ull << 32 : 1000; }};
        EXPECT(f.run(8) == CM_ELIMIT && f.refusals == 1 && f.said_nothing == 0 && f.next == 6 && f.last_first == 6 && f.last_c == 1);
        const long calls = f.calls;
        EXPECT(f.halved == 3 && calls == 7 && f.grown == files);   // [0, 8) -> [0, 4): grown, done; [4, 8) -> [4, 6) done; [6, 8) -> [6, 7): final
    }
    {   // (b, c) growth alone: ranges of 5 of 23 records whose sizes rise, so that the estimate of one growth falls short of the next
        Fake f{files, 23, [&](uint64_t i, int m) { return (m + 1) * 30000 * (1 + i / 5); }};
        f.B[0].cap = 1000;                                  // (too small from the first range; a second file starts at nothing)
        EXPECT(f.run(5) == CM_OK && f.next == 23 && f.halved == 0 && f.grown >= 2 * files && f.calls > 5);
        for (int m = 0; m < files; ++m) EXPECT(f.B[m].n == f.sum(m));
    }
    {   // (c) ranges taken away by the caller (the sorted records): every range starts at byte 0 of buffers sized beforehand
        Fake f{files, 40, [&](uint64_t i, int m) { return m == big ? (1ull << 28) + i : 64; }};
        f.append = false;
        for (int m = 0; m < files; ++m) f.B[m].cap = f.sum(m) + (1u << 16);
        EXPECT(f.run(~0ull) == CM_OK && f.next == 40 && f.halved == 2 && f.grown == 0 && f.taken_ranges == 4);
        for (int m = 0; m < files; ++m) EXPECT(f.bytes[m] == f.sum(m));
    }
    {   // (d) another failure, in the third call: passed through once, no call after it
        Fake f{files, 30, [](uint64_t, int) { return 50; }};
        f.fail_call = 2;
        for (int m = 0; m < files; ++m) f.B[m].cap = 1 << 20;
        EXPECT(f.run(7) == CM_EHIP && f.calls == 3 && f.refusals == 1 && f.said_nothing == 0 && f.next == 14 && f.grown == 0);
    }
    {   // (d) ... and a refusal for a limit that names no size, behind the first range, is that too
        Fake f{files, 30, [](uint64_t, int) { return 50; }};
        f.fail_call = 1, f.fail_code = CM_ELIMIT;
        for (int m = 0; m < files; ++m) f.B[m].cap = 1 << 20;
        EXPECT(f.run(7) == CM_ELIMIT && f.calls == 2 && f.refusals == 1 && f.said_nothing == 0 && f.next == 7);
    }
    {   // (f) the same refusal for the first range says nothing: the caller's fall-back, once
        Fake f{files, 30, [](uint64_t, int) { return 50; }};
        f.fail_call = 0, f.fail_code = CM_ELIMIT;
        EXPECT(f.run(~0ull) == CM_ELIMIT && f.calls == 1 && f.refusals == 1 && f.said_nothing == 1 && f.next == 0 && f.grown == 0);
    }
    {   // (f) ... and is no fall-back when the first range was halved and a later one is refused
        Fake f{files, 8, [&](uint64_t, int m) { return m == big ? 1ull << 30 : 10; }};
        f.append = false, f.fail_call = 2, f.fail_code = CM_ELIMIT;
        for (int m = 0; m < files; ++m) f.B[m].cap = 1ull << 33;
        EXPECT(f.run(~0ull) == CM_ELIMIT && f.halved == 2 && f.calls == 3 && f.refusals == 1 && f.said_nothing == 1);   // call 2 is still the first range: [0, 2)
        Fake g{files, 8, [&](uint64_t, int m) { return m == big ? 1ull << 30 : 10; }};
        g.append = false, g.fail_call = 3, g.fail_code = CM_ELIMIT;
        for (int m = 0; m < files; ++m) g.B[m].cap = 1ull << 33;
        EXPECT(g.run(~0ull) == CM_ELIMIT && g.calls == 4 && g.refusals == 1 && g.said_nothing == 0 && g.next == 2);      // call 3 is [2, 4)
    }
    {   // (e) an empty set: one call where the call tells the size, none where the size is known
        Fake f{files, 0, [](uint64_t, int) { return 1; }};
        f.learn = true;
        EXPECT(f.run(~0ull) == CM_OK && f.calls == 1 && f.total == 0 && f.grown == 0 && f.refusals == 0);
        Fake g{files, 0, [](uint64_t, int) { return 1; }};
        EXPECT(g.run(1 << 17) == CM_OK && g.calls == 0);
    }
}

int main() {
    scenarios(1);
    scenarios(2);
    printf("%d mismatches\n", g_bad);
    return g_bad != 0;
}
