// cm_row_ranges.h — format_ranges: the loop cm_mapping_run gets a batch's text out of a device formatter with (cm_format_pam / _sam /
// _remain / _remain_sorted).  A formatter takes records [first, first + count) and a buffer per file, and refuses (CM_ELIMIT) with
// the bytes it would need where a file of the range would reach 2^32 bytes (its offsets are 32 bits) or does not fit its buffer.
// The back end is passed in: the library's is the entry points and cm_host_alloc, tests/diag/row_ranges_san_main.cpp's only counts.
#ifndef CM_ROW_RANGES_H
#define CM_ROW_RANGES_H

#include <algorithm>
#include <functional>
#include "circminer_hot.h"

struct RowBuf {                                                        // the text of one file: n bytes of cap, page-locked
    void *p = nullptr;
    uint64_t cap = 0, n = 0;
    char *tail() const { return p ? (char *)p + n : nullptr; }         // where the next range goes
    uint64_t room() const { return cap - n; }
};
struct RowRanges {
    // got[m]: file m's bytes (those it needs, when refused for a size).  *total == ~0: the number of records is not known; the call
    // is asked for count ~0, "to the end", and sets it: an empty set costs one call (one of a known size: none)
    std::function<int(uint64_t first, uint64_t count, uint64_t got[2], uint64_t *total)> format;
    std::function<int(RowBuf &, uint64_t cap)> grow;                   // room for cap bytes, what the buffer holds kept
    std::function<int(uint64_t c)> appended;    // (may be empty) a range of c records is behind what B held; a caller that takes it away resets n
    // ends the loop on a failure it has no answer to; nothing_said: CM_ELIMIT without byte counts for the first range (a tie group)
    std::function<int(int status, bool nothing_said)> refused;
};
// Records [0, *total) into the `files` (1 or 2) buffers B, in ranges of at most `step` records (~0: all in one).  A range a file of which would reach 2^32 bytes is
// halved, down to one record, where the refusal is final; a buffer too small grows to what it holds + the range + the records behind it at the range's bytes per record + 64 KB.
inline int format_ranges(RowBuf *B, int files, uint64_t *total, uint64_t step, const RowRanges &back) {
    for (uint64_t done = 0; *total == ~0ull || done < *total;) {
        const uint64_t count = *total == ~0ull ? ~0ull : std::min(step, *total - done);
        uint64_t got[2] = {0, 0};
        int r = back.format(done, count, got, total);
        const uint64_t c = count == ~0ull ? *total - done : count, most = std::max(got[0], got[1]);
        if (r == CM_ELIMIT && most >= (1ull << 32) && c > 1) {
            step = c / 2;
            continue;
        }
        bool grown = false;
        for (int m = 0; m < files && r == CM_ELIMIT && c && most < (1ull << 32); ++m) {     // (no buffer helps a record of 2^32 bytes)
            if (got[m] <= B[m].room()) continue;
            if (int g = back.grow(B[m], B[m].n + got[m] + got[m] / c * (*total - done - c) + (1u << 16))) return g;
            grown = true;
        }
        if (grown) continue;
        if (r != CM_OK) return back.refused(r, r == CM_ELIMIT && most == 0 && done == 0);
        for (int m = 0; m < files; ++m) B[m].n += got[m];
        if (back.appended && (r = back.appended(c)) != CM_OK) return r;
        done += c;
    }
    return CM_OK;
}
#endif /* CM_ROW_RANGES_H */
