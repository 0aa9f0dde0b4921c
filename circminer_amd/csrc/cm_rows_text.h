// cm_rows_text.h — what the device-side row formatters (cm_format_pam, cm_format_sam, cm_format_remain, cm_format_remain_sorted)
// share on the device: everything that is not a row format.
//
// Shared by the HIP kernels (cm_hot.hip: k_pam_len / k_sam_len / k_remain_len, k_pam_rows / k_sam_rows / k_remain_rows) and by the
// host emulation (tests/hostemu_rows.h) that g++ compiles, the way cm_fastq_text.h is shared.  The formats are cm_pam_text.h,
// cm_sam_text.h and cm_remain_text.h; each plugs into the plan below as a policy type.  The host side is written once as well:
// one driver in cm_hot.hip (RowsRun) runs the plan for the one or two files of a call -- a file is a length kernel, a span kernel,
// their Src and its buffers --, with a format's constants (PAIR_ITEMS .. ITEM_CHRS below) handed to it as values, and one loop
// (cm_row_ranges.h) takes a batch through any of the entry points in ranges.
// The plan of a call: one lane per item (a PAM row, a SAM record) computes the item's length (item_length) -> exclusive scan = the
// item's offset in the output -> a wave takes F::SPAN_ITEMS consecutive items, which are one contiguous span [s, e) of the output
// (format_span).  A span of at most WINDOW bytes is put together in the wave's LDS window, every byte at window_at() of its place
// in the output, and then streamed to global memory as whole aligned words (stream_span: single bytes only for the up to three
// bytes on either side, whose words a neighbouring wave shares -- the rule of cmft::copy_bases).  A larger span (long names, 250 -
// 300-bp reads) takes the direct path: the format's steps store to global memory themselves.
#ifndef CM_ROWS_TEXT_H
#define CM_ROWS_TEXT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CMRT_HD __host__ __device__ inline
#define CMRT_PLAN __host__ __device__ __forceinline__
#define CMRT_UNROLL _Pragma("unroll")            // the steps of a format are told apart at compile time
#else
#define CMRT_HD inline
#define CMRT_PLAN inline
#define CMRT_UNROLL
#endif

namespace cmrt {

constexpr uint32_t WAVE = 64;                        // lanes of a span: one wave, a workgroup of its own
// Bytes of a wave's LDS window.  8 KB per one-wave workgroup lets 20 waves share the 160 KB of a compute unit: 5 per SIMD where the
// registers would allow 8.  What fits: a PAM row of a mapped pair is its name + about 90 bytes (20 tabs and the line feed, four
// positions of up to 9 - 10 digits, two chromosome names, twelve short fields), so 64 rows with names of up to ~ 35 bytes; a SAM
// record of a 150-bp read is its name + 2 x 150 + about 60 - 90 bytes of numbers and tags, so 16 of them with names of up to ~ 60
// bytes.  A window that does not limit the waves (5 KB) would hold 64 rows of 80 bytes: shorter than a mapped PAM row with any
// name; 32 SAM records per wave would need 16 KB (10 waves per unit) for the same share of staged spans.
constexpr uint32_t WINDOW = 8192;
constexpr uint32_t WINDOW_WORDS = WINDOW / 4 + 1;    // the span lies in the window at its offset inside its first global word

// chromosome names on the device: name c is text[off[c] .. off[c + 1])
struct ChrTab {
    const uint8_t *text;
    const uint32_t *off;
    uint32_t n;
};

// Numbers are written into their place from the last digit backwards: the length is known beforehand (dec_len: compares, no
// division loop), so nothing is reversed, and every field of a PAM row and of a SAM record fits 32 bits.
// decimal digits of v
CMRT_HD uint32_t dec_len(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
CMRT_HD uint32_t int_len(int32_t v) { return v < 0 ? 1u + dec_len(0u - (uint32_t)v) : dec_len((uint32_t)v); }
// a chr_id outside [0, n) prints "-"
CMRT_HD uint32_t chr_len(const ChrTab &ct, int32_t id) { return (id >= 0 && (uint32_t)id < ct.n) ? ct.off[id + 1] - ct.off[id] : 1u; }

CMRT_HD uint8_t *put_u32(uint8_t *p, uint32_t v) {
    const uint32_t k = dec_len(v);
    for (uint32_t i = k; i-- > 0;) {
        p[i] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return p + k;
}
CMRT_HD uint8_t *put_i32(uint8_t *p, int32_t v) {
    if (v >= 0) return put_u32(p, (uint32_t)v);
    *p++ = '-';
    return put_u32(p, 0u - (uint32_t)v);
}
// The one field that does not fit 32 bits: the sort key of a remain record (cm_remain_text.h), a 64-bit signed decimal.
// decimal digits of v
CMRT_HD uint32_t dec_len64(uint64_t v) {
    if (v <= 0xffffffffull) return dec_len((uint32_t)v);
    uint32_t k = 10;
    for (uint64_t p = 10000000000ull; k < 20u && v >= p; p *= 10u) ++k;      // (p = 10^19 is the last power below 2^64)
    return k;
}
CMRT_HD uint32_t int_len64(int64_t v) { return v < 0 ? 1u + dec_len64(0ull - (uint64_t)v) : dec_len64((uint64_t)v); }
CMRT_HD uint8_t *put_u64(uint8_t *p, uint64_t v) {
    if (v <= 0xffffffffull) return put_u32(p, (uint32_t)v);
    const uint32_t k = dec_len64(v);
    for (uint32_t i = k; i-- > 0;) {
        p[i] = (uint8_t)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    }
    return p + k;
}
CMRT_HD uint8_t *put_i64(uint8_t *p, int64_t v) {
    if (v >= 0) return put_u64(p, (uint64_t)v);
    *p++ = '-';
    return put_u64(p, 0ull - (uint64_t)v);
}
CMRT_HD uint8_t *put_bytes(uint8_t *p, const uint8_t *from, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) p[i] = from[i];
    return p + n;
}
CMRT_HD uint8_t *put_chr(uint8_t *p, const ChrTab &ct, int32_t id) {
    if (id >= 0 && (uint32_t)id < ct.n) return put_bytes(p, ct.text + ct.off[id], ct.off[id + 1] - ct.off[id]);
    *p++ = '-';
    return p;
}
CMRT_HD uint8_t *put_lit(uint8_t *p, const char *s, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) p[i] = (uint8_t)s[i];
    return p + n;
}

// the span [s, e) of the output takes the LDS-staged path (window: WINDOW on the device; the emulation may ask for less)
CMRT_HD bool span_in_window(uint32_t s, uint32_t e, uint32_t window = WINDOW) { return e - s <= window; }
// where byte g of the output (s <= g < e) lies in the window of the span that starts at s: the window keeps the span at its
// offset inside the span's first global word, so that an aligned word of the output is an aligned word of the window
CMRT_HD uint32_t window_shift(uint32_t s) { return s & ~3u; }
CMRT_HD uint32_t window_at(uint32_t s, uint32_t g) { return g - window_shift(s); }
// Lane `lane` of `lanes` moves its share of the span [s, e) from the window to out (4-byte aligned, the output's byte 0): whole
// words as words, single bytes for the up to three bytes on either side of them.
CMRT_HD void stream_span(uint8_t *out, const uint8_t *win, uint32_t s, uint32_t e, uint32_t lane, uint32_t lanes) {
    const uint32_t w0 = (uint32_t)(((uint64_t)s + 3u) >> 2), w1 = e >> 2;       // the whole words [w0, w1)
    // (64-bit byte positions: a span may end within `lanes` bytes of 2^32)
    if (w0 >= w1) {
        for (uint64_t g = (uint64_t)s + lane; g < e; g += lanes) out[g] = win[window_at(s, (uint32_t)g)];
        return;
    }
    for (uint64_t g = (uint64_t)s + lane; g < 4ull * w0; g += lanes) out[g] = win[window_at(s, (uint32_t)g)];
    for (uint64_t g = 4ull * w1 + lane; g < e; g += lanes) out[g] = win[window_at(s, (uint32_t)g)];
    uint32_t *ow = (uint32_t *)out;
    const uint32_t *ww = (const uint32_t *)win;
    for (uint32_t w = w0 + lane; w < w1; w += lanes) ow[w] = ww[w - (s >> 2)];
}

// ---- the plan, written once ---------------------------------------------------------------------------------------------------
// A row format F is a struct of constants and static functions (cmpt::Format, cmst::Format):
//   PAIR_ITEMS, SPAN_ITEMS      items a pair makes; items of one span
//   PAIR_LIMIT                  a call takes fewer pairs than this (items and their count + 1 fit 32 bits)
//   ITEM_FIXED_MAX, ITEM_CHRS   what an item can take at most besides its name and its strings; chromosome names it prints
//   Src                         what the format reads of the resident batch
//   Scratch                     what a span's steps hand over to each other: the plan's caller allocates one per span
//   item_len(S, ct, first, q)   bytes of item q of the call (pair first + q / PAIR_ITEMS)
//   STEPS, step(i, dst, shift, scratch, S, ct, first, q0, n, off, lane)
//                               lane's share of step i of the span of items [q0, q0 + n): byte g of the output goes to
//                               dst[g - shift]; all lanes finish step i before any starts step i + 1
// and the plan is run by an executor Ex, which says what "every lane" and "finish" mean:
//   in_window(s, e, f) / in_output(s, e, f)   f(lane, dst) for the executor's lane(s), dst the window / the output
//   sync()                      all lanes have finished what was started
//   window()                    the window, to read;  first_lane(): true for one lane of the span
// The kernel's executor is a lane of a wave: f once, sync() = __syncthreads().  The emulation's runs every lane of a step, in a
// shuffled order, against shadow buffers that count the writes, and has nothing to wait for.

// the length pass: lane q of items + 1; item `items` is 0, the slot the scan leaves the total in
template <class F>
CMRT_PLAN void item_length(const typename F::Src &S, const ChrTab &ct, uint64_t first, uint32_t items, uint32_t q, uint32_t *len) {
    if (q > items) return;
    len[q] = q < items ? F::item_len(S, ct, first, q) : 0u;
}

// Span `span` of a call of `items` items with the scanned offsets off[0 .. items]: formatted in the window and streamed out as
// words, or, for a span larger than the window, stored by the steps themselves.  path[span] = 1 / 0 says which.
template <class F, class Ex>
CMRT_PLAN void format_span(Ex &ex, const typename F::Src &S, const ChrTab &ct, uint64_t first, uint32_t items, const uint32_t *off, uint32_t span, uint32_t window,
                           typename F::Scratch &scratch, uint8_t *path) {
    const uint32_t q0 = span * F::SPAN_ITEMS, q1 = items - q0 < F::SPAN_ITEMS ? items : q0 + F::SPAN_ITEMS, n = q1 - q0;
    const uint32_t s = off[q0], e = off[q1];
    const bool staged = span_in_window(s, e, window);                // (uniform)
    if (ex.first_lane()) path[span] = staged ? 1 : 0;
    if (staged) {
        const uint32_t shift = window_shift(s);
        CMRT_UNROLL
        for (uint32_t i = 0; i < F::STEPS; ++i) {
            if (i) ex.sync();
            ex.in_window(s, e, [&](uint32_t lane, uint8_t *win) { F::step(i, win, shift, scratch, S, ct, first, q0, n, off, lane); });
        }
        ex.sync();
        ex.in_output(s, e, [&](uint32_t lane, uint8_t *out) { stream_span(out, ex.window(), s, e, lane, WAVE); });
    } else {
        CMRT_UNROLL
        for (uint32_t i = 0; i < F::STEPS; ++i) {
            if (i) ex.sync();
            ex.in_output(s, e, [&](uint32_t lane, uint8_t *out) { F::step(i, out, 0u, scratch, S, ct, first, q0, n, off, lane); });
        }
    }
}

}  // namespace cmrt
#endif /* CM_ROWS_TEXT_H */
