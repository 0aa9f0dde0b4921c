// cm_pam_text.h — the bodies of the device-side PAM formatter (cm_format_pam) and of the names cm_reads_stage_text keeps for it.
//
// Shared by the HIP kernels (cm_hot.hip: k_ft_name_len, k_ft_name_copy, k_pam_len, k_pam_rows) and by a host emulation
// (tests/hostemu_pam.cpp) that g++ compiles, the way cm_fastq_text.h is shared.  The rules are those of pam_row / name_len /
// split_header in host_fastq.cpp:
//   * the name of a pair is token 0 of its R1 header line (tokens: runs of bytes other than ' ' behind the '@'), without a
//     trailing "/x", up to its first NUL byte (cm_write_pam prints names with strlen); a header without a token has an empty name;
//   * a row is the name and 20 tab-separated fields of the state ("%u" / "%d" as pam_row prints them) for a type of mapped_type(),
//     and the name, 21 "*" fields and the type for every other type; a chr_id outside [0, n_chr) prints "-".
// The plan of a call: one lane per pair computes the row's length (row_len) -> exclusive scan = the row's offset in the output ->
// a wave takes SPAN_ROWS consecutive rows, which are one contiguous span [s, e) of the output.  A span of at most WINDOW bytes is
// formatted into the wave's LDS window (format_row, every lane its own row, at the row's offset inside the span) and then streamed
// to global memory as whole aligned words (stream_span: single bytes only for the up to three bytes on either side, whose words a
// neighbouring wave shares -- the rule of cmft::copy_bases).  A larger span (long names) takes the direct path: every lane
// stores its row's bytes itself.  Numbers are written into their place from the last digit backwards: the length is known
// beforehand (dec_len: compares, no division loop), so nothing is reversed, and every field fits 32 bits.
#ifndef CM_PAM_TEXT_H
#define CM_PAM_TEXT_H

#include <stdint.h>

#include "circminer_hot.h"

#if defined(__HIPCC__)
#define CMPT_HD __host__ __device__ inline
#else
#define CMPT_HD inline
#endif

namespace cmpt {

constexpr uint32_t SPAN_ROWS = 64;                   // rows of one span: the lanes of a wave
// Bytes of a wave's LDS window.  A row of a mapped pair is its name + about 90 bytes (20 tabs and the line feed, four positions
// of up to 9 - 10 digits, two chromosome names, twelve short fields), so 64 rows with names of up to ~ 35 bytes fit.  8 KB per
// one-wave workgroup lets 20 waves share the 160 KB of a compute unit: 5 per SIMD where the registers would allow 8.  A window
// that does not limit the waves (5 KB) would hold 64 rows of 80 bytes: shorter than a mapped row with any name.
constexpr uint32_t WINDOW = 8192;
constexpr uint32_t WINDOW_WORDS = WINDOW / 4 + 1;    // the span lies in the window at its offset inside its first global word
constexpr uint32_t UNMAPPED_STARS = 21;
// what a row can take at most without its name and its two chromosome names: 20 tabs and the line feed, eight "%u" of 10 digits,
// six "%d" of 11 bytes, junc_num, gm_compatible, two strands
constexpr uint32_t ROW_FIXED_MAX = 21 + 8 * 10 + 6 * 11 + 5 + 1 + 2;

// chromosome names on the device: name c is text[off[c] .. off[c + 1])
struct ChrTab {
    const uint8_t *text;
    const uint32_t *off;
    uint32_t n;
};

CMPT_HD bool mapped_type(int32_t t) {
    return t == CM_CONCRD || t == CM_DISCRD || t == CM_CHIORF || t == CM_CHIBSJ || t == CM_CHI2BSJ || t == CM_CONGNM || t == CM_CONGEN;
}

// The name inside the header line p[0 .. len) (p[0] is the '@'): where it starts and how long it is.
CMPT_HD void name_span(const uint8_t *p, uint32_t len, uint32_t *start, uint32_t *name_len) {
    uint32_t i = 1;
    while (i < len && p[i] == ' ') ++i;
    uint32_t j = i;
    while (j < len && p[j] != ' ') ++j;
    uint32_t l = j > i ? j - i : 0u;
    if (l >= 2 && p[i + l - 2] == '/') l -= 2;
    for (uint32_t k = 0; k < l; ++k)
        if (p[i + k] == 0) {
            l = k;
            break;
        }
    *start = l ? i : 0u;
    *name_len = l;
}

// decimal digits of v
CMPT_HD uint32_t dec_len(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
CMPT_HD uint32_t int_len(int32_t v) { return v < 0 ? 1u + dec_len(0u - (uint32_t)v) : dec_len((uint32_t)v); }
CMPT_HD uint32_t chr_len(const ChrTab &ct, int32_t id) { return (id >= 0 && (uint32_t)id < ct.n) ? ct.off[id + 1] - ct.off[id] : 1u; }

// bytes of the row of state m behind a name of name_len bytes
CMPT_HD uint32_t row_len(const cm_mapped_read &m, uint32_t name_len, const ChrTab &ct) {
    if (!mapped_type(m.type)) return name_len + 2u * UNMAPPED_STARS + 1u + int_len(m.type) + 1u;
    return name_len + 21u + 2u * chr_len(ct, m.chr_id) + dec_len(m.spos_r1) + dec_len(m.epos_r1) + int_len((int32_t)m.mlen_r1) + dec_len(m.qspos_r1) +
           dec_len(m.qepos_r1) + 1u + int_len(m.ed_r1) + dec_len(m.spos_r2) + dec_len(m.epos_r2) + int_len((int32_t)m.mlen_r2) + dec_len(m.qspos_r2) +
           dec_len(m.qepos_r2) + 1u + int_len(m.ed_r2) + int_len(m.tlen) + dec_len(m.junc_num) + 1u + int_len(m.type);
}

CMPT_HD uint8_t *put_u32(uint8_t *p, uint32_t v) {
    const uint32_t k = dec_len(v);
    for (uint32_t i = k; i-- > 0;) {
        p[i] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return p + k;
}
CMPT_HD uint8_t *put_i32(uint8_t *p, int32_t v) {
    if (v >= 0) return put_u32(p, (uint32_t)v);
    *p++ = '-';
    return put_u32(p, 0u - (uint32_t)v);
}
CMPT_HD uint8_t *put_bytes(uint8_t *p, const uint8_t *from, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) p[i] = from[i];
    return p + n;
}
CMPT_HD uint8_t *put_chr(uint8_t *p, const ChrTab &ct, int32_t id) {
    if (id >= 0 && (uint32_t)id < ct.n) return put_bytes(p, ct.text + ct.off[id], ct.off[id + 1] - ct.off[id]);
    *p++ = '-';
    return p;
}
#define CMPT_TAB(p) (*(p)++ = '\t')
// the row of state m at dst: exactly row_len() bytes
CMPT_HD void format_row(uint8_t *dst, const cm_mapped_read &m, const uint8_t *name, uint32_t name_len, const ChrTab &ct) {
    uint8_t *p = put_bytes(dst, name, name_len);
    if (!mapped_type(m.type)) {
        for (uint32_t i = 0; i < UNMAPPED_STARS; ++i) {
            CMPT_TAB(p);
            *p++ = '*';
        }
        CMPT_TAB(p);
        p = put_i32(p, m.type);
        *p = '\n';
        return;
    }
    CMPT_TAB(p); p = put_chr(p, ct, m.chr_id);
    CMPT_TAB(p); p = put_u32(p, m.spos_r1);
    CMPT_TAB(p); p = put_u32(p, m.epos_r1);
    CMPT_TAB(p); p = put_i32(p, (int32_t)m.mlen_r1);
    CMPT_TAB(p); p = put_u32(p, m.qspos_r1);
    CMPT_TAB(p); p = put_u32(p, m.qepos_r1);
    CMPT_TAB(p); *p++ = m.r1_forward ? '+' : '-';
    CMPT_TAB(p); p = put_i32(p, m.ed_r1);
    CMPT_TAB(p); p = put_chr(p, ct, m.chr_id);
    CMPT_TAB(p); p = put_u32(p, m.spos_r2);
    CMPT_TAB(p); p = put_u32(p, m.epos_r2);
    CMPT_TAB(p); p = put_i32(p, (int32_t)m.mlen_r2);
    CMPT_TAB(p); p = put_u32(p, m.qspos_r2);
    CMPT_TAB(p); p = put_u32(p, m.qepos_r2);
    CMPT_TAB(p); *p++ = m.r2_forward ? '+' : '-';
    CMPT_TAB(p); p = put_i32(p, m.ed_r2);
    CMPT_TAB(p); p = put_i32(p, m.tlen);
    CMPT_TAB(p); p = put_u32(p, m.junc_num);
    CMPT_TAB(p); *p++ = m.gm_compatible != 0 ? '1' : '0';
    CMPT_TAB(p); p = put_i32(p, m.type);
    *p = '\n';
}
#undef CMPT_TAB

// the span [s, e) of the output takes the LDS-staged path
CMPT_HD bool span_in_window(uint32_t s, uint32_t e) { return e - s <= WINDOW; }
// where byte g of the output (s <= g < e) lies in the window of the span that starts at s: the window keeps the span at its
// offset inside the span's first global word, so that an aligned word of the output is an aligned word of the window
CMPT_HD uint32_t window_at(uint32_t s, uint32_t g) { return g - (s & ~3u); }
// Lane `lane` of `lanes` moves its share of the span [s, e) from the window to out (4-byte aligned, the output's byte 0): whole
// words as words, single bytes for the up to three bytes on either side of them.
CMPT_HD void stream_span(uint8_t *out, const uint8_t *win, uint32_t s, uint32_t e, uint32_t lane, uint32_t lanes) {
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

}  // namespace cmpt
#endif /* CM_PAM_TEXT_H */
