// cm_fastq_text.h — the bodies of the device-side FASTQ tokeniser (cm_reads_stage_text).
//
// Shared by the HIP kernels (cm_hot.hip: k_ft_count, k_ft_lines, k_ft_records, k_ft_offsets, k_ft_copy, k_ft_finish) and by a
// host emulation (tests/hostemu_fastq.cpp) that g++ compiles, the way cm_index_build.h is shared.  The rules are those of
// build_side / next_plain in host_fastq.cpp:
//   * lines end at '\n' and nowhere else ('\r' is an ordinary byte); record i of a block is its lines 4 i .. 4 i + 3, records
//     are counted by line and never resynchronised on '@';
//   * a record is malformed if its header line is empty or does not start with '@', its third line is empty or does not start
//     with '+', or its quality line is not as long as its sequence line;
//   * header tokens are the runs of bytes other than ' ' behind the '@'; 23 of them are a carried MatchedRead.
// The text of a block lives in a 16-byte aligned array that is readable for TEXT_SLACK bytes past its end, so that every
// load is a whole aligned word; what lies beyond the block's length never reaches a result.
// The pipeline, per file: newlines per chunk of NL_CHUNK bytes -> exclusive scan -> line-start table (line j starts at ls[j]
// and ends, without its '\n', at ls[j + 1] - 1; ls[lines] is the end sentinel) -> per record the checks, the token count and
// the sequence length -> exclusive scan = off[] -> the bases copied word by word to their place in the read buffer.
#ifndef CM_FASTQ_TEXT_H
#define CM_FASTQ_TEXT_H

#include <stdint.h>
#include "circminer_hot.h"

#if defined(__HIPCC__)
#define CMFT_HD __host__ __device__ inline
#else
#define CMFT_HD inline
#endif

namespace cmft {

constexpr uint32_t LANE_BYTES = 16;                  // text bytes a lane looks at in one step of the newline passes
constexpr uint32_t NL_CHUNK = 64 * LANE_BYTES;       // bytes per newline count: one step of one wave
constexpr uint32_t TEXT_SLACK = 32;                  // readable bytes behind the text (whole 16-byte steps, the word after an unaligned one)
constexpr int COPY_LANES = 16;                       // lanes that move one record's bases
constexpr int CARRIED_TOKENS = 23;                   // FQCOMMENTCNT, src/fastq_parser.h:12
constexpr unsigned long long NO_BAD = ~0ull;

// verdict of one record; the first malformed record of a block is the smallest (record << 3 | verdict)
enum Bad { REC_OK = 0, BAD_HEADER = 1, BAD_PLUS = 2, BAD_QUAL = 3, BAD_CARRIED = 4 };
CMFT_HD unsigned long long bad_key(uint32_t record, uint32_t verdict) { return ((unsigned long long)record << 3) | verdict; }

// The words of the result block a stage leaves for the host (one small read-back).
enum Res {
    RES_BAD1 = 0, RES_BAD2 = 1,          // bad_key of the first malformed record of file 1 / 2 (NO_BAD: none)
    RES_MAX_LEN = 2,                     // longest read over both files
    RES_LINES1 = 3, RES_LINES2 = 4,      // lines of the block (a trailing line without '\n' counts at the end of input)
    RES_PAIRS = 5,                       // n = min(lines1 / 4, lines2 / 4, max_pairs)
    RES_BASES1 = 6, RES_BASES2 = 7,      // off1[n], off2[n]
    RES_USED1 = 8, RES_USED2 = 9,        // bytes consumed = start of the first record not staged
    RES_WORDS = 10
};

// 0x80 in every byte of w that equals '\n' (exact per byte: no carry crosses a byte)
CMFT_HD uint32_t nl_bytes(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
// bit b set: byte at + b of the text is a '\n' (b < 16, at a multiple of 16, bytes at or beyond len never count)
CMFT_HD uint32_t nl_mask16(const uint8_t *text, uint64_t at, uint64_t len) {
    if (at >= len) return 0;
    const uint32_t *w = (const uint32_t *)(text + at);
    uint32_t m = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t h = nl_bytes(w[k]);           // bits 7, 15, 23, 31 -> bits 0 .. 3
        m |= (((h >> 7) & 1u) | ((h >> 14) & 2u) | ((h >> 21) & 4u) | ((h >> 28) & 8u)) << (4 * k);
    }
    const uint64_t left = len - at;
    return left >= 16 ? m : (m & ((1u << (uint32_t)left) - 1u));
}
CMFT_HD uint32_t popcount16(uint32_t m) {
    m = (m & 0x5555u) + ((m >> 1) & 0x5555u);
    m = (m & 0x3333u) + ((m >> 2) & 0x3333u);
    m = (m & 0x0f0fu) + ((m >> 4) & 0x0f0fu);
    return (m & 0xffu) + (m >> 8);
}
// The line starts behind the newlines of one lane's 16 bytes: newline number `rank` (0-based, over the whole block) ends line
// `rank` and starts line rank + 1.  Entries beyond ls_cap (the table holds what 4 * max_pairs lines need) are not written.
CMFT_HD void put_line_starts(uint32_t mask, uint64_t at, uint32_t rank, uint32_t *ls, uint32_t ls_cap) {
    for (uint32_t b = 0; mask; ++b, mask >>= 1)
        if (mask & 1u) {
            ++rank;
            if (rank < ls_cap) ls[rank] = (uint32_t)(at + b + 1);
        }
}
// lines of a block with `newlines` line feeds: at the end of the input the bytes behind the last one are a line too
CMFT_HD uint32_t line_count(uint32_t newlines, bool trailing_line) { return newlines + (trailing_line ? 1u : 0u); }
CMFT_HD uint32_t pair_count(uint32_t lines1, uint32_t lines2, uint64_t max_pairs) {
    const uint32_t a1 = lines1 / 4, a2 = lines2 / 4, a = a1 < a2 ? a1 : a2;
    return (uint64_t)a < max_pairs ? a : (uint32_t)max_pairs;
}

// tokens of the header line p[0 .. len): runs of bytes other than ' ' behind the '@' (split_header, host_fastq.cpp)
CMFT_HD int header_tokens(const uint8_t *p, uint32_t len) {
    int nt = 0;
    bool in = false;
    for (uint32_t i = 1; i < len; ++i) {
        const bool tok = p[i] != ' ';
        nt += (tok && !in) ? 1 : 0;
        in = tok;
    }
    return nt;
}
// Record i of a block: its verdict and the length of its sequence line.  carried_matters: file 1 (a 23-token header there is
// a carried state, which the device path does not parse; nobody looks at file 2's tokens).
CMFT_HD uint32_t check_record(const uint8_t *text, const uint32_t *ls, uint32_t i, bool carried_matters, uint32_t *seq_len) {
    const uint32_t s0 = ls[4 * (uint64_t)i], s1 = ls[4 * (uint64_t)i + 1], s2 = ls[4 * (uint64_t)i + 2], s3 = ls[4 * (uint64_t)i + 3],
                   s4 = ls[4 * (uint64_t)i + 4];
    const uint32_t l1 = s1 - 1 - s0, l2 = s2 - 1 - s1, l3 = s3 - 1 - s2, l4 = s4 - 1 - s3;
    *seq_len = l2;
    if (l1 == 0 || text[s0] != '@') return BAD_HEADER;
    if (l3 == 0 || text[s2] != '+') return BAD_PLUS;
    if (l4 != l2) return BAD_QUAL;
    if (carried_matters && header_tokens(text + s0, l1) == CARRIED_TOKENS) return BAD_CARRIED;
    return REC_OK;
}

// bytes s .. s + 3 of a 4-byte aligned little-endian array whose word behind that of byte s is readable
CMFT_HD uint32_t load_unaligned32(const uint8_t *text, uint64_t s) {
    const uint32_t *w = (const uint32_t *)text;
    const uint64_t k = s >> 2;
    const uint32_t sh = (uint32_t)(s & 3u) * 8u;
    const uint32_t lo = w[k];
    if (sh == 0) return lo;
    return (lo >> sh) | (w[k + 1] << (32u - sh));
}
// Lane `lane` of `lanes` moves its share of text[s .. s + len) to dst[d .. d + len) (dst 4-byte aligned): whole destination
// words as words, each put together from two aligned words of the text, and single bytes only for the up to three bytes on
// either side of them -- a neighbouring record owns the rest of those words.
CMFT_HD void copy_bases(uint8_t *dst, uint64_t d, const uint8_t *text, uint32_t s, uint32_t len, int lane, int lanes) {
    const uint64_t d1 = d + len;
    const uint64_t w0 = (d + 3) >> 2, w1 = d1 >> 2;      // the whole words [w0, w1)
    if (w0 >= w1) {
        for (uint32_t j = (uint32_t)lane; j < len; j += (uint32_t)lanes) dst[d + j] = text[s + j];
        return;
    }
    const uint32_t head = (uint32_t)(4 * w0 - d), tail = (uint32_t)(d1 - 4 * w1);
    for (uint32_t j = (uint32_t)lane; j < head; j += (uint32_t)lanes) dst[d + j] = text[s + j];
    for (uint32_t j = (uint32_t)lane; j < tail; j += (uint32_t)lanes) dst[4 * w1 + j] = text[s + (uint32_t)(4 * w1 - d) + j];
    uint32_t *dw = (uint32_t *)dst;
    for (uint64_t w = w0 + (uint64_t)lane; w < w1; w += (uint64_t)lanes) dw[w] = load_unaligned32(text, (uint64_t)s + (4 * w - d));
}

// ---- the host's share, called by cm_reads_stage_text and by the emulation: the sizes a stage is planned by, its verdict ------------
// What the host knows before it has seen a line (bases <= bytes, a record >= 4 bytes).  trail[f]: the block's last line has no '\n'
// and counts (flag bit f: end of input); max_pairs: the caller's, capped at 2^30 (a block below 2^32 bytes holds fewer records); nb: no
// more pairs than this (off, rec and the lengths hold nb + 1 words per file); n_chunks[f] newline counts (+ 1: the total), ls_cap[f]
// line starts (what 4 max_pairs lines need); scan_items: the longest array the tokeniser's scans run over.
struct Sizes { uint32_t trail[2], nb, n_chunks[2], ls_cap[2]; uint64_t max_pairs, scan_items; };
// CM_EINVAL: text[*file] is null with a length; CM_ELIMIT: it is too long for 32-bit line starts (the sentinel behind a last line
// without '\n' is len + 1, a uint32 like every line start).  The files are looked at in order.
inline int plan_sizes(const uint8_t *const text[2], const uint64_t len[2], uint64_t max_pairs, uint32_t flags, Sizes *S, int *file) {
    S->max_pairs = max_pairs < (1ull << 30) ? max_pairs : 1ull << 30;
    const uint64_t shorter = (len[0] < len[1] ? len[0] : len[1]) / 4, ls_max = 4 * S->max_pairs + 1;
    S->nb = (uint32_t)(S->max_pairs < shorter ? S->max_pairs : shorter);
    S->scan_items = (uint64_t)S->nb + 1;
    for (int f = 0; f < 2; ++f) {
        *file = f;
        if (len[f] && !text[f]) return CM_EINVAL;
        S->trail[f] = ((flags >> f) & 1u) && len[f] && text[f][len[f] - 1] != '\n';
        if (len[f] > 0xffffffffull - S->trail[f]) return CM_ELIMIT;
        S->n_chunks[f] = (uint32_t)((len[f] + NL_CHUNK - 1) / NL_CHUNK);
        S->ls_cap[f] = (uint32_t)(len[f] + 2 < ls_max ? len[f] + 2 : ls_max);
        if ((uint64_t)S->n_chunks[f] + 1 > S->scan_items) S->scan_items = (uint64_t)S->n_chunks[f] + 1;
    }
    return CM_OK;
}
// floor(longest read / k) seeds are more than a build of the kernels takes: the one line every way a batch comes in refuses by
inline bool too_many_seeds(int max_len, int kmer, int max_seeds) { return max_len / kmer > max_seeds; }
// What the result block says about the batch: the verdicts of next_plain / build_side / check_reads, the first that applies.
// LINES_LEFT: file `file` ends (its flag bit) `count` lines behind its last whole record, within max_pairs; FILE2_SHORT: file 2
// ends (flag bit 1) before file 1; MALFORMED: record `record` of file `file` is `count` (a Bad; BAD_CARRIED in file 1 only, behind
// the other three of either file); READ_TOO_LONG, TOO_MANY_SEEDS: the longest read has `count` bases.
enum Case { ACCEPTED = 0, LINES_LEFT, FILE2_SHORT, MALFORMED, READ_TOO_LONG, TOO_MANY_SEEDS };
struct Verdict { int code; Case what; int file; unsigned long long record, count; };      // code: CM_OK, CM_EINVAL, CM_ELIMIT (TOO_MANY_SEEDS)
inline Verdict verdict(const unsigned long long *R, uint32_t flags, uint64_t max_pairs, int32_t max_read_len, int32_t kmer, int max_seeds) {
    const unsigned long long lines[2] = {R[RES_LINES1], R[RES_LINES2]}, max_len = R[RES_MAX_LEN];
    for (int f = 0; f < 2; ++f)
        if (((flags >> f) & 1u) && lines[f] % 4 != 0 && lines[f] / 4 < max_pairs) return {CM_EINVAL, LINES_LEFT, f, 0, lines[f] % 4};
    if ((flags & 2u) && lines[1] / 4 < (lines[0] / 4 < max_pairs ? lines[0] / 4 : max_pairs)) return {CM_EINVAL, FILE2_SHORT, 1, 0, 0};
    for (int f = 0; f < 2; ++f)
        if (R[RES_BAD1 + f] != NO_BAD && (R[RES_BAD1 + f] & 7u) != BAD_CARRIED) return {CM_EINVAL, MALFORMED, f, R[RES_BAD1 + f] >> 3, R[RES_BAD1 + f] & 7u};
    if (R[RES_BAD1] != NO_BAD) return {CM_EINVAL, MALFORMED, 0, R[RES_BAD1] >> 3, BAD_CARRIED};
    if (max_len > (unsigned long long)max_read_len) return {CM_EINVAL, READ_TOO_LONG, 0, 0, max_len};
    if (too_many_seeds((int)max_len, kmer, max_seeds)) return {CM_ELIMIT, TOO_MANY_SEEDS, 0, 0, max_len};
    return {CM_OK, ACCEPTED, 0, 0, 0};
}

}  // namespace cmft
#endif /* CM_FASTQ_TEXT_H */
