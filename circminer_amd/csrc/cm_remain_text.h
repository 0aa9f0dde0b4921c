// cm_remain_text.h — the remain-FASTQ record format of the device-side formatter (cm_format_remain).
//
// Shared by the HIP kernels (cm_hot.hip: k_remain_len, k_remain_rows) and by a host emulation (tests/hostemu_remain.cpp) that g++
// compiles, the way cm_fastq_text.h is shared.  The number formats, the window and the plan of a call are cm_rows_text.h's;
// Format<MATE> below is what this format plugs into that plan.  The rules are those of write_remain_rows in host_fastq.cpp
// (write_read_category of the reference):
//   * an item is the record of mate MATE of one SELECTED pair: item q of a call is pair sel[first + q], sel the ascending list of
//     the active pairs (the set of cm_collect_records).  One run of the plan per mate file: Format<0> makes <..>_remain_R1.fastq,
//     Format<1> _R2.fastq, from one Src;
//   * '@', the mate's kept name (R1's in file 1, R2's in file 2: the rule of cmpt::name_span, so a name ends at its first NUL
//     byte), the header fields -- the same in both files --, '\n', the bases as the read buffer holds them, "\n+\n", the kept
//     qualities, '\n';
//   * the header fields of a type of cmpt::mapped_type() are the 22 fields of the MatchedRead, each behind a space:
//     " %lld %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d" = gspos, type, chromosome, spos / epos / mlen / qspos /
//     qepos / strand / ed of R1, chromosome, the same of R2, tlen, junc_num, gm_compatible != 0, contig_num, with
//     gspos = (uint64)(int64)contig_num * CM_CONTIG_SIZE + (uint32)(spos_r1 + shift) printed SIGNED (sort_key), shift = start_pos of
//     chr_id inside [0, n_chr) and 0 outside, where the chromosome prints "-"; mlen_* through (int), junc_num a uint16;
//   * every other type prints the star form " * <type>" and 20 times " *"; its sort key is 0 (what `sort -k2,2n` makes of "*").
// A span is SPAN_RECS records.  Like a SAM record a remain record is mostly two byte strings, so a span has the same two steps:
// lane r < SPAN_RECS writes the ends of record r (format_ends: the header line, the three bytes between bases and qualities, the
// last line feed) and leaves a descriptor; then REC_LANES lanes per record move bases and qualities (cmst::put_field, never
// reversed), whole words as words.  Both steps write the window or, on the direct path, global memory.
// The sources are those of cm_sam_text.h: 4-byte aligned arrays, readable for a whole word past their last byte.
#ifndef CM_REMAIN_TEXT_H
#define CM_REMAIN_TEXT_H

#include <stdint.h>

#include "circminer_hot.h"
#include "cm_pam_text.h"
#include "cm_rows_text.h"
#include "cm_sam_text.h"

#define CMRM_HD CMRT_HD

namespace cmrm {

using namespace cmrt;

// Records of one span.  A record of a 150-bp read is '@' + name + header fields + 2 x 150 bases / qualities + 5 bytes of line ends
// and '+'; the fields of a mapped pair on a human-sized genome take about 115 bytes (22 spaces, gspos of 10 - 11 digits, four
// positions of 9 - 10, two chromosome names, 14 short fields), the star form 44 - 45.  So a record is about 420 bytes + its name,
// and 16 of them fit the 8-KB window with names of up to ~ 90 bytes: every ordinary span is staged.  32 such records are 13 KB
// before their names, so none of their spans would be; 8 would leave half the window unused for the same LDS per wave.  16 records
// of 250 - 300-bp reads (10 - 11.5 KB) and runs of long names take the direct path.  (cmst::SPAN_RECS is 16 for the same reason.)
constexpr uint32_t SPAN_RECS = 16;
constexpr uint32_t REC_LANES = WAVE / SPAN_RECS;     // lanes that move one record's bases and qualities
#define CMRM_STARS " * * * * * * * * * * * * * * * * * * * *"
constexpr uint32_t STARS_LEN = sizeof(CMRM_STARS) - 1u;      // the 20 fields behind the type of the star form
// what a record can take at most without its name, its two chromosome names and its two strings: '@', the header's line feed, 22
// spaces, gspos (20), eight "%u" of 10 digits, seven "%d" of 11 bytes, junc_num (5), gm_compatible, two strands, "\n+\n", '\n'
constexpr uint32_t REC_FIXED_MAX = 1 + 1 + 22 + 20 + 8 * 10 + 7 * 11 + 5 + 1 + 2 + 3 + 1;
static_assert(REC_FIXED_MAX >= 1 + 1 + 3 + 11 + STARS_LEN + 3 + 1, "the star form is the shorter one");

// where a chromosome starts in its contig (cm_chr_info.start_pos); 0 for a chr_id outside the table
CMRM_HD uint32_t shift_of(const uint32_t *chr_shift, uint32_t n_chr, int32_t id) { return (id >= 0 && (uint32_t)id < n_chr) ? chr_shift[id] : 0u; }
// the sort key of a mapped pair (chrloc2conloc of the reference), as the header prints it
CMRM_HD int64_t gspos_of(const cm_mapped_read &m, uint32_t shift) {
    return (int64_t)((uint64_t)(int64_t)m.contig_num * (uint64_t)CM_CONTIG_SIZE + (uint64_t)(uint32_t)(m.spos_r1 + shift));
}
// what `sort -k2,2n` orders record by: key_of in host_circ.cpp
CMRM_HD int64_t key_of(const cm_mapped_read &m, uint32_t shift) { return cmpt::mapped_type(m.type) ? gspos_of(m, shift) : 0; }

// bytes of the header fields of state m, from the space behind the name to the byte in front of the line feed
CMRM_HD uint32_t fields_len(const cm_mapped_read &m, uint32_t shift, const ChrTab &ct) {
    if (!cmpt::mapped_type(m.type)) return 3u + int_len(m.type) + STARS_LEN;
    return 22u + int_len64(gspos_of(m, shift)) + int_len(m.type) + 2u * chr_len(ct, m.chr_id) + dec_len(m.spos_r1) + dec_len(m.epos_r1) +
           int_len((int32_t)m.mlen_r1) + dec_len(m.qspos_r1) + dec_len(m.qepos_r1) + 1u + int_len(m.ed_r1) + dec_len(m.spos_r2) + dec_len(m.epos_r2) +
           int_len((int32_t)m.mlen_r2) + dec_len(m.qspos_r2) + dec_len(m.qepos_r2) + 1u + int_len(m.ed_r2) + int_len(m.tlen) + dec_len(m.junc_num) + 1u +
           int_len(m.contig_num);
}
// bytes of the record of a read of len bases behind a name of name_len bytes
CMRM_HD uint32_t item_len(const cm_mapped_read &m, uint32_t shift, uint32_t name_len, uint32_t len, const ChrTab &ct) {
    return 1u + name_len + fields_len(m, shift, ct) + 1u + len + 3u + len + 1u;
}

#define CMRM_SP(p) (*(p)++ = ' ')
// the header fields at p: exactly fields_len() bytes
CMRM_HD uint8_t *put_fields(uint8_t *p, const cm_mapped_read &m, uint32_t shift, const ChrTab &ct) {
    if (!cmpt::mapped_type(m.type)) {
        p = put_lit(p, " * ", 3);
        p = put_i32(p, m.type);
        return put_lit(p, CMRM_STARS, STARS_LEN);
    }
    CMRM_SP(p); p = put_i64(p, gspos_of(m, shift));
    CMRM_SP(p); p = put_i32(p, m.type);
    CMRM_SP(p); p = put_chr(p, ct, m.chr_id);
    CMRM_SP(p); p = put_u32(p, m.spos_r1);
    CMRM_SP(p); p = put_u32(p, m.epos_r1);
    CMRM_SP(p); p = put_i32(p, (int32_t)m.mlen_r1);
    CMRM_SP(p); p = put_u32(p, m.qspos_r1);
    CMRM_SP(p); p = put_u32(p, m.qepos_r1);
    CMRM_SP(p); *p++ = m.r1_forward ? '+' : '-';
    CMRM_SP(p); p = put_i32(p, m.ed_r1);
    CMRM_SP(p); p = put_chr(p, ct, m.chr_id);
    CMRM_SP(p); p = put_u32(p, m.spos_r2);
    CMRM_SP(p); p = put_u32(p, m.epos_r2);
    CMRM_SP(p); p = put_i32(p, (int32_t)m.mlen_r2);
    CMRM_SP(p); p = put_u32(p, m.qspos_r2);
    CMRM_SP(p); p = put_u32(p, m.qepos_r2);
    CMRM_SP(p); *p++ = m.r2_forward ? '+' : '-';
    CMRM_SP(p); p = put_i32(p, m.ed_r2);
    CMRM_SP(p); p = put_i32(p, m.tlen);
    CMRM_SP(p); p = put_u32(p, m.junc_num);
    CMRM_SP(p); *p++ = m.gm_compatible != 0 ? '1' : '0';
    CMRM_SP(p); p = put_i32(p, m.contig_num);
    return p;
}
#undef CMRM_SP

// the two strings of a record, as format_ends leaves them for copy_strings
struct Strings {
    uint64_t src;            // the read's offset in seq / qual
    uint32_t at;             // where the bases start in the destination; the qualities start at + len + 3
    uint32_t len;            // bytes of the read
};
// The ends of the record at dst[d ..): everything but the bases and the qualities.
CMRM_HD Strings format_ends(uint8_t *dst, uint64_t d, const cm_mapped_read &m, uint32_t shift, const uint8_t *name, uint32_t name_len, uint64_t src, uint32_t len,
                            const ChrTab &ct) {
    uint8_t *p = dst + d;
    *p++ = '@';
    p = put_bytes(p, name, name_len);
    p = put_fields(p, m, shift, ct);
    *p++ = '\n';
    Strings S;
    S.src = src;
    S.at = (uint32_t)(p - dst);
    S.len = len;
    p += len;
    p = put_lit(p, "\n+\n", 3);
    p += len;
    *p = '\n';
    return S;
}
// bases and qualities of the record S describes, into the dst format_ends wrote its ends to (word 0 of dst is a word of the
// output: see cmrt::window_at)
CMRM_HD void copy_strings(uint8_t *dst, const Strings &S, const uint8_t *seq, const uint8_t *qual, uint32_t lane, uint32_t lanes) {
    cmst::put_field(dst, S.at, S.len, seq, S.src, S.len, false, false, lane, lanes);
    cmst::put_field(dst, (uint64_t)S.at + S.len + 3u, S.len, qual, S.src, S.len, false, false, lane, lanes);
}

// What the format reads of the resident batch, for both mates: the selection list, the states, the kept names, the bases and the
// kept qualities, and the chromosome shifts (n_chr words, beside the names of the plan's chromosome table).  keys (nullable): where
// the run of mate 0 leaves key_of() of item q, at keys[q].
struct Src {
    const uint32_t *sel;
    const cm_mapped_read *state;
    const uint8_t *names[2];
    const uint32_t *name_off[2];
    const uint8_t *seq[2], *qual[2];
    const uint64_t *off[2];
    const uint32_t *chr_shift;
    int64_t *keys;
};

// the format as the plan of cm_rows_text.h takes it: the file of mate MATE (0: R1, 1: R2)
template <uint32_t MATE>
struct Format {
    static_assert(MATE < 2, "a pair has two mates");
    static constexpr uint32_t PAIR_ITEMS = 1, SPAN_ITEMS = SPAN_RECS, STEPS = 2;
    static constexpr uint64_t PAIR_LIMIT = 0xffffffffull;
    static constexpr uint32_t ITEM_FIXED_MAX = REC_FIXED_MAX, ITEM_CHRS = 2;
    using Src = cmrm::Src;
    struct Scratch {
        Strings desc[SPAN_RECS];
    };
    // item q of the call is the record of pair sel[first + q]
    static CMRT_PLAN uint32_t item_len(const Src &S, const ChrTab &ct, uint64_t first, uint32_t q) {
        const uint64_t pair = S.sel[first + q];
        const cm_mapped_read m = S.state[pair];
        return cmrm::item_len(m, shift_of(S.chr_shift, ct.n, m.chr_id), S.name_off[MATE][pair + 1] - S.name_off[MATE][pair],
                              (uint32_t)(S.off[MATE][pair + 1] - S.off[MATE][pair]), ct);
    }
    // step 0: the ends of the span's records (and their keys), a lane each; step 1: their strings
    static CMRT_PLAN void step(uint32_t i, uint8_t *dst, uint32_t shift, Scratch &sc, const Src &S, const ChrTab &ct, uint64_t first, uint32_t q0, uint32_t n,
                               const uint32_t *off, uint32_t lane) {
        if (i == 0) {
            if (lane >= n) return;
            const uint32_t q = q0 + lane;
            const uint64_t pair = S.sel[first + q];
            const cm_mapped_read m = S.state[pair];
            const uint32_t cs = shift_of(S.chr_shift, ct.n, m.chr_id), na = S.name_off[MATE][pair];
            const uint64_t a = S.off[MATE][pair];
            sc.desc[lane] = format_ends(dst, off[q] - shift, m, cs, S.names[MATE] + na, S.name_off[MATE][pair + 1] - na, a, (uint32_t)(S.off[MATE][pair + 1] - a), ct);
            if (MATE == 0 && S.keys) S.keys[q] = key_of(m, cs);
        } else {
            const uint32_t r = lane / REC_LANES;
            if (r >= n) return;
            copy_strings(dst, sc.desc[r], S.seq[MATE], S.qual[MATE], lane % REC_LANES, REC_LANES);
        }
    }
};

}  // namespace cmrm
#endif /* CM_REMAIN_TEXT_H */
