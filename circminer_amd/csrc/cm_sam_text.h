// cm_sam_text.h — the SAM record format of the device-side formatter (cm_format_sam).
//
// Shared by the HIP kernels (cm_hot.hip: k_sam_len, k_sam_rows) and by a host emulation (tests/hostemu_sam.cpp) that g++ compiles,
// the way cm_fastq_text.h is shared.  The number formats, the chromosome table, the window and the plan of a call are
// cm_rows_text.h's; Format below is what this format plugs into that plan.  The rules are those of cm_write_sam, sam_flag and
// comp_of in host_fastq.cpp:
//   * a pair makes two records, mate 1 then mate 2 ("items" 2 p and 2 p + 1 of a call); QNAME of both is the kept R1 name;
//   * a pair is mapped for type <= CM_CHIORF || type == CM_CONGEN || type == CM_CONGNM (signed: negative types are mapped; this is
//     not cmpt::mapped_type); any other pair has RUNMAP | MUNMAP in both flags, RNAME "*", POS 0, RNEXT "*", PNEXT 0, TLEN 0 and
//     the tags NM / JC / TC 0;
//   * a mapped record: RNAME is the chromosome name ("-" for a chr_id outside the table), RNEXT "=", POS / PNEXT are spos_r1 /
//     spos_r2 crosswise, TLEN is +tlen for the mate with the smaller spos (strict spos_r1 < spos_r2 gives it to mate 1, anything
//     else to mate 2) and -tlen for the other, printed as "%u" of the int32.  The negation is done in unsigned arithmetic
//     (0u - (uint32_t)tlen): for tlen == INT_MIN both mates print 2147483648 here, where the host's `tlen * -1` is signed
//     overflow -- the one value of the field the byte-for-byte tests leave out;
//   * MAPQ and CIGAR are the literal "255\t*"; the tags are AT:i:type, NM:i:ed of the mate, JC:i:junc_num, TC:i:(gm_compatible != 0);
//   * a record with RREVER prints the reverse complement: the complement maps ACGTNacgtn to TGCANTGCAN and every other byte to
//     NUL, and SEQ ends in front of the first NUL ("%s"), i.e. at the first byte, counted from the read's end, that is outside
//     the ten (rc_cut); QUAL is reversed at full length.  Every other record prints SEQ and QUAL raw, NUL bytes included.
// The length of a record (item_len): only a record with RREVER looks at its read, from the end, a word at a time.  A span is
// SPAN_RECS records.  A record is mostly two byte strings, so the work of a span is split by kind into two steps:
// lane r < SPAN_RECS writes the "ends" of record r -- the name and the numbers in front of SEQ, the tab between SEQ and
// QUAL, the tags behind QUAL (format_ends) -- and leaves a descriptor of the two strings (Strings); then REC_LANES lanes per
// record, all 64 together, move SEQ and QUAL (copy_strings): whole destination words as words, each put together from two
// aligned words of the source (reversed: byte-swapped, SEQ complemented by compares), single bytes only for the up to three bytes
// on either side of a field, whose words the neighbouring field shares.  Both steps write the window or, on the direct path,
// global memory, by the same split.
// The sources: bases and qualities of read i are seq[off[i] .. off[i + 1]) / qual[off[i] .. off[i + 1]) of 4-byte aligned arrays
// that are readable for a whole word past their last byte.
#ifndef CM_SAM_TEXT_H
#define CM_SAM_TEXT_H

#include <stdint.h>

#include "circminer_hot.h"
#include "cm_fastq_text.h"
#include "cm_rows_text.h"

#define CMST_HD CMRT_HD

namespace cmst {

using namespace cmrt;

constexpr uint32_t SPAN_RECS = 16;                   // records of one span (8 pairs)
constexpr uint32_t REC_LANES = WAVE / SPAN_RECS;     // lanes that move one record's SEQ and QUAL
// what a record can take at most without its name, its chromosome name and its two strings: 14 tabs and the line feed, FLAG (3),
// POS / PNEXT / TLEN (10 each), "255", "*", RNEXT (1), four tags of 5 bytes with 11 + 11 + 5 + 1 bytes of numbers
constexpr uint32_t REC_FIXED_MAX = 15 + 3 + 30 + 3 + 1 + 1 + 20 + 28;

enum Flag : uint32_t { PAIRED = 1u << 0, PROPER = 1u << 1, RUNMAP = 1u << 2, MUNMAP = 1u << 3, RREVER = 1u << 4, MREVER = 1u << 5, FIPAIR = 1u << 6, SIPAIR = 1u << 7 };

CMST_HD bool mapped_type(int32_t t) { return t <= CM_CHIORF || t == CM_CONGEN || t == CM_CONGNM; }
// FLAG of mate `mate` (0: R1, 1: R2)
CMST_HD uint32_t flag_of(const cm_mapped_read &m, uint32_t mate) {
    uint32_t f = PAIRED | (mate ? SIPAIR : FIPAIR);
    if (m.type == CM_CONCRD) f |= PROPER;
    if (!mapped_type(m.type)) return f | RUNMAP | MUNMAP;
    if (!(mate ? m.r2_forward : m.r1_forward)) f |= RREVER;
    if (!(mate ? m.r1_forward : m.r2_forward)) f |= MREVER;
    return f;
}
// the complement of a base; 0 for a byte outside ACGTNacgtn (b & 0xDF is 'A' for 'A' and 'a' only, and so on)
CMST_HD uint32_t comp(uint32_t b) {
    const uint32_t u = b & 0xdfu;
    return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : u == 'N' ? 'N' : 0u;
}
CMST_HD uint32_t comp4(uint32_t w) { return comp(w & 0xffu) | comp((w >> 8) & 0xffu) << 8 | comp((w >> 16) & 0xffu) << 16 | comp(w >> 24) << 24; }
CMST_HD uint32_t bswap(uint32_t w) { return w << 24 | (w & 0xff00u) << 8 | (w >> 8 & 0xff00u) | w >> 24; }
// bytes j .. j + 3 of a field over the read src[s .. s + len) (j + 4 <= len): the read's bytes, or those of the reversed read,
// complemented for cmp
CMST_HD uint32_t field_word(const uint8_t *src, uint64_t s, uint32_t len, uint32_t j, bool rev, bool cmp) {
    if (!rev) return cmft::load_unaligned32(src, s + j);
    const uint32_t w = bswap(cmft::load_unaligned32(src, s + (len - 4u - j)));
    return cmp ? comp4(w) : w;
}
CMST_HD uint8_t field_byte(const uint8_t *src, uint64_t s, uint32_t len, uint32_t j, bool rev, bool cmp) {
    if (!rev) return src[s + j];
    const uint8_t b = src[s + (len - 1u - j)];
    return cmp ? (uint8_t)comp(b) : b;
}
// bytes of SEQ of a reversed record: the bytes in front of the first one, counted from the read's end, that has no complement
CMST_HD uint32_t rc_cut(const uint8_t *seq, uint64_t s, uint32_t len) {
    uint32_t x = 0;
    for (; x + 4u <= len; x += 4u) {
        const uint32_t w = comp4(field_word(seq, s, len, x, true, false));
        if ((w & 0xffu) == 0) return x;
        if ((w & 0xff00u) == 0) return x + 1u;
        if ((w & 0xff0000u) == 0) return x + 2u;
        if ((w >> 24) == 0) return x + 3u;
    }
    for (; x < len; ++x)
        if (comp(seq[s + (len - 1u - x)]) == 0) return x;
    return len;
}

// the printed numbers of a record
struct Fields {
    uint32_t flag, pos, pnext, tlen;
    int32_t nm, jc, tc;
};
CMST_HD Fields fields_of(const cm_mapped_read &m, uint32_t mate) {
    Fields f;
    f.flag = flag_of(m, mate);
    if (f.flag & RUNMAP) {
        f.pos = f.pnext = f.tlen = 0;
        f.nm = f.jc = f.tc = 0;
        return f;
    }
    f.pos = mate ? m.spos_r2 : m.spos_r1;
    f.pnext = mate ? m.spos_r1 : m.spos_r2;
    const bool plus = (m.spos_r1 < m.spos_r2) == (mate == 0);
    f.tlen = plus ? (uint32_t)m.tlen : 0u - (uint32_t)m.tlen;
    f.nm = mate ? m.ed_r2 : m.ed_r1;
    f.jc = (int32_t)m.junc_num;
    f.tc = m.gm_compatible != 0 ? 1 : 0;
    return f;
}
// QNAME .. TLEN with the tab behind it
CMST_HD uint32_t head_len(const Fields &f, const cm_mapped_read &m, uint32_t name_len, const ChrTab &ct) {
    const uint32_t rname = (f.flag & RUNMAP) ? 1u : chr_len(ct, m.chr_id);
    return name_len + 1u + dec_len(f.flag) + 1u + rname + 1u + dec_len(f.pos) + 7u + 1u + 1u + dec_len(f.pnext) + 1u + dec_len(f.tlen) + 1u;
}
// the four tags and the line feed
CMST_HD uint32_t tail_len(const Fields &f, const cm_mapped_read &m) {
    return 4u * 6u + int_len(m.type) + int_len(f.nm) + int_len(f.jc) + int_len(f.tc) + 1u;
}
// bytes of the record of mate `mate` of state m: the name, the read seq[s .. s + len) (looked at only when the record is reversed)
CMST_HD uint32_t item_len(const cm_mapped_read &m, uint32_t mate, uint32_t name_len, const uint8_t *seq, uint64_t s, uint32_t len, const ChrTab &ct) {
    const Fields f = fields_of(m, mate);
    const uint32_t cut = (f.flag & RREVER) ? rc_cut(seq, s, len) : len;
    return head_len(f, m, name_len, ct) + cut + 1u + len + tail_len(f, m);
}

// the two strings of a record, as format_ends leaves them for copy_strings
struct Strings {
    uint64_t src;            // the read's offset in seq / qual
    uint32_t at;             // where SEQ starts in the destination
    uint32_t cut, len;       // bytes of SEQ, bytes of the read (= bytes of QUAL)
    uint32_t rev_mate;       // bit 0: reversed, bit 1: mate 2
};
// The ends of the record of `total` bytes at dst[d ..): everything but SEQ and QUAL.  `total` is the record's length from the scan;
// the length of SEQ follows from it, so the read is not looked at here.
CMST_HD Strings format_ends(uint8_t *dst, uint64_t d, uint32_t total, const cm_mapped_read &m, uint32_t mate, const uint8_t *name, uint32_t name_len, uint64_t src,
                            uint32_t len, const ChrTab &ct) {
    const Fields f = fields_of(m, mate);
    const bool un = (f.flag & RUNMAP) != 0;
    uint8_t *p = put_bytes(dst + d, name, name_len);
    *p++ = '\t'; p = put_u32(p, f.flag);
    *p++ = '\t';
    if (un) *p++ = '*';
    else p = put_chr(p, ct, m.chr_id);
    *p++ = '\t'; p = put_u32(p, f.pos);
    p = put_lit(p, "\t255\t*\t", 7);
    *p++ = un ? '*' : '=';
    *p++ = '\t'; p = put_u32(p, f.pnext);
    *p++ = '\t'; p = put_u32(p, f.tlen);
    *p++ = '\t';
    const uint32_t hl = (uint32_t)(p - (dst + d)), cut = total - hl - 1u - len - tail_len(f, m);
    p += cut;
    *p++ = '\t';
    p += len;
    p = put_lit(p, "\tAT:i:", 6); p = put_i32(p, m.type);
    p = put_lit(p, "\tNM:i:", 6); p = put_i32(p, f.nm);
    p = put_lit(p, "\tJC:i:", 6); p = put_i32(p, f.jc);
    p = put_lit(p, "\tTC:i:", 6); p = put_i32(p, f.tc);
    *p = '\n';
    Strings S;
    S.src = src;
    S.at = (uint32_t)d + hl;
    S.cut = cut;
    S.len = len;
    S.rev_mate = ((f.flag & RREVER) ? 1u : 0u) | (mate ? 2u : 0u);
    return S;
}
// Lane `lane` of `lanes` moves its share of the first n bytes of a field over the read src[s .. s + len) to dst[d .. d + n) (dst
// 4-byte aligned): the rule of cmft::copy_bases.
CMST_HD void put_field(uint8_t *dst, uint64_t d, uint32_t n, const uint8_t *src, uint64_t s, uint32_t len, bool rev, bool cmp, uint32_t lane, uint32_t lanes) {
    const uint64_t d1 = d + n;
    const uint64_t w0 = (d + 3) >> 2, w1 = d1 >> 2;      // the whole words [w0, w1)
    if (w0 >= w1) {
        for (uint32_t j = lane; j < n; j += lanes) dst[d + j] = field_byte(src, s, len, j, rev, cmp);
        return;
    }
    const uint32_t head = (uint32_t)(4 * w0 - d), tail = (uint32_t)(d1 - 4 * w1), body = (uint32_t)(4 * w1 - d);
    for (uint32_t j = lane; j < head; j += lanes) dst[d + j] = field_byte(src, s, len, j, rev, cmp);
    for (uint32_t j = lane; j < tail; j += lanes) dst[4 * w1 + j] = field_byte(src, s, len, body + j, rev, cmp);
    uint32_t *dw = (uint32_t *)dst;
    for (uint64_t w = w0 + lane; w < w1; w += lanes) dw[w] = field_word(src, s, len, (uint32_t)(4 * w - d), rev, cmp);
}
// SEQ and QUAL of the record S describes, into the dst format_ends wrote its ends to (word 0 of dst is a word of the output: see
// cmrt::window_at)
CMST_HD void copy_strings(uint8_t *dst, const Strings &S, const uint8_t *seq, const uint8_t *qual, uint32_t lane, uint32_t lanes) {
    const bool rev = (S.rev_mate & 1u) != 0;
    put_field(dst, S.at, S.cut, seq, S.src, S.len, rev, rev, lane, lanes);
    put_field(dst, (uint64_t)S.at + S.cut + 1u, S.len, qual, S.src, S.len, rev, false, lane, lanes);
}

// the format as the plan of cm_rows_text.h takes it
struct Format {
    static constexpr uint32_t PAIR_ITEMS = 2, SPAN_ITEMS = SPAN_RECS, STEPS = 2;
    static constexpr uint64_t PAIR_LIMIT = 0x7fffffffull;
    static constexpr uint32_t ITEM_FIXED_MAX = REC_FIXED_MAX, ITEM_CHRS = 1;
    // the states, the kept names, the bases and the kept qualities of the resident batch
    struct Src {
        const cm_mapped_read *state;
        const uint8_t *names;
        const uint32_t *name_off;
        const uint8_t *seq[2], *qual[2];
        const uint64_t *off[2];
    };
    struct Scratch {
        Strings desc[SPAN_RECS];
    };
    // record q of the call is mate q & 1 of pair first + q / 2
    static CMRT_PLAN uint32_t item_len(const Src &S, const ChrTab &ct, uint64_t first, uint32_t q) {
        const uint64_t pair = first + q / 2;
        const uint32_t mate = q & 1u;
        const cm_mapped_read m = S.state[pair];
        const uint64_t a = S.off[mate][pair];
        return cmst::item_len(m, mate, S.name_off[pair + 1] - S.name_off[pair], S.seq[mate], a, (uint32_t)(S.off[mate][pair + 1] - a), ct);
    }
    // step 0: the ends of the span's records, a lane each; step 1: their strings
    static CMRT_PLAN void step(uint32_t i, uint8_t *dst, uint32_t shift, Scratch &sc, const Src &S, const ChrTab &ct, uint64_t first, uint32_t q0, uint32_t n,
                               const uint32_t *off, uint32_t lane) {
        if (i == 0) {
            if (lane >= n) return;
            const uint32_t q = q0 + lane, mate = q & 1u;
            const uint64_t pair = first + q / 2;
            const cm_mapped_read m = S.state[pair];
            const uint32_t na = S.name_off[pair];
            const uint64_t a = S.off[mate][pair];
            sc.desc[lane] = format_ends(dst, off[q] - shift, off[q + 1] - off[q], m, mate, S.names + na, S.name_off[pair + 1] - na, a, (uint32_t)(S.off[mate][pair + 1] - a), ct);
        } else {
            const uint32_t r = lane / REC_LANES;
            if (r >= n) return;
            const Strings D = sc.desc[r];
            const uint32_t mate = D.rev_mate >> 1;
            copy_strings(dst, D, S.seq[mate], S.qual[mate], lane % REC_LANES, REC_LANES);
        }
    }
};

}  // namespace cmst
#endif /* CM_SAM_TEXT_H */
