// cm_pam_text.h — the PAM row format of the device-side formatter (cm_format_pam), and the rule of the names cm_reads_stage_text
// keeps for it.
//
// Shared by the HIP kernels (cm_hot.hip: k_ft_name_len, k_pam_len, k_pam_rows) and by a host emulation (tests/hostemu_pam.cpp) that
// g++ compiles, the way cm_fastq_text.h is shared.  The number formats, the chromosome table, the window and the plan of a call
// are cm_rows_text.h's; Format below is what this format plugs into that plan.  The rules are those of pam_row / name_len /
// split_header in host_fastq.cpp:
//   * the name of a pair is token 0 of its R1 header line (tokens: runs of bytes other than ' ' behind the '@'), without a
//     trailing "/x", up to its first NUL byte (cm_write_pam prints names with strlen); a header without a token has an empty name;
//   * a row is the name and 20 tab-separated fields of the state ("%u" / "%d" as pam_row prints them) for a type of mapped_type(),
//     and the name, 21 "*" fields and the type for every other type; a chr_id outside [0, n_chr) prints "-".
// A span is SPAN_ROWS rows; it has one step: every lane formats its own row (format_row), at the row's place in the destination.
#ifndef CM_PAM_TEXT_H
#define CM_PAM_TEXT_H

#include <stdint.h>

#include "circminer_hot.h"
#include "cm_rows_text.h"

#define CMPT_HD CMRT_HD

namespace cmpt {

using namespace cmrt;

constexpr uint32_t SPAN_ROWS = WAVE;                 // rows of one span: the lanes of a wave
constexpr uint32_t UNMAPPED_STARS = 21;
// what a row can take at most without its name and its two chromosome names: 20 tabs and the line feed, eight "%u" of 10 digits,
// six "%d" of 11 bytes, junc_num, gm_compatible, two strands
constexpr uint32_t ROW_FIXED_MAX = 21 + 8 * 10 + 6 * 11 + 5 + 1 + 2;

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

// bytes of the row of state m behind a name of name_len bytes
CMPT_HD uint32_t row_len(const cm_mapped_read &m, uint32_t name_len, const ChrTab &ct) {
    if (!mapped_type(m.type)) return name_len + 2u * UNMAPPED_STARS + 1u + int_len(m.type) + 1u;
    return name_len + 21u + 2u * chr_len(ct, m.chr_id) + dec_len(m.spos_r1) + dec_len(m.epos_r1) + int_len((int32_t)m.mlen_r1) + dec_len(m.qspos_r1) +
           dec_len(m.qepos_r1) + 1u + int_len(m.ed_r1) + dec_len(m.spos_r2) + dec_len(m.epos_r2) + int_len((int32_t)m.mlen_r2) + dec_len(m.qspos_r2) +
           dec_len(m.qepos_r2) + 1u + int_len(m.ed_r2) + int_len(m.tlen) + dec_len(m.junc_num) + 1u + int_len(m.type);
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

// the format as the plan of cm_rows_text.h takes it
struct Format {
    static constexpr uint32_t PAIR_ITEMS = 1, SPAN_ITEMS = SPAN_ROWS, STEPS = 1;
    static constexpr uint64_t PAIR_LIMIT = 0xffffffffull;
    static constexpr uint32_t ITEM_FIXED_MAX = ROW_FIXED_MAX, ITEM_CHRS = 2;
    // the states and the kept names of the resident batch: name i = names[name_off[i] .. name_off[i + 1])
    struct Src {
        const cm_mapped_read *state;
        const uint8_t *names;
        const uint32_t *name_off;
    };
    struct Scratch {};
    static CMRT_PLAN uint32_t item_len(const Src &S, const ChrTab &ct, uint64_t first, uint32_t k) {
        const cm_mapped_read m = S.state[first + k];
        return row_len(m, S.name_off[first + k + 1] - S.name_off[first + k], ct);
    }
    static CMRT_PLAN void step(uint32_t, uint8_t *dst, uint32_t shift, Scratch &, const Src &S, const ChrTab &ct, uint64_t first, uint32_t q0, uint32_t n,
                               const uint32_t *off, uint32_t lane) {
        if (lane >= n) return;
        const uint32_t k = q0 + lane;
        const cm_mapped_read m = S.state[first + k];
        const uint32_t a = S.name_off[first + k];
        format_row(dst + (off[k] - shift), m, S.names + a, S.name_off[first + k + 1] - a, ct);
    }
};

}  // namespace cmpt
#endif /* CM_PAM_TEXT_H */
