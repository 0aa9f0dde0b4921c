// cm_remain_order.h — the order of the sorted remain records (cm_format_remain_sorted), written once.
//
// Shared by the HIP kernels (cm_hot.hip: k_remain_keys, k_remain_heads, k_remain_gstart, k_remain_gsizes, k_remain_rank) and by a
// host emulation (tests/hostemu_remain_order.cpp) that g++ compiles, the way cm_remain_text.h is shared.  The order is that of
// cm_sort_remain (host_circ.cpp) on the files cm_format_remain writes, `paste - - - - | sort -k2,2n` in the C locale:
//   * primary: cmrm::key_of(state, shift), a signed 64-bit value, ascending -- the same for both mate files.  The value, not a parse
//     of the text's second field: a name that holds a TAB moves that field and is outside this order's promise;
//   * ties: the record of mate MATE as cmrm::Format<MATE> prints it, without its last line feed and with the other three read as
//     TAB, compared as unsigned bytes, a proper prefix first (pasted_cmp); records whose pasted lines are identical keep their order
//     in the active set.  Inside a tie group the two files may therefore order the same pairs differently.
// The plan of a call: a lane per entry of the active set makes (radix key, pair) -> a stable radix sort by the key (the sign bit
// flipped: negative keys first) -> a lane per entry marks whether its key differs from its left neighbour's (head), the scan of the
// heads numbers the tie groups, the heads scatter their position into the groups' start table, a lane per group takes its size ->
// per mate file a lane per ENTRY ranks itself inside its group by counting (rank_in_group): rank = members that compare lower,
// or equal and stand to the left.  Counting needs no order of evaluation and no exchange between lanes; a group of g members costs
// g lanes g compares each.  A group above the cap is refused by the driver before any lane ranks.
// The comparator reads the sources (way (a) of the design): the names first, and only when neither name decides -- they are equal,
// or one is a prefix of the other, whose next byte then stands against the space that opens the fields -- both lines as lists of
// segments (Line): name, header fields, TAB, bases, TAB '+' TAB, qualities.  The fields come from cmrm::put_fields into a buffer of
// the lane (FIELDS_BUF bytes, scratch memory on the device: the one place of the formatters that uses any), printed with an EMPTY
// chromosome table, so that either chromosome name is the one byte "-" at a place the spaces give: the names themselves, of any
// length, are segments that point into the table.
#ifndef CM_REMAIN_ORDER_H
#define CM_REMAIN_ORDER_H

#include <stdint.h>

#include "cm_remain_text.h"

namespace cmro {

using namespace cmrm;

// Members of a tie group the ranking takes: 4096^2 compares per file are what one group may cost (k_ib_order_wg's bound for a
// bucket of the index builder).  CM_REMAIN_TIE_CAP (a test knob) lowers it.
constexpr uint32_t TIE_CAP = 4096;

// the key as the radix sort orders it: unsigned, negative values first
CMRM_HD uint64_t radix_of(int64_t key) { return (uint64_t)key ^ (1ull << 63); }
CMRM_HD int64_t key_of_radix(uint64_t r) { return (int64_t)(r ^ (1ull << 63)); }

// entry q of the active set S.sel: its radix key and its pair
CMRM_HD void entry_key(const Src &S, uint32_t n_chr, uint32_t q, uint64_t *rkey, uint32_t *pair) {
    const uint32_t p = S.sel[q];
    const cm_mapped_read m = S.state[p];
    rkey[q] = radix_of(key_of(m, shift_of(S.chr_shift, n_chr, m.chr_id)));
    pair[q] = p;
}
// lane i of n + 1 over the sorted keys: 1 where a tie group starts; entry n is 0, the slot the scan leaves the groups' count in
CMRM_HD void group_head(const uint64_t *rkey, uint32_t n, uint32_t i, uint32_t *head) {
    if (i > n) return;
    head[i] = (i < n && (i == 0 || rkey[i] != rkey[i - 1])) ? 1u : 0u;
}
// lane i of n + 1 over the scanned heads ex[0 .. n]: a head leaves its position in its group's slot; lane n closes the table
CMRM_HD void group_start(const uint32_t *ex, uint32_t n, uint32_t i, uint32_t *gstart) {
    if (i > n) return;
    if (i == n) gstart[ex[n]] = n;
    else if (ex[i + 1] != ex[i]) gstart[ex[i]] = i;
}
// members of group g (0 for a lane beyond the groups)
CMRM_HD uint32_t group_size(const uint32_t *gstart, uint32_t n_groups, uint32_t g) { return g < n_groups ? gstart[g + 1] - gstart[g] : 0u; }

// ---- the comparator -----------------------------------------------------------------------------------------------------------
constexpr uint32_t SEGS = 10;                                   // name, fields (up to five pieces), TAB, bases, TAB + TAB, qualities
constexpr uint32_t FIELDS_BUF = REC_FIXED_MAX + 2u + 4u;        // the fields with "-" for either chromosome, and the four bytes between the strings
struct Line {
    const uint8_t *p[SEGS];
    uint32_t n[SEGS];
};

// the pasted line of mate MATE of `pair` behind its '@' (which every line has): segments into the sources and into buf
template <uint32_t MATE>
CMRM_HD void make_line(Line &L, uint8_t *buf, const Src &S, const ChrTab &ct, uint32_t pair) {
    const cm_mapped_read m = S.state[pair];
    const uint32_t na = S.name_off[MATE][pair];
    const uint64_t a = S.off[MATE][pair];
    const uint32_t len = (uint32_t)(S.off[MATE][pair + 1] - a);
    const ChrTab none{ct.text, ct.off, 0u};
    const uint32_t f = (uint32_t)(put_fields(buf, m, shift_of(S.chr_shift, ct.n, m.chr_id), none) - buf);
    uint8_t *t = buf + f;
    t[0] = '\t', t[1] = '\t', t[2] = '+', t[3] = '\t';
    for (uint32_t k = 0; k < SEGS; ++k) L.p[k] = buf, L.n[k] = 0u;
    L.p[0] = S.names[MATE] + na, L.n[0] = S.name_off[MATE][pair + 1] - na;
    if (cmpt::mapped_type(m.type) && m.chr_id >= 0 && (uint32_t)m.chr_id < ct.n) {
        // the chromosome is the field behind the third space and again the one behind the eleventh
        uint32_t c[2] = {0u, 0u}, spaces = 0u;
        for (uint32_t k = 0; k < f; ++k)
            if (buf[k] == ' ') {
                ++spaces;
                if (spaces == 3u) c[0] = k + 1u;
                if (spaces == 11u) c[1] = k + 1u;
            }
        const uint8_t *name = ct.text + ct.off[m.chr_id];
        const uint32_t nl = ct.off[m.chr_id + 1] - ct.off[m.chr_id];
        L.p[1] = buf, L.n[1] = c[0];
        L.p[2] = name, L.n[2] = nl;
        L.p[3] = buf + c[0] + 1u, L.n[3] = c[1] - c[0] - 1u;
        L.p[4] = name, L.n[4] = nl;
        L.p[5] = buf + c[1] + 1u, L.n[5] = f - c[1] - 1u;
    } else {
        L.p[1] = buf, L.n[1] = f;
    }
    L.p[6] = t, L.n[6] = 1u;
    L.p[7] = S.seq[MATE] + a, L.n[7] = len;
    L.p[8] = t + 1, L.n[8] = 3u;
    L.p[9] = S.qual[MATE] + a, L.n[9] = len;
}
// unsigned bytes, a proper prefix first: < 0, 0, > 0
CMRM_HD int cmp_lines(const Line &A, const Line &B) {
    uint32_t ia = 0, ib = 0, ka = 0, kb = 0;
    for (;;) {
        while (ia < SEGS && ka == A.n[ia]) ++ia, ka = 0;
        while (ib < SEGS && kb == B.n[ib]) ++ib, kb = 0;
        if (ia == SEGS || ib == SEGS) return (ia == SEGS ? 0 : 1) - (ib == SEGS ? 0 : 1);
        const uint8_t x = A.p[ia][ka], y = B.p[ib][kb];
        if (x != y) return x < y ? -1 : 1;
        ++ka, ++kb;
    }
}
// the names alone: < 0 / > 0 where a byte both names have decides, 0 where the lines have to be read
template <uint32_t MATE>
CMRM_HD int cmp_names(const Src &S, uint32_t pa, uint32_t pb) {
    const uint32_t oa = S.name_off[MATE][pa], ob = S.name_off[MATE][pb];
    const uint32_t la = S.name_off[MATE][pa + 1] - oa, lb = S.name_off[MATE][pb + 1] - ob, l = la < lb ? la : lb;
    const uint8_t *a = S.names[MATE] + oa, *b = S.names[MATE] + ob;
    for (uint32_t k = 0; k < l; ++k)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return 0;
}
// the pasted lines of mate MATE of two pairs
template <uint32_t MATE>
CMRM_HD int cmp_pairs(const Src &S, const ChrTab &ct, uint32_t pa, uint32_t pb) {
    const int c = cmp_names<MATE>(S, pa, pb);
    if (c) return c;
    Line A, B;
    uint8_t fa[FIELDS_BUF], fb[FIELDS_BUF];
    make_line<MATE>(A, fa, S, ct, pa);
    make_line<MATE>(B, fb, S, ct, pb);
    return cmp_lines(A, B);
}

// Entry i of the key-sorted list `by_key` (n entries; ex: the scanned heads, gstart: the groups' starts) takes its place in mate
// MATE's list: where it stands for a group of one, otherwise the group's start + the members that sort before it.
template <uint32_t MATE>
CMRM_HD void rank_in_group(const Src &S, const ChrTab &ct, const uint32_t *by_key, const uint32_t *ex, const uint32_t *gstart, uint32_t n, uint32_t i, uint32_t *list) {
    if (i >= n) return;
    const uint32_t g = ex[i + 1] - 1u, gs = gstart[g], ge = gstart[g + 1], me = by_key[i];
    if (ge - gs == 1u) {
        list[i] = me;
        return;
    }
    Line mine, other;
    uint8_t fm[FIELDS_BUF], fo[FIELDS_BUF];
    bool made = false;
    uint32_t r = 0;
    for (uint32_t j = gs; j < ge; ++j) {
        if (j == i) continue;
        const uint32_t pj = by_key[j];
        int c = cmp_names<MATE>(S, pj, me);
        if (c == 0) {
            if (!made) make_line<MATE>(mine, fm, S, ct, me), made = true;
            make_line<MATE>(other, fo, S, ct, pj);
            c = cmp_lines(other, mine);
        }
        r += (c < 0 || (c == 0 && j < i)) ? 1u : 0u;
    }
    list[gs + r] = me;
}

}  // namespace cmro
#endif /* CM_REMAIN_ORDER_H */
