// Host emulation of cm_format_remain and of what cm_reads_stage_text keeps for it -- test infrastructure only.
//
// The kept names (flag bits 2 and 4: the same body over file 1 and over file 2) and the kept qualities (bit 3) are the emulations
// of hostemu_pam.cpp / hostemu_sam.cpp, compiled into this library as they are.  The records are hostemu_rows.h's emu::format with
// cmrm::Format<0> for the first file and cmrm::Format<1> for the second: the plan the kernels run, under shadow buffers, once per
// mate file over one Src, as the driver in cm_hot.hip does -- both sized before either is written.  The selection list, the bases,
// the qualities and the keys are exact-size heap blocks (bases and qualities with the word of slack the device arrays have).
#include "hostemu_pam.cpp"
#include "hostemu_sam.cpp"

#include "cm_remain_text.h"

// cm_format_remain over host arrays.  sel: the n_sel active pairs, ascending (compact_active's list); bits: the batch has names of
// both files and qualities.  writes (nullable): [0] / [1] the fewest / most writes a byte of either file got.  window: see
// hostemu_rows.h.
extern "C" int emu_format_remain(const cm_mapped_read *states, uint64_t n_pairs, const uint32_t *sel, uint64_t n_sel, const uint8_t *names1,
                                 const uint32_t *name_off1, const uint8_t *names2, const uint32_t *name_off2, const uint8_t *seq1, const uint64_t *off1,
                                 const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs, uint32_t n_chr,
                                 uint64_t first, uint64_t count, uint8_t *out1, uint64_t cap1, uint8_t *out2, uint64_t cap2, uint64_t *out_bytes, int64_t *out_keys,
                                 uint64_t *n_records, uint64_t *stats, uint64_t seed, uint32_t window, uint64_t *writes) {
    if (!out_bytes || (n_chr && !chrs)) return CM_EINVAL;
    out_bytes[0] = out_bytes[1] = 0;
    if (n_records) *n_records = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n_pairs == 0) return CM_ESTATE;
    if (n_records) *n_records = n_sel;
    if (!name_off1 || !name_off2 || !qual1 || !qual2) return CM_ESTATE;
    if (count == ~0ull && first <= n_sel) count = n_sel - first;
    if (first > n_sel || count > n_sel - first) return CM_EINVAL;
    if ((!out1 && cap1) || (!out2 && cap2)) return CM_EINVAL;
    if (count == 0) return CM_OK;
    if (window == 0) window = cmrt::WINDOW;
    if (window > cmrt::WINDOW) return CM_EINVAL;
    const std::vector<uint32_t> selv(sel, sel + n_sel);
    std::vector<uint32_t> shv(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) shv[c] = chrs[c].start_pos;
    uint32_t *p_sel = exact(selv), *p_sh = exact(shv);
    int64_t *keys = (int64_t *)malloc(count * sizeof(int64_t));
    memset(keys, 0xa5, count * sizeof(int64_t));
    const Source s1(seq1, (size_t)off1[n_pairs]), s2(seq2, (size_t)off2[n_pairs]), q1(qual1, (size_t)off1[n_pairs]), q2(qual2, (size_t)off2[n_pairs]);
    const cmrm::Src S{p_sel, states, {names1, names2}, {name_off1, name_off2}, {s1.bytes(), s2.bytes()}, {q1.bytes(), q2.bytes()}, {off1, off2}, p_sh, out_keys ? keys : nullptr};
    auto run = [&](int m, uint8_t *out, uint64_t cap, uint64_t *bytes, uint64_t *st, uint64_t *wr) {
        return m ? format<cmrm::Format<1>>(S, chrs, n_chr, first, count, out, cap, bytes, st, seed + 1, window, nullptr, wr)
                 : format<cmrm::Format<0>>(S, chrs, n_chr, first, count, out, cap, bytes, st, seed, window, nullptr, wr);
    };
    int rc = CM_OK;
    uint64_t need[2] = {0, 0};
    for (int m = 0; m < 2; ++m) (void)run(m, nullptr, 0, &need[m], nullptr, nullptr);       // the length passes: CM_ELIMIT with the size
    out_bytes[0] = need[0];
    out_bytes[1] = need[1];
    if (need[0] >= (1ull << 32) || need[1] >= (1ull << 32) || need[0] > cap1 || need[1] > cap2) rc = CM_ELIMIT;
    uint64_t w[2][3] = {{0, 0, 0}, {0, 0, 0}}, st[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (int m = 0; m < 2 && rc == CM_OK; ++m) rc = run(m, m ? out2 : out1, m ? cap2 : cap1, &need[m], st[m], w[m]);
    if (rc == CM_OK) {
        if (out_keys) memcpy(out_keys, keys, count * sizeof(int64_t));
        if (stats)
            for (int k = 0; k < 4; ++k) stats[k] = st[0][k] + st[1][k];
        if (writes) writes[0] = std::min(w[0][0], w[1][0]), writes[1] = std::max(w[0][1], w[1][1]);
    }
    free(keys);
    free(p_sh);
    free(p_sel);
    return rc;
}
