// Host emulation of the kept qualities of cm_reads_stage_text (flag bit 3) and of cm_format_sam -- test infrastructure only.
//
// The qualities run cmft::copy_bases the way k_ft_qual_copy calls it, records and lanes in a SHUFFLED order (seed), into an
// exact-size heap block.  The records are hostemu_rows.h's emu::format with the SAM format: the plan the kernels run, under shadow
// buffers; the bases and qualities are exact-size heap blocks plus the word of slack the device arrays have.
#include "hostemu_rows.h"

#include "cm_sam_text.h"

using namespace emu;

// k_ft_qual_copy over host arrays: the quality lines (line 4 i + 3) of the first n records of `text` into qual[off[i] ..)
extern "C" int emu_quals(const uint8_t *text, uint64_t len, uint32_t n, const uint64_t *off, uint64_t seed, uint8_t *qual) {
    if (!off || len > 0xfffffff0ull) return CM_EINVAL;
    std::mt19937_64 rng(seed);
    const TextLines T(text, len);
    if (!T.holds(n)) return CM_EINVAL;
    Words dst((size_t)off[n], 0xa5);                              // exactly the bytes of the qualities
    for (uint32_t i : shuffled(n, rng))
        for (uint32_t lane : shuffled(cmft::COPY_LANES, rng))
            cmft::copy_bases(dst.bytes(), off[i], T.t(), T.ls[4 * (size_t)i + 3], (uint32_t)(off[i + 1] - off[i]), (int)lane, cmft::COPY_LANES);
    if (qual && off[n]) memcpy(qual, dst.bytes(), (size_t)off[n]);
    return CM_OK;
}

// cm_format_sam over host arrays
extern "C" int emu_format_sam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const uint8_t *seq1,
                              const uint64_t *off1, const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats, uint64_t seed,
                              uint32_t window, uint32_t *rec_off, uint64_t *writes) {
    int rc;
    if (refused<cmst::Format>(&rc, n_pairs, name_off && qual1 && qual2, chrs, n_chr, first, count, out, cap, out_bytes, stats, &window)) return rc;
    const Source s1(seq1, (size_t)off1[n_pairs]), s2(seq2, (size_t)off2[n_pairs]), q1(qual1, (size_t)off1[n_pairs]), q2(qual2, (size_t)off2[n_pairs]);
    const cmst::Format::Src S{states, names, name_off, {s1.bytes(), s2.bytes()}, {q1.bytes(), q2.bytes()}, {off1, off2}};
    return format<cmst::Format>(S, chrs, n_chr, first, count, out, cap, out_bytes, stats, seed, window, rec_off, writes);
}
