// Host emulation of the kept names of cm_reads_stage_text (flag bit 2) and of cm_format_pam -- test infrastructure only.
//
// The names run the bodies of circminer_amd/csrc/cm_pam_text.h the way the kernels of cm_hot.hip call them: one lane per record
// for the name's place and length, an exclusive scan, COPY_LANES lanes per record for the copy (cmft::copy_bases), records and
// lanes in a SHUFFLED order (seed), into an exact-size heap block filled with 0xA5.  The rows are hostemu_rows.h's emu::format
// with the PAM format: the plan the kernels run, under shadow buffers.
#include "hostemu_rows.h"

#include "cm_pam_text.h"

using namespace emu;

// The names of the first n records of `text` (FASTQ, records of four lines, all well-formed): names = room for len bytes,
// name_off = n + 1 words.
extern "C" int emu_names(const uint8_t *text, uint64_t len, uint32_t n, uint64_t seed, uint8_t *names, uint32_t *name_off) {
    if (!name_off || len > 0xfffffff0ull) return CM_EINVAL;
    std::mt19937_64 rng(seed);
    const TextLines T(text, len);
    if (!T.holds(n)) return CM_EINVAL;
    std::vector<uint32_t> nstart((size_t)n + 1, 0xa5a5a5a5u), off((size_t)n + 1, 0xa5a5a5a5u);
    for (uint32_t i : shuffled(n + 1, rng)) {                     // k_ft_name_len
        uint32_t s = 0, l = 0;
        if (i < n) {
            const uint32_t h = T.ls[4 * (size_t)i];
            cmpt::name_span(T.t() + h, T.ls[4 * (size_t)i + 1] - 1u - h, &s, &l);
            s += h;
        }
        nstart[i] = s;
        off[i] = l;
    }
    exclusive_scan(off.data(), off.size());
    const uint32_t total = off[n];
    Words dst(total, 0xa5);                                       // exactly the bytes of the names
    for (uint32_t i : shuffled(n, rng))                           // k_ft_name_copy
        for (uint32_t lane : shuffled(cmft::COPY_LANES, rng)) cmft::copy_bases(dst.bytes(), off[i], T.t(), nstart[i], off[i + 1] - off[i], (int)lane, cmft::COPY_LANES);
    if (names && total) memcpy(names, dst.bytes(), total);
    memcpy(name_off, off.data(), off.size() * sizeof(uint32_t));
    return CM_OK;
}

// cm_format_pam over host arrays: states (n_pairs), the names as emu_names leaves them, the chromosome table
extern "C" int emu_format_pam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats,
                              uint64_t seed, uint32_t window, uint32_t *rec_off, uint64_t *writes) {
    int rc;
    if (refused<cmpt::Format>(&rc, n_pairs, name_off != nullptr, chrs, n_chr, first, count, out, cap, out_bytes, stats, &window)) return rc;
    const cmpt::Format::Src S{states, names, name_off};
    return format<cmpt::Format>(S, chrs, n_chr, first, count, out, cap, out_bytes, stats, seed, window, rec_off, writes);
}
