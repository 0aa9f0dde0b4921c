// Host emulation of the kept names of cm_reads_stage_text (flag bit 2) and of cm_format_pam -- test infrastructure only.
//
// Runs the bodies of circminer_amd/csrc/cm_pam_text.h the way the kernels of cm_hot.hip call them: one lane per record for the
// name's place and length, an exclusive scan, COPY_LANES lanes per record for the copy (cmft::copy_bases); one lane per row for
// its length, an exclusive scan, one wave per span of SPAN_ROWS rows, which formats into a window and streams the window out, or
// lets every lane store its own row.  Records, rows, spans, the lanes of a span and the lanes of a copy run in a SHUFFLED order
// (seed): nothing may depend on the order the device happens to run them in.  Every array a body writes is an exact-size heap
// block filled with 0xA5: a byte nobody wrote shows, and a sanitizer sees a byte written past the end.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_fastq_text.h"
#include "cm_pam_text.h"

namespace {
std::vector<uint32_t> shuffled(uint32_t n, std::mt19937_64 &rng) {
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}
void exclusive_scan(uint32_t *v, size_t n) {
    uint32_t run = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
}
// an exact-size heap block (word aligned, as device memory is), filled with 0xA5
struct Words {
    uint32_t *p;
    explicit Words(size_t bytes) : p((uint32_t *)malloc(bytes ? bytes : 1)) { memset(p, 0xa5, bytes ? bytes : 1); }
    ~Words() { free(p); }
    uint8_t *bytes() const { return (uint8_t *)p; }
};
}  // namespace

// The names of the first n records of `text` (FASTQ, records of four lines, all well-formed): names = room for len bytes,
// name_off = n + 1 words.  The line table is made here the plain way; the tokeniser's own is tests/hostemu_fastq.cpp's business.
extern "C" int emu_names(const uint8_t *text, uint64_t len, uint32_t n, uint64_t seed, uint8_t *names, uint32_t *name_off) {
    if (!name_off || len > 0xfffffff0ull) return CM_EINVAL;
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> store((size_t)((len + 15) / 16 * 16 + cmft::TEXT_SLACK) / 4, 0xa5a5a5a5u);
    if (len) memcpy(store.data(), text, len);
    const uint8_t *t = (const uint8_t *)store.data();
    std::vector<uint32_t> ls{0u};
    for (uint64_t i = 0; i < len; ++i)
        if (t[i] == '\n') ls.push_back((uint32_t)i + 1u);
    if (len && t[len - 1] != '\n') ls.push_back((uint32_t)len + 1u);
    if (ls.size() < 4 * (size_t)n + 1) return CM_EINVAL;
    std::vector<uint32_t> nstart((size_t)n + 1, 0xa5a5a5a5u), off((size_t)n + 1, 0xa5a5a5a5u);
    for (uint32_t i : shuffled(n + 1, rng)) {                     // k_ft_name_len
        uint32_t s = 0, l = 0;
        if (i < n) {
            const uint32_t h = ls[4 * (size_t)i];
            cmpt::name_span(t + h, ls[4 * (size_t)i + 1] - 1u - h, &s, &l);
            s += h;
        }
        nstart[i] = s;
        off[i] = l;
    }
    exclusive_scan(off.data(), off.size());
    const uint32_t total = off[n];
    Words dst(total);                                             // exactly the bytes of the names
    for (uint32_t i : shuffled(n, rng))                           // k_ft_name_copy
        for (uint32_t lane : shuffled(cmft::COPY_LANES, rng)) cmft::copy_bases(dst.bytes(), off[i], t, nstart[i], off[i + 1] - off[i], (int)lane, cmft::COPY_LANES);
    if (names && total) memcpy(names, dst.bytes(), total);
    memcpy(name_off, off.data(), off.size() * sizeof(uint32_t));
    return CM_OK;
}

// cm_format_pam over host arrays: states (n_pairs), the names as emu_names leaves them, the chromosome table
extern "C" int emu_format_pam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats,
                              uint64_t seed) {
    if (!out_bytes || (n_chr && !chrs)) return CM_EINVAL;
    *out_bytes = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n_pairs == 0 || !name_off) return CM_ESTATE;
    if (first > n_pairs || count > n_pairs - first) return CM_EINVAL;
    if (!out && cap) return CM_EINVAL;
    if (count == 0) return CM_OK;
    if (count >= 0xffffffffull) return CM_ELIMIT;
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> chr_off((size_t)n_chr + 1, 0u);
    std::vector<uint8_t> chr_text;
    for (uint32_t c = 0; c < n_chr; ++c) {
        if (chrs[c].name) chr_text.insert(chr_text.end(), chrs[c].name, chrs[c].name + strlen(chrs[c].name));
        chr_off[c + 1] = (uint32_t)chr_text.size();
    }
    chr_text.push_back(0);
    const cmpt::ChrTab ct{chr_text.data(), chr_off.data(), n_chr};
    const uint32_t cnt = (uint32_t)count, spans = (cnt + cmpt::SPAN_ROWS - 1) / cmpt::SPAN_ROWS;
    std::vector<uint32_t> off((size_t)cnt + 1, 0xa5a5a5a5u);
    unsigned long long total64 = 0;
    for (uint32_t k : shuffled(cnt + 1, rng)) {                   // k_pam_len
        uint32_t l = 0;
        if (k < cnt) l = cmpt::row_len(states[first + k], name_off[first + k + 1] - name_off[first + k], ct);
        off[k] = l;
        total64 += l;                                             // (k_pam_total)
    }
    exclusive_scan(off.data(), off.size());
    *out_bytes = total64;
    if (total64 >= (1ull << 32) || total64 > cap) return CM_ELIMIT;
    const uint32_t total = (uint32_t)total64;
    Words rows(total);
    std::vector<uint8_t> path(spans, 0xa5);
    for (uint32_t b : shuffled(spans, rng)) {                     // k_pam_rows, one wave per span
        const uint32_t k0 = b * cmpt::SPAN_ROWS, k1 = cnt - k0 < cmpt::SPAN_ROWS ? cnt : k0 + cmpt::SPAN_ROWS;
        const uint32_t s = off[k0], e = off[k1];
        const bool staged = cmpt::span_in_window(s, e);
        path[b] = staged ? 1 : 0;
        if (staged) {
            Words win(cmpt::WINDOW_WORDS * 4);
            for (uint32_t lane : shuffled(cmpt::SPAN_ROWS, rng)) {
                const uint32_t k = k0 + lane;
                if (k >= cnt) continue;
                const uint32_t a = name_off[first + k];
                cmpt::format_row(win.bytes() + cmpt::window_at(s, off[k]), states[first + k], names + a, name_off[first + k + 1] - a, ct);
            }
            for (uint32_t lane : shuffled(cmpt::SPAN_ROWS, rng)) cmpt::stream_span(rows.bytes(), win.bytes(), s, e, lane, cmpt::SPAN_ROWS);
        } else {
            for (uint32_t lane : shuffled(cmpt::SPAN_ROWS, rng)) {
                const uint32_t k = k0 + lane;
                if (k >= cnt) continue;
                const uint32_t a = name_off[first + k];
                cmpt::format_row(rows.bytes() + off[k], states[first + k], names + a, name_off[first + k + 1] - a, ct);
            }
        }
    }
    memcpy(out, rows.bytes(), total);
    if (stats) {
        stats[0] = count;
        stats[1] = total;
        for (uint32_t b = 0; b < spans; ++b) ++stats[path[b] ? 2 : 3];
    }
    return CM_OK;
}
