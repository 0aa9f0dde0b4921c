// The host emulation of the device-side row formatters (cm_format_pam, cm_format_sam) -- test infrastructure only; included by
// hostemu_pam.cpp, hostemu_sam.cpp and the stand-alone sanitizer programs tests/diag/pam_san_main.cpp / sam_san_main.cpp.
//
// emu_format<F> runs the plan of circminer_amd/csrc/cm_rows_text.h -- the very functions the kernels of cm_hot.hip run
// (cmrt::item_length, cmrt::format_span) -- with an executor that stands for a wave: every lane of a step, in a SHUFFLED order
// (seed), and items and spans shuffled too: nothing may depend on the order the device happens to run them in.  Every call of a
// step writes into shadow buffers pre-filled with 0xA5 and with 0x5A: a byte that differs from its fill in either was written by
// that call, is counted, and goes into the real window / output; a byte written outside the span's own bytes is an error.  So
// every byte of the output is known to be written exactly once, and the sources are exact-size heap blocks for a sanitizer.
#ifndef HOSTEMU_ROWS_H
#define HOSTEMU_ROWS_H

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_fastq_text.h"
#include "cm_rows_text.h"

// the emulations' entry points (hostemu_pam.cpp, hostemu_sam.cpp).  window: bytes of the window (0: cmrt::WINDOW; 1 forces every
// span onto the direct path).  rec_off (nullable, items + 1 words): the scanned lengths.  writes (nullable): [0] / [1] the fewest /
// most writes a byte of the output got, [2] items whose bytes do not end with their only line feed where the length body says.
extern "C" int emu_names(const uint8_t *text, uint64_t len, uint32_t n, uint64_t seed, uint8_t *names, uint32_t *name_off);
extern "C" int emu_quals(const uint8_t *text, uint64_t len, uint32_t n, const uint64_t *off, uint64_t seed, uint8_t *qual);
extern "C" int emu_format_pam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats,
                              uint64_t seed, uint32_t window, uint32_t *rec_off, uint64_t *writes);
extern "C" int emu_format_sam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const uint8_t *seq1,
                              const uint64_t *off1, const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats, uint64_t seed,
                              uint32_t window, uint32_t *rec_off, uint64_t *writes);

namespace emu {

inline std::vector<uint32_t> shuffled(uint32_t n, std::mt19937_64 &rng) {
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}
inline void exclusive_scan(uint32_t *v, size_t n) {
    uint32_t run = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
}
// an exact-size heap block (word aligned, as device memory is)
struct Words {
    uint32_t *p;
    size_t n;
    Words(size_t bytes, int fill) : p((uint32_t *)malloc(bytes ? bytes : 1)), n(bytes) { memset(p, fill, bytes ? bytes : 1); }
    Words(const Words &) = delete;
    ~Words() { free(p); }
    uint8_t *bytes() const { return (uint8_t *)p; }
};
// a source array as the device holds it: the bytes, rounded up to a word, and one word of slack
struct Source : Words {
    Source(const uint8_t *from, size_t bytes) : Words((bytes + 3) / 4 * 4 + 4, 0x3f) {
        if (bytes) memcpy(p, from, bytes);
    }
};
// Two shadows of a destination of `bytes` bytes.  run(f, lo, hi): f writes into both; what it wrote inside [lo, hi) moves into
// `real` and is counted, the shadows are clean again afterwards.  A write outside [lo, hi) stays and is found by clean().
struct Shadow {
    Words a, b;
    explicit Shadow(size_t bytes) : a(bytes, 0xa5), b(bytes, 0x5a) {}
    template <class F>
    void run(F f, uint8_t *real, uint32_t *count, size_t lo, size_t hi) {
        f(a.bytes());
        f(b.bytes());
        uint8_t *x = a.bytes(), *y = b.bytes();
        for (size_t i = lo; i < hi; ++i)
            if (x[i] != 0xa5 || y[i] != 0x5a) {
                real[i] = x[i];
                if (x[i] != y[i]) count[i] += 1000;          // (a body that writes what it read from its destination)
                ++count[i];
                x[i] = 0xa5;
                y[i] = 0x5a;
            }
    }
    bool clean() const {
        for (size_t i = 0; i < a.n; ++i)
            if (a.bytes()[i] != 0xa5 || b.bytes()[i] != 0x5a) return false;
        return true;
    }
};
// the chromosome names as RowsRun::prepare (cm_hot.hip) lays them out
struct ChrTable {
    std::vector<uint32_t> off;
    std::vector<uint8_t> text;
    ChrTable(const cm_chr_info *chrs, uint32_t n_chr) : off((size_t)n_chr + 1, 0u) {
        for (uint32_t c = 0; c < n_chr; ++c) {
            if (chrs[c].name) text.insert(text.end(), chrs[c].name, chrs[c].name + strlen(chrs[c].name));
            off[c + 1] = (uint32_t)text.size();
        }
        text.push_back(0);
    }
    cmrt::ChrTab tab() const { return cmrt::ChrTab{text.data(), off.data(), (uint32_t)off.size() - 1u}; }
};
// A FASTQ text as the tokeniser holds it (padded, with its slack) and its line table, made the plain way; the tokeniser's own is
// tests/hostemu_fastq.cpp's business.  ls[i]: where line i starts.
struct TextLines {
    std::vector<uint32_t> store, ls{0u};
    TextLines(const uint8_t *text, uint64_t len) : store((size_t)((len + 15) / 16 * 16 + cmft::TEXT_SLACK) / 4, 0xa5a5a5a5u) {
        if (len) memcpy(store.data(), text, len);
        for (uint64_t i = 0; i < len; ++i)
            if (t()[i] == '\n') ls.push_back((uint32_t)i + 1u);
        if (len && t()[len - 1] != '\n') ls.push_back((uint32_t)len + 1u);
    }
    const uint8_t *t() const { return (const uint8_t *)store.data(); }
    bool holds(uint32_t records) const { return ls.size() >= 4 * (size_t)records + 1; }
};

// The refusals of a formatter's call in the driver's order (format_rows in cm_hot.hip).  true: *rc is the call's answer.
template <class F>
bool refused(int *rc, uint64_t n_pairs, bool staged_bits, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, const uint8_t *out, uint64_t cap,
             uint64_t *out_bytes, uint64_t *stats, uint32_t *window) {
    *rc = CM_EINVAL;
    if (!out_bytes || (n_chr && !chrs)) return true;
    *out_bytes = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n_pairs == 0 || !staged_bits) return *rc = CM_ESTATE, true;
    if (first > n_pairs || count > n_pairs - first) return true;
    if (!out && cap) return true;
    if (count == 0) return *rc = CM_OK, true;
    if (count >= F::PAIR_LIMIT) return *rc = CM_ELIMIT, true;
    if (*window == 0) *window = cmrt::WINDOW;
    return *window > cmrt::WINDOW;
}

// cmrt::format_span's executor for one span: all WAVE lanes of every step, shuffled, under the shadows
struct Lanes {
    std::mt19937_64 &rng;
    Shadow &sh_win, &sh_out;
    uint8_t *rows;
    uint32_t *n_out;
    Words win{cmrt::WINDOW_WORDS * 4, 0xa5};
    std::vector<uint32_t> n_win = std::vector<uint32_t>(cmrt::WINDOW_WORDS * 4, 0u);
    template <class Fn>
    void in_window(uint32_t s, uint32_t e, Fn f) {
        for (uint32_t lane : shuffled(cmrt::WAVE, rng))
            sh_win.run([&](uint8_t *dst) { f(lane, dst); }, win.bytes(), n_win.data(), cmrt::window_at(s, s), (size_t)cmrt::window_at(s, e - 1) + 1);
    }
    template <class Fn>
    void in_output(uint32_t s, uint32_t e, Fn f) {
        for (uint32_t lane : shuffled(cmrt::WAVE, rng)) sh_out.run([&](uint8_t *dst) { f(lane, dst); }, rows, n_out, s, e);
    }
    void sync() {}
    const uint8_t *window() const { return win.bytes(); }
    bool first_lane() const { return true; }
    // every byte of the window's span written exactly once
    bool window_once(uint32_t s, uint32_t e) const {
        for (size_t i = cmrt::window_at(s, s); i <= cmrt::window_at(s, e - 1); ++i)
            if (n_win[i] != 1) return false;
        return true;
    }
};

// A formatter's call over host arrays, behind refused(): the length pass, the scan, every span through the plan.  -100: a byte
// was written outside its span; -101: a byte of a window was written twice or not at all.
template <class F>
int format(const typename F::Src &S, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes,
           uint64_t *stats, uint64_t seed, uint32_t window, uint32_t *rec_off, uint64_t *writes) {
    std::mt19937_64 rng(seed);
    const ChrTable table(chrs, n_chr);
    const cmrt::ChrTab ct = table.tab();
    const uint32_t items = F::PAIR_ITEMS * (uint32_t)count, spans = (items + F::SPAN_ITEMS - 1) / F::SPAN_ITEMS;
    std::vector<uint32_t> off((size_t)items + 1, 0xa5a5a5a5u);
    for (uint32_t q : shuffled(items + 1, rng)) cmrt::item_length<F>(S, ct, first, items, q, off.data());
    const unsigned long long total64 = std::accumulate(off.begin(), off.end(), 0ull);       // (k_rows_total)
    exclusive_scan(off.data(), off.size());
    *out_bytes = total64;
    if (rec_off) memcpy(rec_off, off.data(), off.size() * sizeof(uint32_t));
    if (total64 >= (1ull << 32) || total64 > cap) return CM_ELIMIT;
    const uint32_t total = (uint32_t)total64;
    Words rows((size_t)total + 4, 0xa5);                          // (the device's output buffer: the bytes and a word)
    Shadow sh_out((size_t)total + 4), sh_win(cmrt::WINDOW_WORDS * 4);
    std::vector<uint32_t> n_out((size_t)total + 4, 0u);
    std::vector<uint8_t> path(spans, 0xa5);
    bool bad = false;
    for (uint32_t b : shuffled(spans, rng)) {                     // one wave per span
        Lanes ex{rng, sh_win, sh_out, rows.bytes(), n_out.data()};
        typename F::Scratch scratch;
        cmrt::format_span<F>(ex, S, ct, first, items, off.data(), b, window, scratch, path.data());
        const uint32_t q0 = b * F::SPAN_ITEMS;
        if (path[b] == 1) bad |= !ex.window_once(off[q0], off[std::min<uint64_t>(items, (uint64_t)q0 + F::SPAN_ITEMS)]);
    }
    if (!sh_out.clean() || !sh_win.clean()) return -100;
    if (bad) return -101;
    uint64_t w_min = ~0ull, w_max = 0, wrong = 0;
    for (uint32_t i = 0; i < total; ++i) {
        w_min = std::min<uint64_t>(w_min, n_out[i]);
        w_max = std::max<uint64_t>(w_max, n_out[i]);
    }
    for (uint32_t i = total; i < total + 4; ++i) w_max = std::max<uint64_t>(w_max, n_out[i] ? 2000 : 0);    // (behind the end)
    for (uint32_t q = 0; q < items; ++q) {
        const uint8_t *r = rows.bytes() + off[q];
        const uint32_t l = off[q + 1] - off[q];
        const void *nl = l ? memchr(r, '\n', l) : nullptr;
        if (!nl || (const uint8_t *)nl != r + l - 1) ++wrong;
    }
    if (writes) writes[0] = w_min, writes[1] = w_max, writes[2] = wrong;
    memcpy(out, rows.bytes(), total);
    if (stats) {
        stats[0] = items;
        stats[1] = total;
        for (uint32_t b = 0; b < spans; ++b) ++stats[path[b] ? 2 : 3];
    }
    return CM_OK;
}

// ---- for the stand-alone sanitizer programs -------------------------------------------------------------------------------------
// an exact-size heap copy, so that any read or write past an argument array is seen
template <class T>
T *exact(const std::vector<T> &v) {
    T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
// State i of the directed states of tests/pam_text_util.py (every printed field at the boundaries of its format).  for_sam: tlen
// without INT_MIN, every fifth pair with equal positions, the lengths left at their fill (tests/sam_text_util.py's concerns).
inline cm_mapped_read directed_state(uint32_t i, int n_chr, bool for_sam) {
    static const uint32_t U32V[] = {0u, 9u, 10u, 99u, 100u, 999999999u, 1000000000u, 4294967295u};
    static const uint32_t MLENV[] = {0u, 9u, 10u, 99u, 100u, 999999999u, 1000000000u, 4294967295u, 2147483648u};
    static const int32_t TYPEV[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, -1, 14, -9, -10, INT_MIN, INT_MAX, 1000000000, 100, 13};
    const int32_t INTV[] = {0, -1, -9, -10, for_sam ? INT_MIN + 1 : INT_MIN, INT_MAX, 1000000000};
    cm_mapped_read m;
    memset(&m, 0xee, sizeof m);
    m.type = TYPEV[i % 23];
    uint32_t *u[8] = {&m.spos_r1, &m.spos_r2, &m.epos_r1, &m.epos_r2, &m.qspos_r1, &m.qspos_r2, &m.qepos_r1, &m.qepos_r2};
    for (uint32_t j = 0; j < 8; ++j) *u[j] = U32V[(i + j) % 8];
    if (for_sam) {
        if (i % 5 == 0) m.spos_r2 = m.spos_r1;
    } else {
        m.mlen_r1 = MLENV[i % 9];
        m.mlen_r2 = MLENV[(i + 4) % 9];
    }
    m.ed_r1 = INTV[i % 7];
    m.ed_r2 = INTV[(i + 2) % 7];
    m.tlen = INTV[(i + 4) % 7];
    m.junc_num = i % 2 ? 65535 : 0;
    m.gm_compatible = (uint8_t)(i % 3 == 2 ? 255 : i % 3);
    m.r1_forward = i & 1;
    m.r2_forward = (i >> 1) & 1;
    const int32_t ids[4] = {-1, 0, n_chr - 1, n_chr};
    m.chr_id = ids[i % 4];
    m.contig_num = (int32_t)(i % 5) - 1;
    return m;
}

}  // namespace emu
#endif /* HOSTEMU_ROWS_H */
