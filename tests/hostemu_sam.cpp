// Host emulation of the kept qualities of cm_reads_stage_text (flag bit 3) and of cm_format_sam -- test infrastructure only.
//
// Runs the bodies of circminer_amd/csrc/cm_sam_text.h the way the kernels of cm_hot.hip call them: one lane per record for its
// length, an exclusive scan, one wave per span of SPAN_RECS records: a lane per record for its ends, REC_LANES lanes per record
// for SEQ and QUAL, into a window that is then streamed out, or straight into the output.  Items, spans and the lanes of every
// step run in a SHUFFLED order (seed): nothing may depend on the order the device happens to run them in.  Every call of a body
// writes into shadow buffers pre-filled with 0xA5 and with 0x5A: a byte that differs from its fill in either was written by that
// call, is counted, and goes into the real window / output; a byte written outside the span's own bytes is an error.  So every
// byte of the output is known to be written exactly once, and the sources are exact-size heap blocks (plus the word of slack the
// device arrays have) for a sanitizer.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_fastq_text.h"
#include "cm_pam_text.h"
#include "cm_sam_text.h"

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
// an exact-size heap block (word aligned, as device memory is)
struct Words {
    uint32_t *p;
    size_t n;
    Words(size_t bytes, int fill) : p((uint32_t *)malloc(bytes ? bytes : 1)), n(bytes) { memset(p, fill, bytes ? bytes : 1); }
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
    Shadow(size_t bytes) : a(bytes, 0xa5), b(bytes, 0x5a) {}
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
}  // namespace

// k_ft_qual_copy over host arrays: the quality lines (line 4 i + 3) of the first n records of `text` into qual[off[i] ..)
extern "C" int emu_quals(const uint8_t *text, uint64_t len, uint32_t n, const uint64_t *off, uint64_t seed, uint8_t *qual) {
    if (!off || len > 0xfffffff0ull) return CM_EINVAL;
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> store((size_t)((len + 15) / 16 * 16 + cmft::TEXT_SLACK) / 4, 0xa5a5a5a5u);
    if (len) memcpy(store.data(), text, len);
    const uint8_t *t = (const uint8_t *)store.data();
    std::vector<uint32_t> ls{0u};
    for (uint64_t i = 0; i < len; ++i)
        if (t[i] == '\n') ls.push_back((uint32_t)i + 1u);
    if (len && t[len - 1] != '\n') ls.push_back((uint32_t)len + 1u);
    if (ls.size() < 4 * (size_t)n + 1) return CM_EINVAL;
    Words dst((size_t)off[n], 0xa5);                              // exactly the bytes of the qualities
    for (uint32_t i : shuffled(n, rng))
        for (uint32_t lane : shuffled(cmft::COPY_LANES, rng))
            cmft::copy_bases(dst.bytes(), off[i], t, ls[4 * (size_t)i + 3], (uint32_t)(off[i + 1] - off[i]), (int)lane, cmft::COPY_LANES);
    if (qual && off[n]) memcpy(qual, dst.bytes(), (size_t)off[n]);
    return CM_OK;
}

// cm_format_sam over host arrays.  window: bytes of the window (0: cmst::WINDOW; 1 forces every span onto the direct path).
// rec_off (nullable, 2 count + 1 words): the scanned lengths.  writes (nullable): [0] / [1] the fewest / most writes a byte of the
// output got, [2] records whose bytes do not end with their only line feed where the length body says.
extern "C" int emu_format_sam(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names, const uint32_t *name_off, const uint8_t *seq1,
                              const uint64_t *off1, const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs,
                              uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *out_bytes, uint64_t *stats, uint64_t seed,
                              uint32_t window, uint32_t *rec_off, uint64_t *writes) {
    if (!out_bytes || (n_chr && !chrs)) return CM_EINVAL;
    *out_bytes = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n_pairs == 0 || !name_off || !qual1 || !qual2) return CM_ESTATE;
    if (first > n_pairs || count > n_pairs - first) return CM_EINVAL;
    if (!out && cap) return CM_EINVAL;
    if (count == 0) return CM_OK;
    if (count >= 0x7fffffffull) return CM_ELIMIT;
    if (window == 0) window = cmst::WINDOW;
    if (window > cmst::WINDOW) return CM_EINVAL;
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> chr_off((size_t)n_chr + 1, 0u);
    std::vector<uint8_t> chr_text;
    for (uint32_t c = 0; c < n_chr; ++c) {
        if (chrs[c].name) chr_text.insert(chr_text.end(), chrs[c].name, chrs[c].name + strlen(chrs[c].name));
        chr_off[c + 1] = (uint32_t)chr_text.size();
    }
    chr_text.push_back(0);
    const cmpt::ChrTab ct{chr_text.data(), chr_off.data(), n_chr};
    const Source s1(seq1, (size_t)off1[n_pairs]), s2(seq2, (size_t)off2[n_pairs]), q1(qual1, (size_t)off1[n_pairs]), q2(qual2, (size_t)off2[n_pairs]);
    const uint8_t *seq[2] = {s1.bytes(), s2.bytes()}, *qual[2] = {q1.bytes(), q2.bytes()};
    const uint64_t *roff[2] = {off1, off2};
    const uint32_t items = 2u * (uint32_t)count, spans = (items + cmst::SPAN_RECS - 1) / cmst::SPAN_RECS;
    std::vector<uint32_t> off((size_t)items + 1, 0xa5a5a5a5u);
    unsigned long long total64 = 0;
    for (uint32_t q : shuffled(items + 1, rng)) {                 // k_sam_len
        uint32_t l = 0;
        if (q < items) {
            const uint64_t pair = first + q / 2;
            const uint32_t mate = q & 1u;
            const uint64_t a = roff[mate][pair];
            l = cmst::item_len(states[pair], mate, name_off[pair + 1] - name_off[pair], seq[mate], a, (uint32_t)(roff[mate][pair + 1] - a), ct);
        }
        off[q] = l;
        total64 += l;                                             // (k_pam_total)
    }
    exclusive_scan(off.data(), off.size());
    *out_bytes = total64;
    if (rec_off) memcpy(rec_off, off.data(), off.size() * sizeof(uint32_t));
    if (total64 >= (1ull << 32) || total64 > cap) return CM_ELIMIT;
    const uint32_t total = (uint32_t)total64;
    Words rows((size_t)total + 4, 0xa5);                          // (the device's output buffer: the bytes and a word)
    Shadow sh_out((size_t)total + 4), sh_win(cmst::WINDOW_WORDS * 4);
    std::vector<uint32_t> n_out((size_t)total + 4, 0u);
    std::vector<uint8_t> path(spans, 0xa5);
    bool bad = false;
    for (uint32_t b : shuffled(spans, rng)) {                     // k_sam_rows, one wave per span
        const uint32_t q0 = b * cmst::SPAN_RECS, q1e = items - q0 < cmst::SPAN_RECS ? items : q0 + cmst::SPAN_RECS;
        const uint32_t s = off[q0], e = off[q1e];
        const bool staged = e - s <= window;
        path[b] = staged ? 1 : 0;
        Words win(cmst::WINDOW_WORDS * 4, 0xa5);
        std::vector<uint32_t> n_win(cmst::WINDOW_WORDS * 4, 0u);
        // where the span's bytes lie in the destination of the two steps
        const size_t lo = staged ? cmpt::window_at(s, s) : s, hi = staged ? cmpt::window_at(s, e - 1) + 1 : e;
        uint8_t *real = staged ? win.bytes() : rows.bytes();
        uint32_t *cnt = staged ? n_win.data() : n_out.data();
        Shadow &sh = staged ? sh_win : sh_out;
        std::vector<cmst::Strings> desc(cmst::SPAN_RECS);
        for (uint32_t lane : shuffled(cmst::WAVE, rng)) {         // the ends: lanes 0 .. SPAN_RECS - 1
            if (lane >= q1e - q0) continue;
            const uint32_t q = q0 + lane, mate = q & 1u;
            const uint64_t pair = first + q / 2;
            const uint32_t na = name_off[pair];
            const uint64_t a = roff[mate][pair];
            const uint64_t d = staged ? cmpt::window_at(s, off[q]) : off[q];
            sh.run([&](uint8_t *dst) {
                desc[lane] = cmst::format_ends(dst, d, off[q + 1] - off[q], states[pair], mate, names + na, name_off[pair + 1] - na, a, (uint32_t)(roff[mate][pair + 1] - a), ct);
            }, real, cnt, lo, hi);
        }
        for (uint32_t lane : shuffled(cmst::WAVE, rng)) {         // the strings: REC_LANES lanes per record
            const uint32_t r = lane / cmst::REC_LANES;
            if (r >= q1e - q0) continue;
            const cmst::Strings D = desc[r];
            const uint32_t mate = D.rev_mate >> 1;
            sh.run([&](uint8_t *dst) { cmst::copy_strings(dst, D, seq[mate], qual[mate], lane % cmst::REC_LANES, cmst::REC_LANES); }, real, cnt, lo, hi);
        }
        if (staged) {
            for (size_t i = lo; i < hi; ++i) bad |= n_win[i] != 1;
            for (uint32_t lane : shuffled(cmst::WAVE, rng))
                sh_out.run([&](uint8_t *dst) { cmpt::stream_span(dst, win.bytes(), s, e, lane, cmst::WAVE); }, rows.bytes(), n_out.data(), s, e);
        }
    }
    if (!sh_out.clean() || !sh_win.clean()) return -100;          // a byte written outside its span
    if (bad) return -101;                                         // a byte of a window written twice or not at all
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
