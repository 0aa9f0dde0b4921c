// Host emulation of the device-side FASTQ tokeniser (cm_reads_stage_text) -- test infrastructure only.
//
// Runs the bodies of circminer_amd/csrc/cm_fastq_text.h the way the kernels of cm_hot.hip call them: newline counts per chunk of
// NL_CHUNK bytes (64 lanes x 16 bytes), an exclusive scan, the line-start table, one lane per record for the checks, a scan of
// the sequence lengths, COPY_LANES lanes per record for the copy into a buffer with CM_STAGE_PAD bytes of slack on both sides.
// Chunks, records and the lanes of a copy run in a SHUFFLED order (seed): nothing may depend on the order the device happens to
// run them in.  The read buffers start out filled with 0xA5, so a byte nobody wrote shows.  The sizes every array is made by and
// the verdicts drawn from the result block are the entry point's own: cmft::plan_sizes and cmft::verdict, which both call.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_fastq_text.h"

namespace {
constexpr uint32_t PAD = 64;          // cmc::CM_STAGE_PAD
constexpr uint32_t REC_TILE = 256;    // records per workgroup of the record kernel

struct File {
    std::vector<uint32_t> store;      // the block in an aligned array with TEXT_SLACK readable bytes behind it
    const uint8_t *text = nullptr;
    uint64_t len = 0;
    std::vector<uint32_t> cnt, ls, slen;
    std::vector<uint64_t> off, rec;
    std::vector<uint8_t> seq;
};

std::vector<uint32_t> shuffled(uint32_t n, std::mt19937_64 &rng) {
    std::vector<uint32_t> v(n);
    std::iota(v.begin(), v.end(), 0u);
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}
void exclusive_scan(std::vector<uint32_t> &v) {
    uint32_t run = 0;
    for (uint32_t &x : v) {
        const uint32_t c = x;
        x = run;
        run += c;
    }
}
}  // namespace

// seq1 / seq2: len1 / len2 bytes of room; off* / rec*: min(max_pairs, min(len1, len2) / 4) + 1 words.  res: cmft::RES_WORDS words.
extern "C" int emu_stage_text(const uint8_t *text1, uint64_t len1, const uint8_t *text2, uint64_t len2, uint64_t max_pairs, uint32_t flags,
                              int32_t max_read_len, int32_t kmer, uint64_t seed, uint8_t *seq1, uint64_t *off1, uint64_t *rec1, uint8_t *seq2,
                              uint64_t *off2, uint64_t *rec2, cm_text_batch *out, unsigned long long *res) {
    if (!out || !res || kmer < 1) return CM_EINVAL;
    memset(out, 0, sizeof *out);
    std::mt19937_64 rng(seed);
    File F[2];
    const uint8_t *const text[2] = {text1, text2};
    const uint64_t len[2] = {len1, len2};
    cmft::Sizes S;
    if (int file = 0; const int rc = cmft::plan_sizes(text, len, max_pairs, flags, &S, &file)) return rc;
    for (int f = 0; f < 2; ++f) {
        File &X = F[f];
        X.len = len[f];
        X.store.assign((size_t)((len[f] + 15) / 16 * 16 + cmft::TEXT_SLACK) / 4, 0xa5a5a5a5u);
        if (len[f]) memcpy(X.store.data(), text[f], len[f]);
        X.text = (const uint8_t *)X.store.data();
    }
    for (int f = 0; f < 2; ++f) {                            // k_ft_count, scan, k_ft_lines
        File &X = F[f];
        const uint32_t n_chunks = S.n_chunks[f], ls_cap = S.ls_cap[f];
        X.cnt.assign(n_chunks + 1, 0xffffffffu);
        X.ls.assign(ls_cap, 0xffffffffu);
        for (uint32_t c : shuffled(n_chunks + 1, rng)) {
            uint32_t k = 0;
            for (uint32_t lane = 0; lane < 64 && c < n_chunks; ++lane)
                k += cmft::popcount16(cmft::nl_mask16(X.text, (uint64_t)c * cmft::NL_CHUNK + lane * cmft::LANE_BYTES, X.len));
            X.cnt[c] = k;
        }
        exclusive_scan(X.cnt);
        X.ls[0] = 0;
        if (S.trail[f] && X.cnt[n_chunks] + 1 < ls_cap) X.ls[X.cnt[n_chunks] + 1] = (uint32_t)X.len + 1u;
        for (uint32_t c : shuffled(n_chunks, rng)) {
            uint32_t before = X.cnt[c];                      // the wave's exclusive scan over its lanes
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t at = (uint64_t)c * cmft::NL_CHUNK + lane * cmft::LANE_BYTES;
                const uint32_t mask = cmft::nl_mask16(X.text, at, X.len);
                cmft::put_line_starts(mask, at, before, X.ls.data(), ls_cap);
                before += cmft::popcount16(mask);
            }
        }
    }
    const uint32_t lines[2] = {cmft::line_count(F[0].cnt[S.n_chunks[0]], S.trail[0] != 0), cmft::line_count(F[1].cnt[S.n_chunks[1]], S.trail[1] != 0)};
    const uint32_t n = cmft::pair_count(lines[0], lines[1], S.max_pairs);
    if (n > S.nb) return CM_EHIP;                              // (the sizing rule would be wrong)
    for (int w = 0; w < cmft::RES_WORDS; ++w) res[w] = 0;
    res[cmft::RES_BAD1] = res[cmft::RES_BAD2] = cmft::NO_BAD;
    for (int f = 0; f < 2; ++f) {                            // k_ft_records, scan, k_ft_offsets, k_ft_copy
        File &X = F[f];
        X.slen.assign((size_t)S.nb + 1, 0xffffffffu);
        for (uint32_t tile : shuffled(S.nb / REC_TILE + 1, rng))
            for (uint32_t t = 0; t < REC_TILE; ++t) {
                const uint32_t i = tile * REC_TILE + (REC_TILE - 1 - t);
                uint32_t sl = 0;
                if (i < n) {
                    const uint32_t bad = cmft::check_record(X.text, X.ls.data(), i, f == 0, &sl);
                    if (bad) res[cmft::RES_BAD1 + f] = std::min(res[cmft::RES_BAD1 + f], cmft::bad_key(i, bad));
                }
                if (i <= S.nb) X.slen[i] = sl;
                res[cmft::RES_MAX_LEN] = std::max<unsigned long long>(res[cmft::RES_MAX_LEN], sl);
            }
        exclusive_scan(X.slen);
        X.off.assign((size_t)S.nb + 1, ~0ull);
        X.rec.assign((size_t)S.nb + 1, ~0ull);
        for (uint32_t i : shuffled(n + 1, rng)) {
            X.off[i] = X.slen[i];
            const uint32_t r = X.ls[4 * (uint64_t)i];
            X.rec[i] = r > X.len ? X.len : r;
        }
        X.seq.assign((size_t)X.len + 2 * PAD + 8, 0xa5);
        uint8_t *base = X.seq.data() + ((8 - ((uintptr_t)X.seq.data() & 7u)) & 7u);        // word aligned, as the device buffer is
        for (uint32_t t = 0; t < PAD; ++t) {
            base[t] = 0;
            base[PAD + X.off[n] + t] = 0;
        }
        for (uint32_t i : shuffled(n, rng)) {
            const uint32_t s = X.ls[4 * (uint64_t)i + 1], l = X.ls[4 * (uint64_t)i + 2] - 1u - s;
            for (uint32_t lane : shuffled(cmft::COPY_LANES, rng)) cmft::copy_bases(base, PAD + X.off[i], X.text, s, l, (int)lane, cmft::COPY_LANES);
        }
        for (uint32_t t = 0; t < PAD; ++t)
            if (base[t] != 0 || base[PAD + X.off[n] + t] != 0) return CM_EHIP;           // the copy wrote into the slack
        uint8_t *seq = f ? seq2 : seq1;
        uint64_t *off = f ? off2 : off1, *rec = f ? rec2 : rec1;
        if (seq && X.off[n]) memcpy(seq, base + PAD, X.off[n]);
        if (off) memcpy(off, X.off.data(), ((size_t)n + 1) * sizeof(uint64_t));
        if (rec) memcpy(rec, X.rec.data(), ((size_t)n + 1) * sizeof(uint64_t));
    }
    res[cmft::RES_LINES1] = lines[0];
    res[cmft::RES_LINES2] = lines[1];
    res[cmft::RES_PAIRS] = n;
    res[cmft::RES_BASES1] = F[0].off[n];
    res[cmft::RES_BASES2] = F[1].off[n];
    res[cmft::RES_USED1] = F[0].rec[n];
    res[cmft::RES_USED2] = F[1].rec[n];
    const cmft::Verdict v = cmft::verdict(res, flags, max_pairs, max_read_len, kmer, CM_MAX_SEEDS_PER_READ);
    if (v.code == CM_OK) *out = cm_text_batch{res[cmft::RES_PAIRS], res[cmft::RES_USED1], res[cmft::RES_USED2], (int32_t)res[cmft::RES_MAX_LEN], 0};
    return v.code;
}
