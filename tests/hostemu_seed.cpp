// hostemu_seed.cpp — TEST-ONLY: the k-mer word path of cmc::seed_probe (cmc::kmer_from_span, circminer_amd/csrc/cm_core.h) against the
// per-byte loop it replaced, which is kept here as the reference form, and emu-style seeding of a batch through cmc::seed_probe.
// Built as a shared library by tests/test_seed_words_cpu.py and, with a main(), by tests/diag/seed_san_main.cpp (sanitizers).
// Never linked into libcmhot.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "circminer_hot.h"
#include "cm_core.h"

namespace {
constexpr int PAD = 64;             // cmc::CM_STAGE_PAD: what every read buffer on the device has on both sides
static_assert(PAD == cmc::CM_STAGE_PAD, "the test allocates the device's slack");

// the byte loop of seed_probe as it was before the word path (the reference form)
void ref_kmer(const cmc::SV &s, int qpos, int k, int &hv, int &cv, uint32_t &bad) {
    hv = 0; cv = 0; bad = 0;
    const uint32_t rc = s.mode == 1 ? 1u : 0u;
    for (int i = 0; i < k; ++i) {
        uint32_t u = s.mode == 2 ? 0u : (uint32_t)s.p[s.off + (qpos + i) * s.step];
        u = rc ? (u & 0xDFu) : u;
        bad |= (uint32_t)!((u == 'A') | (u == 'C') | (u == 'G') | (u == 'T'));
        uint32_t code = ((u >> 1) ^ (u >> 2)) & 3u;
        code = rc ? 3u - code : code;
        if (i < CM_WINDOW_SIZE) hv = (hv << 2) | (int)code;
        else cv = (cv << 2) | (int)code;
    }
}
// the device's form: KMER_SPAN bytes loaded where kmer_span_at says (over-reads the read, must stay inside the slack)
cmc::KmerCode words_loaded(const cmc::SV &s, int qpos, int k) {
    uint64_t a[3];
    memcpy(a, cmc::kmer_span_at(s, qpos), cmc::KMER_SPAN);
    return cmc::kmer_from_span(a, k, s.mode == 1 ? 1u : 0u);
}
// the host's form: the k bases and nothing else, as seed_probe fills them off the device
cmc::KmerCode words_filled(const cmc::SV &s, int qpos, int k) {
    const uint32_t rc = s.mode == 1 ? 1u : 0u;
    uint8_t span[cmc::KMER_SPAN];
    memset(span, 0xA5, sizeof span);                      // what lies beyond the k bases must not matter
    for (int i = 0; i < k; ++i) span[rc ? cmc::KMER_SPAN - 1 - i : i] = s.p[s.off + (qpos + i) * s.step];
    uint64_t a[3];
    memcpy(a, span, sizeof span);
    return cmc::kmer_from_span(a, k, rc);
}
struct Rng {
    uint64_t x;
    uint32_t next() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); }
};
struct Tally { long long checked = 0, bad_seen = 0, good_seen = 0, mismatch = 0; int first[8] = {0}; };
void compare(const cmc::SV &s, int qpos, int k, Tally &t) {
    int hv, cv; uint32_t bad;
    ref_kmer(s, qpos, k, hv, cv, bad);
    const cmc::KmerCode w[2] = {words_loaded(s, qpos, k), words_filled(s, qpos, k)};
    for (int f = 0; f < 2; ++f) {
        ++t.checked;
        if (w[f].hv != hv || w[f].cv != cv || w[f].bad != bad) {
            if (!t.mismatch) { t.first[0] = k; t.first[1] = s.mode; t.first[2] = qpos; t.first[3] = f; t.first[4] = hv; t.first[5] = w[f].hv; t.first[6] = cv; t.first[7] = w[f].cv; }
            ++t.mismatch;
        }
    }
    if (bad) ++t.bad_seen; else ++t.good_seen;
}
const int KS[4] = {14, 17, 20, 22};
const char ACGT[5] = "ACGT";
// a read of `len` bytes at alignment `al` in a heap block of exactly PAD + al + len + PAD bytes: a load outside it is the sanitizer's
struct Buf {
    std::vector<uint8_t> mem;
    uint8_t *read;
    Buf(int al, int len) : mem((size_t)PAD + al + len + PAD, 0), read(mem.data() + PAD + al) {}
};
void both_strands(const uint8_t *read, int len, int k, Tally &t) {
    const cmc::Read fw{read, len, 0}, rv{read, len, 1};
    for (int qpos = 0; qpos + k <= len; ++qpos) {           // every qpos the read has, not only the seeds' s * k
        compare(fw.view(), qpos, k, t);
        compare(rv.view(), qpos, k, t);
    }
}
}  // namespace

extern "C" {

// one k-mer through kmer_from_span, its span given as bytes (for spot checks from Python)
void seedw_kmer(const uint8_t *span24, int k, int rc, int out[3]) {
    uint64_t a[3];
    memcpy(a, span24, cmc::KMER_SPAN);
    const cmc::KmerCode c = cmc::kmer_from_span(a, k, (uint32_t)rc);
    out[0] = c.hv; out[1] = c.cv; out[2] = (int)c.bad;
}

// Random reads of 150 bytes: k = 14, 17, 20, 22, both strands, every start alignment 0 - 7, every qpos; `flavour` picks the bytes:
// 0 clean ACGT, 1 ACGT with a sprinkle of lower case / N / @ / B D U / bytes >= 0x80 / anything, 2 every byte value 0 - 255 in
// turn (so each lies in some k-mer at every position of it), 3 all lower case.  out: checked, k-mers with / without a bad base,
// mismatches, then the first mismatch (k, mode, qpos, form, hv ref / got, cv ref / got).  Returns the number of mismatches.
long long seedw_sweep(uint64_t seed, int flavour, long long out[12]) {
    Rng g{seed * 2654435761ull + 12345u};
    Tally t;
    static const uint8_t odd[] = {'a', 'c', 'g', 't', 'N', 'n', '@', 'B', 'D', 'U', 'E', 'b', 'd', 'u', 0x80, 0xC1, 0xC3, 0xC7, 0xD4, 0xE1, 0xFF, 0x00, 0x01, 0x21, 0x23, 0x27, 0x34, 0x40, 0x42, 0x45, 0x55, 0x14};
    for (int al = 0; al < 8; ++al) {
        const int len = 150;
        Buf b(al, len);
        for (size_t i = 0; i < b.mem.size(); ++i) b.mem[i] = (uint8_t)g.next();          // the slack holds anything
        for (int i = 0; i < len; ++i) {
            uint8_t ch = (uint8_t)ACGT[g.next() & 3u];
            if (flavour == 1) {
                const uint32_t r = g.next() % 40u;
                if (r == 0) ch = odd[g.next() % sizeof odd];
                else if (r == 1) ch = (uint8_t)g.next();
                else if (r == 2) ch |= 0x20u;
            } else if (flavour == 2) ch = (uint8_t)(i + al * 32 + (int)(seed % 8u) * 150);    // 150 consecutive values slide through every position of a k-mer; seeds 0 and 1 cover 0 - 255
            else if (flavour == 3) ch |= 0x20u;
            b.read[i] = ch;
        }
        for (int ki = 0; ki < 4; ++ki) both_strands(b.read, len, KS[ki], t);
    }
    out[0] = t.checked; out[1] = t.bad_seen; out[2] = t.good_seen; out[3] = t.mismatch;
    for (int i = 0; i < 8; ++i) out[4 + i] = t.first[i];
    return t.mismatch;
}

// A clean k-mer with every byte value 0 - 255 at each of its k positions in turn, both strands, alignments 0 - 7, the k-mer at the
// very start and at the very end of a read of exactly k bytes (both loads reach into the slack).  Same out[] as seedw_sweep.
long long seedw_each_position(uint64_t seed, long long out[12]) {
    Rng g{seed + 77u};
    Tally t;
    for (int ki = 0; ki < 4; ++ki)
        for (int al = 0; al < 8; ++al) {
            const int k = KS[ki];
            Buf b(al, k);
            for (size_t i = 0; i < b.mem.size(); ++i) b.mem[i] = (uint8_t)g.next();
            for (int i = 0; i < k; ++i) b.read[i] = (uint8_t)ACGT[g.next() & 3u];
            for (int pos = 0; pos < k; ++pos) {
                const uint8_t keep = b.read[pos];
                for (int v = 0; v < 256; ++v) {
                    b.read[pos] = (uint8_t)v;
                    both_strands(b.read, k, k, t);
                }
                b.read[pos] = keep;
            }
        }
    out[0] = t.checked; out[1] = t.bad_seen; out[2] = t.good_seen; out[3] = t.mismatch;
    for (int i = 0; i < 8; ++i) out[4 + i] = t.first[i];
    return t.mismatch;
}

// emu-style seeding of a batch (tests/hostemu.cpp: seed_all) through cmc::seed_probe, with bucket descriptors if with_desc; a pair
// whose active[] byte is 0 (active may be null) is not probed.  sums (may be null): k_seed's three counters -- probes, binary-search
// touches, retained hits.
int seedw_seed_batch(const cm_params *P, const cm_index_view *X, const cm_reads *R, uint32_t n_slots, int with_desc, const uint8_t *active,
                     uint32_t *out_start, uint32_t *out_cnt, uint32_t *out_raw, unsigned long long *sums) {
    cmc::Core c;
    c.P = *P;
    c.X = cmc::to_dev(*X);
    memset(&c.A, 0, sizeof c.A);
    std::vector<uint32_t> desc;
    if (with_desc) {
        const uint64_t nb = (uint64_t)1 << (2 * CM_WINDOW_SIZE);
        desc.assign((size_t)nb * cmc::DESC_WORDS, 0u);
        for (uint64_t hv = 0; hv < nb; ++hv) {
            const uint32_t b0 = X->bucket_off[hv], n = X->bucket_off[hv + 1] - b0;
            cmc::desc_pack(b0, n, [&](uint32_t i) { return (uint32_t)X->checksum[b0 + i]; }, P->kmer, desc.data() + hv * cmc::DESC_WORDS);
        }
        c.desc = desc.data();
    }
    const uint64_t n = R->n_pairs;
    const int S = (int)n_slots, k = P->kmer;
    unsigned long long tot[3] = {0, 0, 0};
    for (uint64_t q = 0; q < n * 4 * (uint64_t)S; ++q) {
        const uint32_t s = (uint32_t)(q % S);
        const uint64_t r = q / S, p = r >> 2;
        const int orient = r & 1, mate = (r >> 1) & 1;
        const uint64_t o0 = mate ? R->off2[p] : R->off1[p], o1 = mate ? R->off2[p + 1] : R->off1[p + 1];
        const int len = (int)(o1 - o0);
        out_start[q] = out_cnt[q] = out_raw[q] = 0;
        if ((active && !active[p]) || (int)(s + 1) * k > len) continue;
        const cmc::Read rd{(mate ? R->seq2 : R->seq1) + o0, len, orient};
        const cmc::Probe pr = cmc::seed_probe(c, rd.view(), (int)s * k);
        out_start[q] = pr.start;
        out_raw[q] = pr.raw;
        out_cnt[q] = pr.raw > (uint32_t)P->seed_lim ? 0u : pr.raw;
        tot[0] += 1;
        tot[1] += pr.touches;
        tot[2] += out_cnt[q];
    }
    if (sums) memcpy(sums, tot, sizeof tot);
    return 0;
}

// all the cases above in one call (what tests/diag/seed_san_main.cpp runs); prints and returns the number of mismatches
long long seedw_all(int verbose) {
    long long out[12], bad = 0, checked = 0;
    for (int fl = 0; fl < 4; ++fl)
        for (uint64_t seed = 0; seed < 6u; ++seed) {
            bad += seedw_sweep(seed, fl, out);
            checked += out[0];
            if (verbose) printf("sweep flavour %d seed %d: checked %lld, bad k-mers %lld, clean %lld, mismatches %lld\n", fl, (int)seed, out[0], out[1], out[2], out[3]);
        }
    bad += seedw_each_position(1, out);
    checked += out[0];
    if (verbose) printf("each position: checked %lld, bad k-mers %lld, clean %lld, mismatches %lld\n", out[0], out[1], out[2], out[3]);
    printf("seed words: %lld comparisons, %lld mismatches\n", checked, bad);
    return bad;
}

}  // extern "C"
