// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_fastq_text.h through the host emulation (tests/hostemu_fastq.cpp):
// random file pairs, some malformed, some cut, every argument array an exact-size heap block; then cmft::verdict itself, which the
// library and the emulation share, on result blocks at its boundaries.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc \
//       tests/diag/fastq_san_main.cpp tests/hostemu_fastq.cpp -o /tmp/fastq_san && /tmp/fastq_san
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "circminer_hot.h"
#include "cm_fastq_text.h"
extern "C" int emu_stage_text(const uint8_t *, uint64_t, const uint8_t *, uint64_t, uint64_t, uint32_t, int32_t, int32_t, uint64_t, uint8_t *, uint64_t *, uint64_t *,
                              uint8_t *, uint64_t *, uint64_t *, cm_text_batch *, unsigned long long *);
static std::string make(std::mt19937_64 &rng, int n, int mate, bool junk) {
    std::string t;
    for (int i = 0; i < n; ++i) {
        int len = (int)(rng() % 160);
        if (junk && rng() % 9 == 0) t += "\n";
        t += "@r" + std::to_string(i) + std::string(mate == 2 ? i % 7 : 0, 'x') + (i % 3 ? "" : "  c d") + "\n";
        for (int k = 0; k < len; ++k) t += "ACGTN"[rng() % 5];
        t += "\n+\n";
        int ql = junk && rng() % 11 == 0 ? len + 1 : len;
        for (int k = 0; k < ql; ++k) t += (char)(33 + rng() % 40);
        t += "\n";
    }
    if (rng() % 2 && !t.empty()) t.pop_back();
    return t;
}
// the verdict of a result block with the given lines and longest read, no malformed record: (case, code)
static bool is(unsigned long long lines1, unsigned long long lines2, unsigned long long max_len, uint32_t flags, uint64_t max_pairs, cmft::Case what, int code,
               unsigned long long count = 0) {
    unsigned long long R[cmft::RES_WORDS] = {cmft::NO_BAD, cmft::NO_BAD, max_len, lines1, lines2};
    const cmft::Verdict v = cmft::verdict(R, flags, max_pairs, 300, 20, CM_MAX_SEEDS_PER_READ);
    if (v.what == what && v.code == code && v.count == count) return true;
    printf("verdict(lines %llu / %llu, max_len %llu, flags %u, max_pairs %llu): case %d code %d count %llu\n", lines1, lines2, max_len, flags, (unsigned long long)max_pairs,
           (int)v.what, v.code, v.count);
    return false;
}
static bool boundaries() {
    using namespace cmft;
    bool ok = true;
    // lines % 4 against max_pairs: 10 whole records + 1 .. 3 lines are refused while the batch may reach them, not when it ends before
    for (unsigned long long k = 1; k < 4; ++k) {
        ok &= is(40 + k, 44, 100, 3, 11, LINES_LEFT, CM_EINVAL, k) && is(40 + k, 44, 100, 3, 10, ACCEPTED, CM_OK) && is(40 + k, 44, 100, 2, 11, ACCEPTED, CM_OK);
        ok &= is(44, 40 + k, 100, 3, 11, LINES_LEFT, CM_EINVAL, k) && is(44, 40 + k, 100, 1, 10, ACCEPTED, CM_OK);
    }
    // file 2 one record short: of file 1, of max_pairs
    ok &= is(40, 36, 100, 3, 10, FILE2_SHORT, CM_EINVAL) && is(40, 36, 100, 3, 9, ACCEPTED, CM_OK) && is(40, 36, 100, 1, 10, ACCEPTED, CM_OK) && is(36, 40, 100, 3, 10, ACCEPTED, CM_OK);
    // max_len == max_read_len and one more (k = 20: 15 seeds, within any build)
    ok &= is(40, 40, 300, 3, 10, ACCEPTED, CM_OK) && is(40, 40, 301, 3, 10, READ_TOO_LONG, CM_EINVAL, 301);
    // a seed count at and one above the limit: floor(max_len / k)
    for (int kmer : {1, 7, 12}) {
        const unsigned long long at = (unsigned long long)kmer * CM_MAX_SEEDS_PER_READ + kmer - 1, R[RES_WORDS] = {NO_BAD, NO_BAD, at, 40, 40}, R1[RES_WORDS] = {NO_BAD, NO_BAD, at + 1, 40, 40};
        const Verdict v = verdict(R, 3, 10, 300, kmer, CM_MAX_SEEDS_PER_READ), v1 = verdict(R1, 3, 10, 300, kmer, CM_MAX_SEEDS_PER_READ);
        ok &= v.what == ACCEPTED && v.code == CM_OK && v1.what == TOO_MANY_SEEDS && v1.code == CM_ELIMIT && v1.count == at + 1;
        ok &= !too_many_seeds((int)at, kmer, CM_MAX_SEEDS_PER_READ) && too_many_seeds((int)at + 1, kmer, CM_MAX_SEEDS_PER_READ);
    }
    return ok;
}
int main() {
    if (!boundaries()) { printf("verdict boundaries: FAILED\n"); return 1; }
    std::mt19937_64 rng(7);
    int ok = 0, bad = 0;
    for (int it = 0; it < 600; ++it) {
        int n1 = (int)(rng() % 300), n2 = rng() % 3 ? n1 : (int)(rng() % 300);
        std::string a = make(rng, n1, 1, it % 4 == 0), b = make(rng, n2, 2, it % 5 == 0);
        if (it % 7 == 0) { a.resize(a.size() * (rng() % 100) / 100); b.resize(std::min(b.size(), a.size())); }
        uint64_t mp = rng() % 400;
        uint64_t cap = std::min<uint64_t>(mp, std::min(a.size(), b.size()) / 4) + 1;
        // exact-size heap blocks, so that any read or write past an argument array is seen
        std::vector<uint8_t> ta(a.begin(), a.end()), tb2(b.begin(), b.end());
        uint8_t *s1 = (uint8_t *)malloc(a.size() + 1), *s2 = (uint8_t *)malloc(b.size() + 1);
        uint64_t *o1 = (uint64_t *)malloc(cap * 8), *o2 = (uint64_t *)malloc(cap * 8), *r1 = (uint64_t *)malloc(cap * 8), *r2 = (uint64_t *)malloc(cap * 8);
        cm_text_batch tb;
        unsigned long long res[16];
        int rc = emu_stage_text(ta.data(), ta.size(), tb2.data(), tb2.size(), mp, (uint32_t)(rng() % 4), 300, 20, it, s1, o1, r1, s2, o2, r2, &tb, res);
        (rc == 0 ? ok : bad)++;
        if (rc != 0 && rc != -1) { printf("unexpected rc %d at %d\n", rc, it); return 1; }
        free(s1); free(s2); free(o1); free(o2); free(r1); free(r2);
    }
    printf("sanitizer pass: %d accepted, %d refused\n", ok, bad);
    return 0;
}
