// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_fastq_text.h through the host emulation (tests/hostemu_fastq.cpp):
// random file pairs, some malformed, some cut, every argument array an exact-size heap block.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc \
//       tests/diag/fastq_san_main.cpp tests/hostemu_fastq.cpp -o /tmp/fastq_san && /tmp/fastq_san
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "circminer_hot.h"
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
int main() {
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
