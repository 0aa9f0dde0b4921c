// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_pam_text.h through the host emulation (tests/hostemu_pam.cpp):
// the directed states of tests/pam_text_util.py (every printed field at the boundaries of its format) over names that cover the
// parser's rules and a run of long names, whole batches and ranges, every argument array an exact-size heap block; the rows are
// also compared with printf's.  CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc \
//       tests/diag/pam_san_main.cpp tests/hostemu_pam.cpp -o /tmp/pam_san && /tmp/pam_san
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "circminer_hot.h"
extern "C" int emu_names(const uint8_t *, uint64_t, uint32_t, uint64_t, uint8_t *, uint32_t *);
extern "C" int emu_format_pam(const cm_mapped_read *, uint64_t, const uint8_t *, const uint32_t *, const cm_chr_info *, uint32_t, uint64_t, uint64_t, uint8_t *,
                              uint64_t, uint64_t *, uint64_t *, uint64_t);

static const uint32_t U32V[] = {0u, 9u, 10u, 99u, 100u, 999999999u, 1000000000u, 4294967295u};
static const uint32_t MLENV[] = {0u, 9u, 10u, 99u, 100u, 999999999u, 1000000000u, 4294967295u, 2147483648u};
static const int32_t INTV[] = {0, -1, -9, -10, INT_MIN, INT_MAX, 1000000000};
static const int32_t TYPEV[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, -1, 14, -9, -10, INT_MIN, INT_MAX, 1000000000, 100, 13};

static cm_mapped_read directed(uint32_t i, int n_chr) {
    cm_mapped_read m;
    memset(&m, 0xee, sizeof m);
    m.type = TYPEV[i % 23];
    uint32_t *u[8] = {&m.spos_r1, &m.spos_r2, &m.epos_r1, &m.epos_r2, &m.qspos_r1, &m.qspos_r2, &m.qepos_r1, &m.qepos_r2};
    for (uint32_t j = 0; j < 8; ++j) *u[j] = U32V[(i + j) % 8];
    m.mlen_r1 = MLENV[i % 9];
    m.mlen_r2 = MLENV[(i + 4) % 9];
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
static bool mapped(int t) { return t == 0 || t == 1 || t == 2 || t == 3 || t == 4 || t == 5 || t == 7; }
static std::string printf_row(const std::string &name, const cm_mapped_read &m, const cm_chr_info *chrs, int n_chr) {
    char buf[1024];
    if (!mapped(m.type)) {
        std::string r = name;
        for (int k = 0; k < 21; ++k) r += "\t*";
        snprintf(buf, sizeof buf, "\t%d\n", m.type);
        return r + buf;
    }
    const char *cn = m.chr_id >= 0 && m.chr_id < n_chr ? chrs[m.chr_id].name : "-";
    snprintf(buf, sizeof buf, "\t%s\t%u\t%u\t%d\t%u\t%u\t%c\t%d\t%s\t%u\t%u\t%d\t%u\t%u\t%c\t%d\t%d\t%d\t%d\t%d\n", cn, m.spos_r1, m.epos_r1, (int)m.mlen_r1,
             m.qspos_r1, m.qepos_r1, m.r1_forward ? '+' : '-', m.ed_r1, cn, m.spos_r2, m.epos_r2, (int)m.mlen_r2, m.qspos_r2, m.qepos_r2,
             m.r2_forward ? '+' : '-', m.ed_r2, m.tlen, (int)m.junc_num, (int)(m.gm_compatible != 0), m.type);
    return name + buf;
}

int main() {
    const std::string forty(40, 'x');
    const cm_chr_info chrs[4] = {{"c", 1, 0, 1000}, {forty.c_str(), 1, 1000, 500}, {"chr2", 2, 0, 70000}, {"7", 2, 70000, 10}};
    // (header, the name the host parser keeps)
    const std::pair<std::string, std::string> special[] = {{"@", ""},       {"@   ", ""},           {"@/1", ""},     {"@a/1", "a"},       {"@q", "q"},
                                                           {"@ta\tb/1 c", "ta\tb"}, {std::string("@nu\0l/1", 7), "nu"}, {"@  lead  two", "lead"},
                                                           {"@x/", "x/"},   {"@a/b/2", "a/b"},      {"@//", ""},     {std::string("@\0", 2), ""}};
    std::mt19937_64 rng(11);
    uint64_t rows_checked = 0, staged = 0, direct = 0;
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 130u, 700u}) {
        std::string text;
        std::vector<std::string> want;
        for (uint32_t i = 0; i < n; ++i) {
            std::string h, nm;
            if (i % 9 == 4) {
                h = special[(i / 9) % 12].first;
                nm = special[(i / 9) % 12].second;
            } else {
                const size_t len = (n >= 64 && i >= n / 2 && i < n / 2 + 90) ? 300 + rng() % 101 : 1 + rng() % 30;
                for (size_t k = 0; k < len; ++k) nm += (char)('a' + rng() % 26);
                h = "@" + nm + (i % 2 ? "/1" : "") + (i % 3 ? "" : "  1:N:0 x");
            }
            want.push_back(nm);
            text += h + "\nACGT\n+\nIIII\n";
        }
        if (n % 2) text.pop_back();                                   // a last line without a line feed
        // exact-size heap blocks, so that any read or write past an argument array is seen
        uint8_t *t = (uint8_t *)malloc(text.size());
        memcpy(t, text.data(), text.size());
        size_t name_bytes = 0;
        for (const std::string &s : want) name_bytes += s.size();
        uint8_t *names = (uint8_t *)malloc(name_bytes ? name_bytes : 1);
        uint32_t *off = (uint32_t *)malloc((n + 1) * sizeof(uint32_t));
        if (emu_names(t, text.size(), n, n, names, off) != CM_OK) { printf("emu_names failed at n = %u\n", n); return 1; }
        for (uint32_t i = 0; i < n; ++i)
            if (std::string((const char *)names + off[i], off[i + 1] - off[i]) != want[i]) { printf("name %u of %u differs\n", i, n); return 1; }
        cm_mapped_read *st = (cm_mapped_read *)malloc(n * sizeof(cm_mapped_read));
        for (uint32_t i = 0; i < n; ++i) st[i] = directed(i, 4);
        const uint64_t ranges[][2] = {{0, n}, {n / 3, n - n / 3}, {63 % n, (uint64_t)(n - 63 % n < 2 ? n - 63 % n : 2)}, {n, 0}, {n - 1, 1}};
        for (const auto &r : ranges)
            for (int n_chr : {4, 0}) {
                std::string ref;
                for (uint64_t i = r[0]; i < r[0] + r[1]; ++i) ref += printf_row(want[i], st[i], chrs, n_chr);
                uint64_t got = 0, stats[4];
                const int rc0 = emu_format_pam(st, n, names, off, chrs, (uint32_t)n_chr, r[0], r[1], nullptr, 0, &got, nullptr, 5);
                if (got != ref.size() || rc0 != (ref.empty() ? CM_OK : CM_ELIMIT)) { printf("size of range [%llu, +%llu) of %u differs\n", (unsigned long long)r[0], (unsigned long long)r[1], n); return 1; }
                uint8_t *out = (uint8_t *)malloc(ref.size() ? ref.size() : 1);
                if (emu_format_pam(st, n, names, off, chrs, (uint32_t)n_chr, r[0], r[1], out, ref.size(), &got, stats, n + r[0]) != CM_OK ||
                    memcmp(out, ref.data(), ref.size()) != 0) {
                    printf("rows of range [%llu, +%llu) of %u differ\n", (unsigned long long)r[0], (unsigned long long)r[1], n);
                    return 1;
                }
                rows_checked += r[1];
                staged += stats[2];
                direct += stats[3];
                free(out);
            }
        free(st);
        free(off);
        free(names);
        free(t);
    }
    if (!staged || !direct) { printf("a path of the row kernel was never taken (%llu staged, %llu direct)\n", (unsigned long long)staged, (unsigned long long)direct); return 1; }
    printf("sanitizer pass: %llu rows equal printf's, %llu spans staged, %llu direct\n", (unsigned long long)rows_checked, (unsigned long long)staged,
           (unsigned long long)direct);
    return 0;
}
