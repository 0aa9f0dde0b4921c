// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_pam_text.h and the plan of cm_rows_text.h through the host
// emulation (tests/hostemu_pam.cpp, tests/hostemu_rows.h): the directed states of tests/pam_text_util.py (every printed field at the
// boundaries of its format) over names that cover the parser's rules and a run of long names, whole batches and ranges, the
// window's rule, every span direct, and a small window; every argument array an exact-size heap block; the rows are also compared
// with printf's.  CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc -I tests \
//       tests/diag/pam_san_main.cpp tests/hostemu_pam.cpp -o /tmp/pam_san && /tmp/pam_san
#include <cstdio>
#include <string>
#include "hostemu_rows.h"

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
        for (uint32_t i = 0; i < n; ++i) st[i] = emu::directed_state(i, 4, false);
        const uint64_t ranges[][2] = {{0, n}, {n / 3, n - n / 3}, {63 % n, (uint64_t)(n - 63 % n < 2 ? n - 63 % n : 2)}, {n, 0}, {n - 1, 1}};
        for (const auto &r : ranges)
            for (int n_chr : {4, 0})
                for (uint32_t window : {0u, 1u, 3000u}) {
                    std::string ref;
                    for (uint64_t i = r[0]; i < r[0] + r[1]; ++i) ref += printf_row(want[i], st[i], chrs, n_chr);
                    uint64_t got = 0, stats[4], writes[3] = {0, 0, 0};
                    const int rc0 = emu_format_pam(st, n, names, off, chrs, (uint32_t)n_chr, r[0], r[1], nullptr, 0, &got, nullptr, 5, window, nullptr, nullptr);
                    if (got != ref.size() || rc0 != (ref.empty() ? CM_OK : CM_ELIMIT)) { printf("size of range [%llu, +%llu) of %u differs\n", (unsigned long long)r[0], (unsigned long long)r[1], n); return 1; }
                    uint8_t *out = (uint8_t *)malloc(ref.size() ? ref.size() : 1);
                    const int rc = emu_format_pam(st, n, names, off, chrs, (uint32_t)n_chr, r[0], r[1], out, ref.size(), &got, stats, n + r[0], window, nullptr, writes);
                    if (rc != CM_OK || memcmp(out, ref.data(), ref.size()) != 0) {
                        printf("rows of range [%llu, +%llu) of %u differ (rc %d, window %u)\n", (unsigned long long)r[0], (unsigned long long)r[1], n, rc, window);
                        return 1;
                    }
                    if (r[1] && (writes[0] != 1 || writes[1] != 1 || writes[2] != 0)) { printf("a byte written %llu .. %llu times, %llu rows of another length\n", (unsigned long long)writes[0], (unsigned long long)writes[1], (unsigned long long)writes[2]); return 1; }
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
