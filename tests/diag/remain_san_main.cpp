// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_remain_text.h and the plan of cm_rows_text.h through the host
// emulation (tests/hostemu_remain.cpp, tests/hostemu_rows.h):
// directed states (every printed field at the boundaries of its format; for the sort key gspos: contig_num -1, 0, 1, 15, INT32_MIN,
// INT32_MAX, spos_r1 + shift wrapping 2^32, chr_id -1 and n_chr, an empty chromosome table; every type 0 .. 13 and types outside)
// over reads of 0, 1, 150 and 300 bases and a run of long names in both files; the names of both files and the qualities through
// the tokeniser's bodies, out of the text; the selections all / none / every other / only the last / a third; whole sets and
// ranges, the window's rule, every span direct, and a small window; every argument array an exact-size heap block.  The records
// are compared with snprintf's, the keys with the formula.  CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc -I tests \
//       tests/diag/remain_san_main.cpp tests/hostemu_remain.cpp -o /tmp/remain_san && /tmp/remain_san
#include <cinttypes>
#include <cstdio>
#include <string>
#include "hostemu_rows.h"
using emu::exact;

extern "C" int emu_format_remain(const cm_mapped_read *states, uint64_t n_pairs, const uint32_t *sel, uint64_t n_sel, const uint8_t *names1,
                                 const uint32_t *name_off1, const uint8_t *names2, const uint32_t *name_off2, const uint8_t *seq1, const uint64_t *off1,
                                 const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs, uint32_t n_chr,
                                 uint64_t first, uint64_t count, uint8_t *out1, uint64_t cap1, uint8_t *out2, uint64_t cap2, uint64_t *out_bytes, int64_t *out_keys,
                                 uint64_t *n_records, uint64_t *stats, uint64_t seed, uint32_t window, uint64_t *writes);

static bool mapped(int32_t t) { return t == 0 || t == 1 || t == 2 || t == 3 || t == 4 || t == 5 || t == 7; }
static int64_t gspos(const cm_mapped_read &m, const cm_chr_info *chrs, int n_chr) {
    const uint32_t shift = m.chr_id >= 0 && m.chr_id < n_chr ? chrs[m.chr_id].start_pos : 0u;
    return (int64_t)((uint64_t)(int64_t)m.contig_num * 1100000000ull + (uint32_t)(m.spos_r1 + shift));
}
// the record of one mate, the plain way
static std::string printf_rec(const std::string &name, const cm_mapped_read &m, const std::string &seq, const std::string &qual, const cm_chr_info *chrs, int n_chr) {
    char buf[512];
    if (mapped(m.type)) {
        const char *cn = m.chr_id >= 0 && m.chr_id < n_chr ? chrs[m.chr_id].name : "-";
        snprintf(buf, sizeof buf, " %" PRId64 " %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d", gspos(m, chrs, n_chr), m.type, cn, m.spos_r1, m.epos_r1,
                 (int)m.mlen_r1, m.qspos_r1, m.qepos_r1, m.r1_forward ? '+' : '-', m.ed_r1, cn, m.spos_r2, m.epos_r2, (int)m.mlen_r2, m.qspos_r2, m.qepos_r2,
                 m.r2_forward ? '+' : '-', m.ed_r2, m.tlen, (int)m.junc_num, (int)(m.gm_compatible != 0), m.contig_num);
    } else snprintf(buf, sizeof buf, " * %d * * * * * * * * * * * * * * * * * * * *", m.type);
    return "@" + name + buf + "\n" + seq + "\n+\n" + qual + "\n";
}
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main() {
    const std::string forty(40, 'x');
    const cm_chr_info chrs[4] = {{"c", 1, 0, 1000}, {forty.c_str(), 1, 1000, 500}, {"chr2", 2, 0, 70000}, {"7", 2, 70000, 10}};
    const int32_t contigs[7] = {-1, 0, 1, 15, INT32_MIN, INT32_MAX, 2};
    const uint32_t lens[6] = {0, 1, 150, 300, 0, 150};
    std::mt19937_64 rng(17);
    uint64_t recs_checked = 0, staged = 0, direct = 0, wrapped = 0, wide_keys = 0;
    for (uint32_t n : {1u, 15u, 16u, 17u, 65u, 740u}) {
        std::vector<std::string> name[2], seq[2], qual[2];
        std::string text[2];
        for (int f = 0; f < 2; ++f) {
            name[f].resize(n);
            seq[f].resize(n);
            qual[f].resize(n);
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t len = 30 + rng() % 121;
                if ((i + 5 * f) % 13 < 6) len = lens[(i + 5 * f) % 13];
                for (uint32_t k = 0; k < len; ++k) {
                    seq[f][i] += "ACGTNacgt"[rng() % 9];
                    qual[f][i] += (char)(33 + rng() % 41);
                }
                const size_t nl = (n >= 64 && i >= n / 2 && i < n / 2 + 40) ? 300 + rng() % 101 : (i % 17 == 3 + (uint32_t)f ? 0 : rng() % 30 + (size_t)f * (i % 7));
                for (size_t k = 0; k < nl; ++k) name[f][i] += (char)((f ? 'A' : 'a') + rng() % 26);
                std::string header = "@" + name[f][i] + (nl ? (f ? "/2" : "/1") : "") + (nl && i % 3 == 0 ? "  a comment" : "");       // (nl == 0: no token, an empty name)
                if (i % 19 == 7 && nl > 2) {                                  // a NUL inside the token: the name ends there
                    header = "@" + name[f][i].substr(0, 2) + std::string(1, '\0') + name[f][i].substr(2) + "/1";
                    name[f][i] = name[f][i].substr(0, 2);
                }
                text[f] += header + "\n" + seq[f][i] + "\n+\n" + qual[f][i] + "\n";
            }
        }
        // names and qualities of both files through the tokeniser's bodies, out of the text
        std::vector<uint8_t> s[2];
        std::vector<uint64_t> off[2] = {{0ull}, {0ull}};
        uint8_t *p_names[2], *p_q[2], *p_s[2];
        uint32_t *p_noff[2];
        uint64_t *p_off[2];
        for (int f = 0; f < 2; ++f) {
            for (uint32_t i = 0; i < n; ++i) {
                s[f].insert(s[f].end(), seq[f][i].begin(), seq[f][i].end());
                off[f].push_back(s[f].size());
            }
            p_s[f] = exact(s[f]);
            p_off[f] = exact(off[f]);
            const std::vector<uint8_t> t(text[f].begin(), text[f].end());
            uint8_t *pt = exact(t);
            std::vector<uint8_t> nm(t.size() + 1, 0xa5);
            std::vector<uint32_t> no(n + 1, 0u);
            if (emu_names(pt, t.size(), n, n + f, nm.data(), no.data()) != CM_OK) FAIL("emu_names failed at n = %u", n);
            for (uint32_t i = 0; i < n; ++i)
                if (std::string((const char *)nm.data() + no[i], no[i + 1] - no[i]) != name[f][i]) FAIL("name %u of file %d, n = %u differs", i, f + 1, n);
            nm.resize(no[n]);
            p_names[f] = exact(nm);
            p_noff[f] = exact(no);
            p_q[f] = (uint8_t *)malloc(off[f][n] ? off[f][n] : 1);
            if (emu_quals(pt, t.size(), n, p_off[f], n + f, p_q[f]) != CM_OK) FAIL("emu_quals failed at n = %u", n);
            for (uint32_t i = 0; i < n; ++i)
                if (memcmp(p_q[f] + off[f][i], qual[f][i].data(), qual[f][i].size()) != 0) FAIL("quality %u of file %d, n = %u differs", i, f + 1, n);
            free(pt);
        }
        std::vector<cm_mapped_read> stv(n);
        for (uint32_t i = 0; i < n; ++i) {
            stv[i] = emu::directed_state(i, 4, false);
            stv[i].contig_num = contigs[i % 7];
            const int32_t ids[4] = {-1, 0, 3, 4};
            stv[i].chr_id = ids[(i / 8) % 4];
            if (mapped(stv[i].type) && stv[i].chr_id == 3 && stv[i].spos_r1 == 4294967295u) ++wrapped;
            if (mapped(stv[i].type) && (stv[i].contig_num == INT32_MIN || stv[i].contig_num == INT32_MAX)) ++wide_keys;
        }
        cm_mapped_read *st = exact(stv);
        std::vector<std::vector<uint32_t>> sels(5);
        for (uint32_t i = 0; i < n; ++i) {
            sels[0].push_back(i);
            if (i % 2 == 0) sels[2].push_back(i);
            if (rng() % 3 == 0) sels[4].push_back(i);
        }
        sels[3].push_back(n - 1);
        for (const auto &selv : sels) {
            uint32_t *sel = exact(selv);
            const uint64_t k = selv.size();
            const uint64_t ranges[][2] = {{0, ~0ull}, {k / 3, k - k / 3}, {k ? 15 % k : 0, k ? (k - 15 % k < 2 ? k - 15 % k : 2) : 0}, {k, 0}, {k ? k - 1 : 0, k ? 1ull : 0ull}};
            for (const auto &r : ranges)
                for (int n_chr : {4, 0})
                    for (uint32_t window : {0u, 1u, 3000u}) {
                        const uint64_t c = r[1] == ~0ull ? k - r[0] : r[1];
                        std::string ref[2];
                        std::vector<int64_t> want_keys;
                        for (uint64_t q = r[0]; q < r[0] + c; ++q) {
                            const uint32_t i = selv[q];
                            for (int f = 0; f < 2; ++f) ref[f] += printf_rec(name[f][i], st[i], seq[f][i], qual[f][i], chrs, n_chr);
                            want_keys.push_back(mapped(st[i].type) ? gspos(st[i], chrs, n_chr) : 0);
                        }
                        uint64_t got[2] = {7, 7}, n_rec = 0, stats[4], writes[2] = {0, 0};
                        const int rc0 = emu_format_remain(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1], chrs,
                                                          (uint32_t)n_chr, r[0], r[1], nullptr, 0, nullptr, 0, got, nullptr, &n_rec, nullptr, 5, window, nullptr);
                        if (got[0] != ref[0].size() || got[1] != ref[1].size() || n_rec != k || rc0 != (c ? CM_ELIMIT : CM_OK))
                            FAIL("sizes of range [%llu, +%llu) of %llu of %u differ (rc %d)", (unsigned long long)r[0], (unsigned long long)c, (unsigned long long)k, n, rc0);
                        uint8_t *out[2] = {(uint8_t *)malloc(ref[0].size() ? ref[0].size() : 1), (uint8_t *)malloc(ref[1].size() ? ref[1].size() : 1)};
                        int64_t *keys = (int64_t *)malloc(c ? c * sizeof(int64_t) : 1);
                        const int rc = emu_format_remain(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1], chrs,
                                                         (uint32_t)n_chr, r[0], r[1], out[0], ref[0].size(), out[1], ref[1].size(), got, keys, &n_rec, stats, n + r[0], window, writes);
                        if (rc != CM_OK || memcmp(out[0], ref[0].data(), ref[0].size()) != 0 || memcmp(out[1], ref[1].data(), ref[1].size()) != 0)
                            FAIL("records of range [%llu, +%llu) of %llu of %u differ (rc %d, window %u)", (unsigned long long)r[0], (unsigned long long)c, (unsigned long long)k, n, rc, window);
                        if (c && (writes[0] != 1 || writes[1] != 1)) FAIL("a byte written %llu .. %llu times", (unsigned long long)writes[0], (unsigned long long)writes[1]);
                        if (c && memcmp(keys, want_keys.data(), c * sizeof(int64_t)) != 0) FAIL("keys of range [%llu, +%llu) of %u differ", (unsigned long long)r[0], (unsigned long long)c, n);
                        recs_checked += 2 * c;
                        if (c) staged += stats[2], direct += stats[3];
                        free(keys);
                        free(out[0]);
                        free(out[1]);
                    }
            free(sel);
        }
        free(st);
        for (int f = 0; f < 2; ++f) {
            free(p_q[f]);
            free(p_off[f]);
            free(p_noff[f]);
            free(p_names[f]);
            free(p_s[f]);
        }
    }
    if (!staged || !direct || !wrapped || !wide_keys)
        FAIL("a case was never met (%llu staged, %llu direct, %llu wrapped, %llu wide keys)", (unsigned long long)staged, (unsigned long long)direct, (unsigned long long)wrapped, (unsigned long long)wide_keys);
    printf("sanitizer pass: %llu records equal snprintf's, %llu spans staged, %llu direct, %llu states whose sum wraps, %llu with 20-byte keys\n",
           (unsigned long long)recs_checked, (unsigned long long)staged, (unsigned long long)direct, (unsigned long long)wrapped, (unsigned long long)wide_keys);
    return 0;
}
