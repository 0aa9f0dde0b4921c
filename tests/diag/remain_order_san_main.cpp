// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_remain_order.h through the host emulation
// (tests/hostemu_remain_order.cpp) and over the merge of sorted runs (cm_remain_runs, circminer_amd/csrc/host_circ.cpp):
// tie groups of 1, 2, 16, 17, 64 and 65 members scattered over the batch, whose members differ in the name (a prefix, a byte below
// 0x20, one above 0x7f), in the fields (a mapped 0 among star forms), in the bases (a shorter read among them), in the qualities or
// nowhere, the other way round in file 2; keys that are negative, beyond 2^32 and 20 bytes long; reads of 0, 1, 150 and 300 bases;
// chromosome names of 1 and 40 bytes; whole sets, ranges that cut a group, a lowered cap at its boundary; every argument array an
// exact-size heap block.  The order is compared with std::stable_sort over snprintf's records (key, then the pasted line), the merge
// of 1, 2 and 7 runs -- empty ones and a run of one record among them, every other one handed over unsorted -- with the same.
// CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc -I tests \
//       tests/diag/remain_order_san_main.cpp tests/hostemu_remain_order.cpp circminer_amd/csrc/host_circ.cpp -o /tmp/remain_order_san && /tmp/remain_order_san
#include <cinttypes>
#include <cstdio>
#include <string>
#include "hostemu_rows.h"
using emu::exact;

extern "C" int emu_format_remain_sorted(const cm_mapped_read *states, uint64_t n_pairs, const uint32_t *sel, uint64_t n_sel, const uint8_t *names1,
                                        const uint32_t *name_off1, const uint8_t *names2, const uint32_t *name_off2, const uint8_t *seq1, const uint64_t *off1,
                                        const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs,
                                        uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out1, uint64_t cap1, uint8_t *out2, uint64_t cap2,
                                        uint64_t *out_bytes, int64_t *out_keys, uint32_t *out_off1, uint32_t *out_off2, uint64_t *n_records, uint64_t *stats,
                                        uint64_t seed, uint32_t window, uint32_t tie_cap, uint32_t *tie_stats);

static bool mapped(int32_t t) { return t == 0 || t == 1 || t == 2 || t == 3 || t == 4 || t == 5 || t == 7; }
static int64_t key(const cm_mapped_read &m, const cm_chr_info *chrs, int n_chr) {
    if (!mapped(m.type)) return 0;
    const uint32_t shift = m.chr_id >= 0 && m.chr_id < n_chr ? chrs[m.chr_id].start_pos : 0u;
    return (int64_t)((uint64_t)(int64_t)m.contig_num * 1100000000ull + (uint32_t)(m.spos_r1 + shift));
}
static std::string printf_rec(const std::string &name, const cm_mapped_read &m, const std::string &seq, const std::string &qual, const cm_chr_info *chrs, int n_chr) {
    char buf[512];
    if (mapped(m.type)) {
        const char *cn = m.chr_id >= 0 && m.chr_id < n_chr ? chrs[m.chr_id].name : "-";
        snprintf(buf, sizeof buf, " %" PRId64 " %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d", key(m, chrs, n_chr), m.type, cn, m.spos_r1, m.epos_r1,
                 (int)m.mlen_r1, m.qspos_r1, m.qepos_r1, m.r1_forward ? '+' : '-', m.ed_r1, cn, m.spos_r2, m.epos_r2, (int)m.mlen_r2, m.qspos_r2, m.qepos_r2,
                 m.r2_forward ? '+' : '-', m.ed_r2, m.tlen, (int)m.junc_num, (int)(m.gm_compatible != 0), m.contig_num);
    } else snprintf(buf, sizeof buf, " * %d * * * * * * * * * * * * * * * * * * * *", m.type);
    return "@" + name + buf + "\n" + seq + "\n+\n" + qual + "\n";
}
// the line `paste - - - -` makes of a record
static std::string pasted(const std::string &rec) {
    std::string p = rec.substr(0, rec.size() - 1);
    for (char &c : p)
        if (c == '\n') c = '\t';
    return p;
}
static bool pasted_less(const std::string &a, const std::string &b) {
    return std::lexicographical_compare((const unsigned char *)a.data(), (const unsigned char *)a.data() + a.size(), (const unsigned char *)b.data(),
                                        (const unsigned char *)b.data() + b.size());
}
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main() {
    const std::string forty(40, 'x');
    const cm_chr_info chrs[4] = {{"c", 1, 0, 1000}, {forty.c_str(), 1, 1000, 500}, {"chr2", 2, 0, 70000}, {"7", 2, 70000, 10}};
    const int32_t contigs[7] = {-1, 0, 1, 15, INT32_MIN, INT32_MAX, 2};
    const uint32_t sizes6[6] = {65, 64, 17, 16, 2, 1};
    std::mt19937_64 rng(23);
    uint64_t calls = 0, recs_checked = 0, tied_groups = 0, refusals = 0, merges = 0, orders_differ = 0;
    for (uint32_t n : {1u, 2u, 65u, 700u}) {
        // the groups and their members' places
        std::vector<uint32_t> sizes, place = emu::shuffled(n, rng);
        for (uint32_t k = 0, sum = 0; sum < n; ++k) {
            sizes.push_back(std::min(sizes6[k % 6], n - sum));
            sum += sizes.back();
        }
        std::vector<std::string> name[2], seq[2], qual[2];
        for (int f = 0; f < 2; ++f) name[f].resize(n), seq[f].resize(n), qual[f].resize(n);
        std::vector<cm_mapped_read> stv(n);
        uint32_t at = 0;
        for (uint32_t g = 0; g < sizes.size(); ++g) {
            std::vector<uint32_t> members(place.begin() + at, place.begin() + at + sizes[g]);
            std::sort(members.begin(), members.end());
            at += sizes[g];
            cm_mapped_read lead = emu::directed_state(g, 4, false), other;
            if (g == 0) lead.type = 8;
            else {
                const int32_t types[7] = {0, 1, 2, 3, 4, 5, 7}, ids[5] = {-1, 0, 3, 4, 1};
                lead.type = types[g % 7];
                lead.contig_num = contigs[g % 7];
                lead.chr_id = ids[g % 5];
                lead.spos_r1 = g == 3 ? 4294967295u : g * 100000u + 7u;
                if (g == 3) lead.chr_id = 3;
            }
            other = lead;
            if (g == 0) other.type = 4, other.contig_num = 0, other.spos_r1 = 0, other.chr_id = -1;
            else other.epos_r2 ^= 1u;
            const uint32_t lens[4] = {0, 1, 150, 300}, len = g < 4 ? lens[g] : 2 + (uint32_t)(rng() % 299);
            std::string own_seq[2], own_qual[2];
            for (int f = 0; f < 2; ++f)
                for (uint32_t k = 0; k < len; ++k) own_seq[f] += "ACGTNacgt"[rng() % 9], own_qual[f] += (char)(33 + rng() % 41);
            for (uint32_t j = 0; j < members.size(); ++j) {
                const uint32_t p = members[j];
                stv[p] = (j % 8 == 3 || j % 8 == 4) ? other : lead;
                for (int f = 0; f < 2; ++f) {
                    const uint32_t c = f ? 7 - j % 8 : j % 8;
                    std::string nm = (f ? "h" : "g") + std::to_string(g), s = own_seq[f], q = own_qual[f];
                    if (c >= 1 && c <= 3) nm += std::string(1, "x\x01\xfe"[c - 1]) + (j >= 8 ? std::to_string(j) : "");
                    if (c == 5 && len) {
                        if (g % 2) s = s.substr(0, len / 2), q = q.substr(0, len / 2);
                        else s.back() = s.back() == 'A' ? 'C' : 'A';
                    }
                    if (c == 6 && len) q.back() = q.back() == '!' ? '#' : '!';
                    name[f][p] = nm, seq[f][p] = s, qual[f][p] = q;
                }
            }
        }
        // the arrays as the device holds them
        uint8_t *p_names[2], *p_s[2], *p_q[2];
        uint32_t *p_noff[2];
        uint64_t *p_off[2];
        for (int f = 0; f < 2; ++f) {
            std::vector<uint8_t> nm, s, q;
            std::vector<uint32_t> no{0u};
            std::vector<uint64_t> off{0ull};
            for (uint32_t i = 0; i < n; ++i) {
                nm.insert(nm.end(), name[f][i].begin(), name[f][i].end());
                no.push_back((uint32_t)nm.size());
                s.insert(s.end(), seq[f][i].begin(), seq[f][i].end());
                q.insert(q.end(), qual[f][i].begin(), qual[f][i].end());
                off.push_back(s.size());
            }
            p_names[f] = exact(nm), p_noff[f] = exact(no), p_s[f] = exact(s), p_q[f] = exact(q), p_off[f] = exact(off);
        }
        cm_mapped_read *st = exact(stv);
        std::vector<std::vector<uint32_t>> sels(2);
        for (uint32_t i = 0; i < n; ++i) {
            sels[0].push_back(i);
            if (rng() % 3 != 0) sels[1].push_back(i);
        }
        for (const auto &selv : sels) {
            const uint64_t k = selv.size();
            if (!k) continue;
            uint32_t *sel = exact(selv);
            // the reference order of either file
            std::vector<std::string> ref[2];
            std::vector<int64_t> ref_keys;
            std::vector<uint32_t> ord[2];
            for (int f = 0; f < 2; ++f) {
                std::vector<uint32_t> idx(selv);
                std::vector<std::string> line(n);
                for (uint32_t i : selv) line[i] = pasted(printf_rec(name[f][i], st[i], seq[f][i], qual[f][i], chrs, 4));
                std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
                    const int64_t ka = key(st[a], chrs, 4), kb = key(st[b], chrs, 4);
                    return ka != kb ? ka < kb : pasted_less(line[a], line[b]);
                });
                for (uint32_t i : idx) ref[f].push_back(printf_rec(name[f][i], st[i], seq[f][i], qual[f][i], chrs, 4));
                if (f == 0)
                    for (uint32_t i : idx) ref_keys.push_back(key(st[i], chrs, 4));
                ord[f] = idx;
            }
            orders_differ += ord[0] != ord[1];
            uint32_t cut = 0;                                        // a place inside a tie group, if there is one
            for (uint32_t i = 1; i < k; ++i)
                if (ref_keys[i] == ref_keys[i - 1]) cut = i;
            const uint64_t ranges[][2] = {{0, ~0ull}, {cut, std::min<uint64_t>(3, k - cut)}, {0, cut}, {k, 0}};
            for (const auto &r : ranges)
                for (uint32_t window : {0u, 1u}) {
                    const uint64_t c = r[1] == ~0ull ? k - r[0] : r[1];
                    std::string want[2];
                    for (int f = 0; f < 2; ++f)
                        for (uint64_t q = r[0]; q < r[0] + c; ++q) want[f] += ref[f][q];
                    uint8_t *out[2] = {(uint8_t *)malloc(want[0].size() ? want[0].size() : 1), (uint8_t *)malloc(want[1].size() ? want[1].size() : 1)};
                    int64_t *keys = (int64_t *)malloc(c ? c * sizeof(int64_t) : 1);
                    uint32_t *off[2] = {(uint32_t *)malloc((c + 1) * 4), (uint32_t *)malloc((c + 1) * 4)}, ties[3];
                    uint64_t got[2] = {7, 7}, n_rec = 0, stats[4];
                    const int rc = emu_format_remain_sorted(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1],
                                                            chrs, 4, r[0], r[1], out[0], want[0].size(), out[1], want[1].size(), got, keys, off[0], off[1], &n_rec, stats,
                                                            n + r[0], window, 0, ties);
                    if (rc != CM_OK || n_rec != k || got[0] != want[0].size() || got[1] != want[1].size() || memcmp(out[0], want[0].data(), want[0].size()) != 0 ||
                        memcmp(out[1], want[1].data(), want[1].size()) != 0)
                        FAIL("records of range [%llu, +%llu) of %llu of %u differ (rc %d, window %u)", (unsigned long long)r[0], (unsigned long long)c, (unsigned long long)k, n, rc, window);
                    if (c && memcmp(keys, ref_keys.data() + r[0], c * sizeof(int64_t)) != 0) FAIL("keys of range [%llu, +%llu) of %u differ", (unsigned long long)r[0], (unsigned long long)c, n);
                    for (int f = 0; f < 2 && c; ++f) {
                        uint32_t run = 0;
                        for (uint64_t q = 0; q <= c; ++q) {
                            if (off[f][q] != run) FAIL("offset %llu of file %d differs", (unsigned long long)q, f + 1);
                            if (q < c) run += (uint32_t)ref[f][r[0] + q].size();
                        }
                    }
                    ++calls;
                    recs_checked += 2 * c;
                    if (c) tied_groups += ties[1];
                    for (void *p : {(void *)out[0], (void *)out[1], (void *)keys, (void *)off[0], (void *)off[1]}) free(p);
                }
            // the cap at the largest group and one below it
            uint32_t ties[3] = {0, 0, 0};
            uint64_t got[2], n_rec = 0;
            (void)emu_format_remain_sorted(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1], chrs, 4, 0, ~0ull,
                                           nullptr, 0, nullptr, 0, got, nullptr, nullptr, nullptr, &n_rec, nullptr, 3, 0, 0, ties);
            if (ties[0] >= 2) {
                const int at_cap = emu_format_remain_sorted(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1], chrs, 4,
                                                            0, ~0ull, nullptr, 0, nullptr, 0, got, nullptr, nullptr, nullptr, &n_rec, nullptr, 3, 0, ties[0], nullptr);
                if (at_cap != CM_ELIMIT || !got[0]) FAIL("a group at the cap was not sized (rc %d)", at_cap);
                const int above = emu_format_remain_sorted(st, n, sel, k, p_names[0], p_noff[0], p_names[1], p_noff[1], p_s[0], p_off[0], p_s[1], p_off[1], p_q[0], p_q[1], chrs, 4,
                                                           0, ~0ull, nullptr, 0, nullptr, 0, got, nullptr, nullptr, nullptr, &n_rec, nullptr, 3, 0, ties[0] - 1, nullptr);
                if (above != CM_ELIMIT || got[0] || got[1] || n_rec != k) FAIL("a group above the cap was not refused (rc %d)", above);
                ++refusals;
            }
            // the merge: the set cut into runs where it stands, every other run handed over unsorted
            for (const std::vector<uint64_t> &cuts : {std::vector<uint64_t>{}, std::vector<uint64_t>{k / 2}, std::vector<uint64_t>{0, 1 % k, 1 % k, k / 3, k / 3 + 1 <= k ? k / 3 + 1 : k, k}}) {
                std::vector<uint64_t> b{0};
                b.insert(b.end(), cuts.begin(), cuts.end());
                b.push_back(k);
                std::sort(b.begin(), b.end());
                const char *paths[2] = {"/tmp/remain_order_san_R1.srt", "/tmp/remain_order_san_R2.srt"};
                cm_remain_runs *runs = nullptr;
                if (cm_remain_runs_open(paths[0], paths[1], &runs) != CM_OK) FAIL("cm_remain_runs_open failed");
                for (size_t x = 0; x + 1 < b.size(); ++x) {
                    std::string bytes[2];
                    std::vector<uint32_t> off[2] = {{0u}, {0u}};
                    std::vector<int64_t> keys;
                    const bool unsorted = x % 2 == 1;
                    for (int f = 0; f < 2; ++f) {
                        std::vector<uint32_t> idx;                   // the members of the run in the reference order, or as they stand
                        if (unsorted) idx.assign(selv.begin() + b[x], selv.begin() + b[x + 1]);
                        else
                            for (uint32_t i : ord[f])
                                if (std::find(selv.begin() + b[x], selv.begin() + b[x + 1], i) != selv.begin() + b[x + 1]) idx.push_back(i);
                        for (uint32_t i : idx) {
                            bytes[f] += printf_rec(name[f][i], st[i], seq[f][i], qual[f][i], chrs, 4);
                            off[f].push_back((uint32_t)bytes[f].size());
                            if (f == 0) keys.push_back(key(st[i], chrs, 4));
                        }
                    }
                    uint8_t *pb[2] = {exact(std::vector<uint8_t>(bytes[0].begin(), bytes[0].end())), exact(std::vector<uint8_t>(bytes[1].begin(), bytes[1].end()))};
                    uint32_t *po[2] = {exact(off[0]), exact(off[1])};
                    int64_t *pk = exact(keys);
                    const int rc = unsorted ? cm_remain_runs_add_unsorted(runs, pb[0], bytes[0].size(), pb[1], bytes[1].size())
                                            : cm_remain_runs_add(runs, pb[0], po[0], pb[1], po[1], pk, keys.size());
                    for (void *p : {(void *)pb[0], (void *)pb[1], (void *)po[0], (void *)po[1], (void *)pk}) free(p);
                    if (rc != CM_OK) FAIL("adding run %zu of %zu failed (%d)", x, b.size() - 1, rc);
                }
                if (cm_remain_runs_finish(runs) != CM_OK) FAIL("cm_remain_runs_finish failed");
                cm_remain_runs_close(runs);
                for (int f = 0; f < 2; ++f) {
                    std::string want, have;
                    for (const std::string &r : ref[f]) want += r;
                    FILE *fp = fopen(paths[f], "rb");
                    char buf[65536];
                    for (size_t got_n; fp && (got_n = fread(buf, 1, sizeof buf, fp)) > 0;) have.append(buf, got_n);
                    if (fp) fclose(fp);
                    remove(paths[f]);
                    if (have != want) FAIL("the merge of %zu runs of %llu records differs in file %d", b.size() - 1, (unsigned long long)k, f + 1);
                }
                ++merges;
            }
            free(sel);
        }
        free(st);
        for (int f = 0; f < 2; ++f)
            for (void *p : {(void *)p_names[f], (void *)p_noff[f], (void *)p_s[f], (void *)p_q[f], (void *)p_off[f]}) free(p);
    }
    if (!tied_groups || !refusals || !orders_differ) FAIL("a case was never met (%llu tied groups, %llu refusals, %llu sets the files order differently)",
                                                          (unsigned long long)tied_groups, (unsigned long long)refusals, (unsigned long long)orders_differ);
    printf("sanitizer pass: %llu calls, %llu records in std::stable_sort's order, %llu tied groups ranked, %llu refusals at the cap, %llu merges of runs\n",
           (unsigned long long)calls, (unsigned long long)recs_checked, (unsigned long long)tied_groups, (unsigned long long)refusals, (unsigned long long)merges);
    return 0;
}
