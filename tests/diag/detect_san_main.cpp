// Stand-alone sanitizer pass over the two host pieces of cm_detect_run's memory hand-over, linked straight from their sources:
// the memory finish of the sorted runs (cm_remain_runs_finish_mem, circminer_amd/csrc/host_circ.cpp) and the memory source of the
// FASTQ reader (cm_fastq_open_mem, circminer_amd/csrc/host_fastq.cpp).  The records are remain records with 23-token headers whose
// keys tie in groups of 65, 64, 17, 16, 2 and 1; every text handed in is an exact-size heap block.
//   runs     1, 2 and 7 runs (empty ones and a run of one record among them, every other one handed over unsorted): the two buffers
//            of the memory finish against the two files of the file finish and against cm_sort_remain of the concatenation; runs
//            opened without paths refuse the file finish
//   reader   the merged text from memory against the same bytes in files, every array of every batch and `prior`: the whole text
//            in one batch, batches of 97 pairs, an empty text, no final line feed, a text cut inside its last record (the same
//            error in the same call), R2 shorter than R1
// CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc \
//       tests/diag/detect_san_main.cpp circminer_amd/csrc/host_fastq.cpp circminer_amd/csrc/host_circ.cpp -lz -lpthread -o /tmp/detect_san && /tmp/detect_san
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "circminer_hot.h"

#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static std::string tmp_dir;
static std::string path_of(const std::string &name) { return tmp_dir + "/" + name; }
static bool write_file(const std::string &p, const std::string &s) {
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) return false;
    const bool ok = s.empty() || fwrite(s.data(), 1, s.size(), f) == s.size();
    return fclose(f) == 0 && ok;
}
static bool read_file(const std::string &p, std::string &s) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    s.clear();
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
    fclose(f);
    return true;
}
// an exact-size heap copy: a read past the end is the sanitizer's to see
struct Exact {
    char *p = nullptr;
    size_t n = 0;
    explicit Exact(const std::string &s) : n(s.size()) {
        if (n) {
            p = (char *)malloc(n);
            memcpy(p, s.data(), n);
        }
    }
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

// what a reader hands out to its end: every array of every batch as one string per batch, then the code that ended it
struct Drained {
    std::vector<std::string> batches;
    int rc = CM_OK;
    bool operator==(const Drained &o) const { return rc == o.rc && batches == o.batches; }
};
static Drained drain(cm_fastq *f, uint64_t max_pairs) {
    Drained d;
    for (;;) {
        cm_fastq_batch b;
        d.rc = cm_fastq_next(f, max_pairs, &b);
        if (d.rc != CM_OK || b.reads.n_pairs == 0) break;
        const uint64_t n = b.reads.n_pairs;
        std::string s((const char *)&n, sizeof n);
        s.append((const char *)b.reads.off1, (n + 1) * 8).append((const char *)b.reads.off2, (n + 1) * 8);
        s.append((const char *)b.reads.seq1, b.reads.off1[n]).append((const char *)b.reads.seq2, b.reads.off2[n]);
        s.append((const char *)b.qual1, b.reads.off1[n]).append((const char *)b.qual2, b.reads.off2[n]);
        s.append((const char *)b.name_off1, (n + 1) * 8).append((const char *)b.name_off2, (n + 1) * 8);
        s.append(b.names1, b.name_off1[n]).append(b.names2, b.name_off2[n]);
        s.push_back(b.prior ? 'p' : '-');
        if (b.prior) s.append((const char *)b.prior, n * sizeof(cm_mapped_read));
        d.batches.push_back(std::move(s));
    }
    cm_fastq_close(f);
    return d;
}
static int both(const cm_chr_info *chrs, uint32_t n_chr, const std::string &t1, const std::string &t2, uint64_t max_pairs, const char *tag, Drained *out) {
    const std::string p1 = path_of(std::string(tag) + "_1.fq"), p2 = path_of(std::string(tag) + "_2.fq");
    if (!write_file(p1, t1) || !write_file(p2, t2)) FAIL("%s: cannot write the files", tag);
    cm_fastq *ff = nullptr, *fm = nullptr;
    if (cm_fastq_open(p1.c_str(), p2.c_str(), chrs, n_chr, 4, &ff) != CM_OK) FAIL("%s: cm_fastq_open failed", tag);
    const Drained from_files = drain(ff, max_pairs);
    const Exact e1(t1), e2(t2);
    if (cm_fastq_open_mem(e1.p, e1.n, e2.p, e2.n, chrs, n_chr, 4, &fm) != CM_OK) FAIL("%s: cm_fastq_open_mem failed", tag);
    const Drained from_mem = drain(fm, max_pairs);
    if (!(from_mem == from_files))
        FAIL("%s (max_pairs %" PRIu64 "): memory %zu batches rc %d, files %zu batches rc %d", tag, max_pairs, from_mem.batches.size(), from_mem.rc,
             from_files.batches.size(), from_files.rc);
    if (out) *out = from_mem;
    return 0;
}

int main() {
    char templ[] = "/tmp/detect_san_XXXXXX";
    if (!mkdtemp(templ)) FAIL("mkdtemp failed");
    tmp_dir = templ;
    const cm_chr_info chrs[3] = {{"chr1", 1, 0, 90000}, {"chr2", 1, 90000, 50000}, {"chrB", 2, 0, 70000}};
    const uint32_t sizes6[6] = {65, 64, 17, 16, 2, 1};
    std::mt19937_64 rng(41);
    const uint32_t n = 700;
    // records of both files: keys tie inside a group; the members differ in the name, the bases or the qualities, or not at all
    std::vector<std::string> rec[2];
    for (uint32_t g = 0, done = 0; done < n; ++g) {
        const uint32_t size = std::min(sizes6[g % 6], n - done);
        const int chr = (int)(rng() % 3);
        const uint32_t spos = 1 + (uint32_t)(rng() % 40000);
        const int contig = chrs[chr].contig_id - 1;
        const long long key = (long long)contig * 1100000000ll + spos + chrs[chr].start_pos;
        for (uint32_t m = 0; m < size; ++m, ++done) {
            const uint32_t len = (done % 50 == 7) ? 1u : (done % 50 == 8 ? 300u : 150u);
            for (int f = 0; f < 2; ++f) {
                std::string seq(len, 'A'), qual(len, 'I');
                for (char &c : seq) c = "ACGTN"[(rng() % 41) % 5];
                if (m % 3 == 1) qual[0] = (char)('#' + rng() % 20);          // (never '@': the cases below find records by it)
                char hdr[512];
                snprintf(hdr, sizeof hdr, "@p%u%s/%d %lld %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d", m % 4 == 3 ? done - 1 : done, m % 5 == 2 ? "x" : "",
                         f + 1, key, 3 + (int)(done % 2), chrs[chr].name, spos, spos + 80, 81, 1u, 81u, done % 3 ? '+' : '-', (int)(done % 4), chrs[chr].name,
                         spos + 200, spos + 349, 150, 1u, 150u, done % 3 ? '-' : '+', 0, 350, (int)(done % 70000), (int)(done % 2), contig);
                rec[f].push_back(std::string(hdr) + "\n" + seq + "\n+\n" + qual + "\n");
            }
        }
    }
    // ---- the runs ----
    uint64_t merges = 0;
    std::string merged[2];
    for (const std::vector<uint32_t> &cuts : {std::vector<uint32_t>{}, std::vector<uint32_t>{300}, std::vector<uint32_t>{0, 1, 1, 200, 201, 650}}) {
        std::vector<uint32_t> bounds{0};
        bounds.insert(bounds.end(), cuts.begin(), cuts.end());
        bounds.push_back(n);
        std::string whole[2], want[2];
        for (int f = 0; f < 2; ++f) {
            for (const std::string &r : rec[f]) whole[f] += r;
            const std::string in = path_of("all.fq"), out = path_of("all.fq.srt");
            if (!write_file(in, whole[f]) || cm_sort_remain(in.c_str(), out.c_str()) != CM_OK || !read_file(out, want[f])) FAIL("cm_sort_remain failed");
        }
        const std::string paths[2] = {path_of("m1.srt"), path_of("m2.srt")};
        cm_remain_runs *with_files = nullptr, *without = nullptr;
        if (cm_remain_runs_open(paths[0].c_str(), paths[1].c_str(), &with_files) != CM_OK || cm_remain_runs_open(nullptr, nullptr, &without) != CM_OK)
            FAIL("cm_remain_runs_open failed");
        for (size_t k = 0; k + 1 < bounds.size(); ++k) {
            std::string part[2];
            for (int f = 0; f < 2; ++f)
                for (uint32_t i = bounds[k]; i < bounds[k + 1]; ++i) part[f] += rec[f][i];
            const Exact e1(part[0]), e2(part[1]);
            for (cm_remain_runs *r : {with_files, without})
                if (k % 2 == 0 || bounds.size() == 2) {
                    if (cm_remain_runs_add_unsorted(r, e1.p, e1.n, e2.p, e2.n) != CM_OK) FAIL("cm_remain_runs_add_unsorted failed");
                } else {
                    // a sorted run: the part through cm_sort_remain, its offsets and keys read from the text
                    std::string srt[2];
                    std::vector<uint32_t> off[2];
                    std::vector<int64_t> keys;
                    for (int f = 0; f < 2; ++f) {
                        const std::string in = path_of("part.fq"), out = path_of("part.fq.srt");
                        if (!write_file(in, part[f]) || cm_sort_remain(in.c_str(), out.c_str()) != CM_OK || !read_file(out, srt[f])) FAIL("cm_sort_remain (part) failed");
                        off[f].push_back(0);
                        size_t at = 0;
                        while (at < srt[f].size()) {
                            size_t e = at;
                            for (int line = 0; line < 4; ++line) e = srt[f].find('\n', e) + 1;
                            if (f == 0) keys.push_back(strtoll(srt[f].c_str() + srt[f].find(' ', at) + 1, nullptr, 10));
                            at = e;
                            off[f].push_back((uint32_t)at);
                        }
                    }
                    const Exact s1(srt[0]), s2(srt[1]);
                    if (cm_remain_runs_add(r, s1.p, off[0].data(), s2.p, off[1].data(), keys.data(), keys.size()) != CM_OK) FAIL("cm_remain_runs_add failed");
                }
        }
        for (cm_remain_runs *r : {without, with_files}) {
            for (int again = 0; again < 2; ++again) {
                const void *b1 = nullptr, *b2 = nullptr;
                uint64_t n1 = 0, n2 = 0;
                if (cm_remain_runs_finish_mem(r, &b1, &n1, &b2, &n2) != CM_OK) FAIL("cm_remain_runs_finish_mem failed");
                if (std::string((const char *)b1, n1) != want[0] || std::string((const char *)b2, n2) != want[1])
                    FAIL("%zu runs: the memory finish differs from cm_sort_remain of the concatenation", bounds.size() - 1);
                ++merges;
            }
        }
        if (cm_remain_runs_finish(without) != CM_EINVAL) FAIL("runs without paths took the file finish");
        std::string got[2];
        if (cm_remain_runs_finish(with_files) != CM_OK || !read_file(paths[0], got[0]) || !read_file(paths[1], got[1])) FAIL("cm_remain_runs_finish failed");
        if (got[0] != want[0] || got[1] != want[1]) FAIL("the file finish differs");
        cm_remain_runs_close(with_files);
        cm_remain_runs_close(without);
        merged[0] = want[0];
        merged[1] = want[1];
    }
    {
        cm_remain_runs *r = nullptr;
        const void *b1, *b2;
        uint64_t n1 = 7, n2 = 7;
        if (cm_remain_runs_open(nullptr, nullptr, &r) != CM_OK || cm_remain_runs_finish_mem(r, &b1, &n1, &b2, &n2) != CM_OK || n1 || n2) FAIL("empty runs");
        cm_remain_runs_close(r);
        if (cm_remain_runs_open("x", nullptr, &r) != CM_EINVAL || cm_remain_runs_finish_mem(nullptr, &b1, &n1, &b2, &n2) != CM_EINVAL) FAIL("refusals of the runs");
    }
    // ---- the reader ----
    Drained whole, d;
    if (both(chrs, 3, merged[0], merged[1], ~0ull >> 2, "whole", &whole)) return 1;
    if (whole.rc != CM_OK || whole.batches.size() != 1 || whole.batches[0].size() < merged[0].size() / 2) FAIL("whole: %zu batches, rc %d", whole.batches.size(), whole.rc);
    if (both(chrs, 3, merged[0], merged[1], 97, "parts", &d)) return 1;
    if (d.rc != CM_OK || d.batches.size() != (n + 96) / 97) FAIL("parts: %zu batches, rc %d", d.batches.size(), d.rc);
    if (both(chrs, 3, "", "", 50, "empty", &d)) return 1;
    if (d.rc != CM_OK || !d.batches.empty()) FAIL("empty: %zu batches, rc %d", d.batches.size(), d.rc);
    if (both(chrs, 3, merged[0].substr(0, merged[0].size() - 1), merged[1].substr(0, merged[1].size() - 1), ~0ull >> 2, "nolf", &d)) return 1;
    if (!(d == whole)) FAIL("no final line feed: another batch");
    const size_t last = merged[0].rfind("\n@", merged[0].size() - 2) + 1;
    const std::string cut = merged[0].substr(0, merged[0].find('\n', merged[0].find('\n', last) + 1) + 1);      // two lines of the last record
    for (uint64_t max_pairs : {~0ull >> 2, (unsigned long long)97}) {
        if (both(chrs, 3, cut, merged[1], max_pairs, "cut", &d)) return 1;
        if (d.rc != CM_EINVAL) FAIL("cut mid-record: rc %d", d.rc);
    }
    const size_t r2_last = merged[1].rfind("\n@", merged[1].size() - 2) + 1;
    if (both(chrs, 3, merged[0], merged[1].substr(0, r2_last), ~0ull >> 2, "short2", &d)) return 1;
    if (d.rc != CM_EINVAL) FAIL("R2 shorter than R1: rc %d", d.rc);
    cm_fastq *f = nullptr;
    if (cm_fastq_open_mem(nullptr, 5, nullptr, 0, nullptr, 0, 4, &f) != CM_EINVAL || f) FAIL("a null text of 5 bytes was taken");
    printf("detect_san: %" PRIu64 " memory merges, reader cases whole / parts / empty / no line feed / cut / short R2: all equal to the file path\n", merges);
    return 0;
}
