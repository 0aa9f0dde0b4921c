// Stand-alone sanitizer pass over the host FASTQ reader and the threaded PAM writer (circminer_amd/csrc/host_fastq.cpp), linked straight
// against that file: no Python, no preloaded library.  Small inputs are written into a temporary directory -- plain and gzip
// (zlib's gzwrite), ragged reads, 23-token headers among fresh ones, a last record without a newline, R2 three records longer
// than R1 -- and every way through the reader is compared with a single-threaded re-parse of the same bytes: the plain path with 1
// and 6 threads, the record path, ranks 0 - 2 of 3 on plain and gzip input, text blocks including the "nothing consumed" path, the
// malformed tails, the release hook over reads that grow, and cm_write_pam over 70 000 rows on 5 threads.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I circminer_amd/csrc
//       tests/diag/fastq_reader_san_main.cpp circminer_amd/csrc/host_fastq.cpp -lz -lpthread -o /tmp/fastq_reader_san && /tmp/fastq_reader_san
// and the same with -fsanitize=thread.
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "circminer_hot.h"

static const cm_chr_info CHRS[3] = {{"chr1", 1, 0, 5000}, {"chr2", 1, 5050, 3000}, {"chrX", 2, 0, 4000}};
static int mismatches = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            if (++mismatches <= 20) printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                \
    } while (0)

static std::string dir;
static std::string put(const std::string &name, const std::string &text, bool gz = false) {
    const std::string path = dir + "/" + name;
    if (gz) {
        gzFile g = gzopen(path.c_str(), "wb1");
        if (!g || gzwrite(g, text.data(), (unsigned)text.size()) != (int)text.size() || gzclose(g) != Z_OK) exit(2);
    } else {
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) exit(2);
    }
    return path;
}

// ---- the input and what a reader has to make of it ----------------------------------------------------------------------
static cm_mapped_read some_state(std::mt19937_64 &rng) {           // a mapped state as a remain header carries it
    cm_mapped_read m;
    memset(&m, 0, sizeof m);
    const int types[4] = {CM_CONCRD, CM_DISCRD, CM_CHIBSJ, CM_CONGEN};
    m.type = types[rng() % 4];
    m.chr_id = (int)(rng() % 3);
    m.spos_r1 = 1 + rng() % 4000, m.epos_r1 = 1 + rng() % 4000, m.spos_r2 = 1 + rng() % 4000, m.epos_r2 = 1 + rng() % 4000;
    m.mlen_r1 = 1 + rng() % 150, m.mlen_r2 = 1 + rng() % 150, m.qspos_r1 = 1 + rng() % 150, m.qepos_r1 = 1 + rng() % 150;
    m.qspos_r2 = 1 + rng() % 150, m.qepos_r2 = 1 + rng() % 150;
    m.ed_r1 = (int)(rng() % 5), m.ed_r2 = (int)(rng() % 5), m.tlen = (int)(rng() % 5000) - 50, m.junc_num = (uint16_t)(rng() % 4);
    m.r1_forward = rng() % 2, m.r2_forward = rng() % 2, m.gm_compatible = rng() % 2, m.contig_num = (int)CHRS[m.chr_id].contig_id - 1;
    return m;
}
static cm_mapped_read fresh_state() {
    cm_mapped_read m;
    memset(&m, 0, sizeof m);
    m.ed_r1 = m.ed_r2 = 5, m.type = CM_NOPROC_NOMATCH, m.tlen = 1000000000, m.chr_id = -1, m.r1_forward = m.r2_forward = 1;
    return m;
}
static std::string carried_header(const std::string &name, const cm_mapped_read &m) {      // 23 tokens
    char b[512];
    const char *cn = CHRS[m.chr_id].name;
    snprintf(b, sizeof b, "%s 0 %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d", name.c_str(), m.type, cn, m.spos_r1, m.epos_r1, (int)m.mlen_r1,
             m.qspos_r1, m.qepos_r1, m.r1_forward ? '+' : '-', m.ed_r1, cn, m.spos_r2, m.epos_r2, (int)m.mlen_r2, m.qspos_r2, m.qepos_r2, m.r2_forward ? '+' : '-',
             m.ed_r2, m.tlen, (int)m.junc_num, (int)m.gm_compatible, m.contig_num);
    return b;
}
struct Rec {
    std::string name, seq, qual;
};
// the straightforward parse: lines, four to a record, token 0 of the header without a trailing "/x"
static std::vector<Rec> reparse(const std::string &text) {
    std::vector<std::string> lines;
    for (size_t a = 0; a < text.size();) {
        size_t e = text.find('\n', a);
        if (e == std::string::npos) e = text.size();
        lines.push_back(text.substr(a, e - a));
        a = e + 1;
    }
    std::vector<Rec> out;
    for (size_t i = 0; i + 3 < lines.size(); i += 4) {
        size_t a = 1;
        while (a < lines[i].size() && lines[i][a] == ' ') ++a;
        size_t e = a;
        while (e < lines[i].size() && lines[i][e] != ' ') ++e;
        std::string name = lines[i].substr(a, e - a);
        if (name.size() >= 2 && name[name.size() - 2] == '/') name.resize(name.size() - 2);
        out.push_back({name, lines[i + 1], lines[i + 3]});
    }
    return out;
}
struct Input {
    std::string text[2];
    std::vector<Rec> rec[2];
    std::vector<cm_mapped_read> prior;                // of R1's records
    bool any_carried = false;
};
static Input make_input(uint64_t seed, int n, int surplus2, bool carried, int min_len, int max_len, bool cut_last_newline) {
    std::mt19937_64 rng(seed);
    Input in;
    for (int x = 0; x < 2; ++x) {
        std::string &t = in.text[x];
        for (int i = 0; i < n + (x ? surplus2 : 0); ++i) {
            const int len = min_len + (int)(rng() % (unsigned)(max_len - min_len + 1));
            std::string name = "read" + std::to_string(i) + (i % 3 ? "" : (x ? "/2" : "/1"));
            if (x == 0) {
                if (carried && i % 5 == 0) {
                    in.prior.push_back(some_state(rng));
                    name = carried_header("read" + std::to_string(i), in.prior.back());
                    in.any_carried = true;
                } else {
                    in.prior.push_back(fresh_state());
                    if (i % 7 == 0) name += "  extra tokens here";
                }
            }
            t += "@" + name + "\n";
            for (int k = 0; k < len; ++k) t += "ACGTNacgt"[rng() % 9];
            t += "\n+\n";
            for (int k = 0; k < len; ++k) t += (char)(35 + rng() % 39);
            t += "\n";
        }
        if (x == 0 && cut_last_newline && !t.empty()) t.pop_back();
        in.rec[x] = reparse(t);
    }
    return in;
}

// ---- cm_fastq_next against the re-parse ------------------------------------------------------------------------------------
// the pairs [lo, hi) of `in` are what the reader has to deliver, in batches of at most `batch`
static void expect_pairs(cm_fastq *f, const Input &in, size_t lo, size_t hi, uint64_t batch) {
    size_t at = lo;
    for (;;) {
        cm_fastq_batch b;
        const int rc = cm_fastq_next(f, batch, &b);
        CHECK(rc == CM_OK);
        if (rc != CM_OK || b.reads.n_pairs == 0) break;
        const size_t n = (size_t)b.reads.n_pairs;
        CHECK(at + n <= hi && (n == batch || at + n == hi));
        if (at + n > hi) break;
        bool carried = false;
        for (size_t i = 0; i < n; ++i) {
            const Rec &r1 = in.rec[0][at + i], &r2 = in.rec[1][at + i];
            CHECK(r1.name == b.names1 + b.name_off1[i] && r2.name == b.names2 + b.name_off2[i]);
            CHECK(b.name_off1[i + 1] - b.name_off1[i] == r1.name.size() + 1 && b.name_off2[i + 1] - b.name_off2[i] == r2.name.size() + 1);
            CHECK(b.reads.off1[i + 1] - b.reads.off1[i] == r1.seq.size() && b.reads.off2[i + 1] - b.reads.off2[i] == r2.seq.size());
            CHECK(memcmp(b.reads.seq1 + b.reads.off1[i], r1.seq.data(), r1.seq.size()) == 0 && memcmp(b.qual1 + b.reads.off1[i], r1.qual.data(), r1.qual.size()) == 0);
            CHECK(memcmp(b.reads.seq2 + b.reads.off2[i], r2.seq.data(), r2.seq.size()) == 0 && memcmp(b.qual2 + b.reads.off2[i], r2.qual.data(), r2.qual.size()) == 0);
            carried = carried || in.prior[at + i].type != CM_NOPROC_NOMATCH;
            if (b.prior) CHECK(memcmp(&b.prior[i], &in.prior[at + i], sizeof(cm_mapped_read)) == 0);
        }
        CHECK((b.prior != nullptr) == carried);
        at += n;
    }
    CHECK(at == hi);
}
static void whole_files(const Input &in, const std::string p[2], uint64_t batch) {
    cm_fastq *f = nullptr;
    CHECK(cm_fastq_open(p[0].c_str(), p[1].c_str(), CHRS, 3, 4, &f) == CM_OK);
    if (!f) return;
    expect_pairs(f, in, 0, in.rec[0].size(), batch);
    cm_fastq_close(f);
}
static void shards(const Input &in, const std::string p[2]) {
    const uint64_t n = in.rec[0].size();
    for (int rank = 0; rank < 3; ++rank) {
        cm_fastq *f = nullptr;
        uint64_t first = ~0ull, count = ~0ull;
        CHECK(cm_fastq_open_shard(p[0].c_str(), p[1].c_str(), CHRS, 3, 4, rank, 3, 3, &f, &first, &count) == CM_OK);
        if (!f) continue;
        CHECK(first == n * (uint64_t)rank / 3 && count == n * (uint64_t)(rank + 1) / 3 - first);
        expect_pairs(f, in, (size_t)first, (size_t)(first + count), 1300);
        cm_fastq_close(f);
    }
}

// ---- text blocks -----------------------------------------------------------------------------------------------------------------
static uint64_t whole_records(const uint8_t *t, uint64_t len) {    // bytes of the whole records at the front of a block
    uint64_t lines = 0, used = 0;
    for (uint64_t i = 0; i < len; ++i)
        if (t[i] == '\n' && ++lines % 4 == 0) used = i + 1;
    return used;
}
static void text_blocks(const Input &in, const std::string p[2]) {
    cm_fastq *f = nullptr;
    CHECK(cm_fastq_open(p[0].c_str(), p[1].c_str(), CHRS, 3, 4, &f) == CM_OK);
    if (!f) return;
    uint64_t pos[2] = {0, 0};
    struct Held {
        const uint8_t *t[2];
        std::string copy[2];
    };
    std::vector<Held> held;
    int starved = 0;
    for (int call = 0; call < 100000; ++call) {
        // 64 bytes hold no record: the first blocks of the files, and one in the middle, grow over several calls
        const uint64_t want = (pos[0] == 0 || (call > 40 && call < 60)) ? 64 : 3000;
        const uint8_t *t[2];
        uint64_t len[2];
        int eof[2];
        if (cm_fastq_next_text(f, want, &t[0], &len[0], &eof[0], &t[1], &len[1], &eof[1]) != CM_OK) {
            CHECK(!"cm_fastq_next_text");
            break;
        }
        uint64_t used[2];
        for (int x = 0; x < 2; ++x) {
            CHECK(pos[x] + len[x] <= in.text[x].size() && memcmp(t[x], in.text[x].data() + pos[x], (size_t)len[x]) == 0);
            CHECK((eof[x] != 0) == (pos[x] + len[x] == in.text[x].size()));
            used[x] = whole_records(t[x], len[x]);
        }
        for (size_t k = held.size() >= 3 ? held.size() - 3 : 0; k < held.size(); ++k)                // the three blocks before this one
            for (int x = 0; x < 2; ++x) CHECK(memcmp(held[k].t[x], held[k].copy[x].data(), held[k].copy[x].size()) == 0);
        if ((used[0] == 0 || used[1] == 0) && !(eof[0] && eof[1])) {                                  // no pair yet: more of the same block
            ++starved;
            CHECK(cm_fastq_text_consumed(f, 0, 0) == CM_OK);
            continue;
        }
        held.push_back({{t[0], t[1]}, {std::string((const char *)t[0], (size_t)len[0]), std::string((const char *)t[1], (size_t)len[1])}});
        if (eof[0] && eof[1]) used[0] = len[0], used[1] = len[1];
        CHECK(cm_fastq_text_consumed(f, used[0], used[1]) == CM_OK);
        pos[0] += used[0], pos[1] += used[1];
        if (len[0] == 0 && len[1] == 0) break;
    }
    CHECK(pos[0] == in.text[0].size() && pos[1] == in.text[1].size() && starved > 10 && held.size() > 60);
    cm_fastq_close(f);
}

// ---- malformed tails: both parsers refuse them in the same call -------------------------------------------------------------------
static std::vector<long> call_log(const std::string &r1, const std::string &r2, uint64_t batch, bool serial) {
    if (serial) setenv("CM_FASTQ_SERIAL", "1", 1);
    else unsetenv("CM_FASTQ_SERIAL");
    std::vector<long> log;
    cm_fastq *f = nullptr;
    if (cm_fastq_open(r1.c_str(), r2.c_str(), CHRS, 3, 4, &f) != CM_OK) return log;
    for (;;) {
        cm_fastq_batch b;
        const int rc = cm_fastq_next(f, batch, &b);
        if (rc != CM_OK) {
            log.push_back(rc);
            break;
        }
        if (b.reads.n_pairs == 0) break;
        log.push_back((long)b.reads.n_pairs);
    }
    cm_fastq_close(f);
    unsetenv("CM_FASTQ_SERIAL");
    return log;
}
static void malformed_tails() {
    const Input in = make_input(5, 40, 0, false, 30, 150, false);
    const std::string good = put("good.fq", in.text[0]);
    const char *tails[5] = {"\n", "\n\n\n", "\n\n\n\n", "@partial\nACGT\n", "@partial\nACGT\n+\n"};
    for (const char *tail : tails) {
        const std::string dirty = put("dirty.fq", in.text[0] + tail);
        for (int side = 0; side < 2; ++side)
            for (uint64_t batch : {45, 40, 16, 7}) {
                const std::vector<long> fast = call_log(side ? good : dirty, side ? dirty : good, batch, false);
                const std::vector<long> slow = call_log(side ? good : dirty, side ? dirty : good, batch, true);
                CHECK(fast == slow && !fast.empty() && fast.back() == CM_EINVAL);
            }
    }
}

// ---- the release hook: an array that grows is announced before it goes -----------------------------------------------------------
static std::set<const void *> live;
static int announced = 0;
static std::mutex hook_mutex;                    // the hook runs on whichever thread frees: R1's arrays on the caller's, R2's on the second
static void on_release(void *, const void *p, uint64_t) {
    std::lock_guard<std::mutex> lock(hook_mutex);
    live.erase(p);
    ++announced;
}
static void growing_reads(bool serial) {
    std::string text[2];
    const int per = 300, nb = 12;
    for (int b = 0; b < nb; ++b)
        for (int i = 0; i < per; ++i)
            for (int x = 0; x < 2; ++x) {
                const size_t len = 40 + 60 * (size_t)b + 3 * (size_t)x;
                text[x] += "@r" + std::to_string(b) + "_" + std::to_string(i) + "\n" + std::string(len, "ACGT"[i % 4]) + "\n+\n" + std::string(len, 'I') + "\n";
            }
    const std::string p[2] = {put("grow_1.fq", text[0]), put("grow_2.fq", text[1])};
    if (serial) setenv("CM_FASTQ_SERIAL", "1", 1);
    cm_fastq *f = nullptr;
    CHECK(cm_fastq_open(p[0].c_str(), p[1].c_str(), nullptr, 0, 4, &f) == CM_OK);
    if (!f) return;
    live.clear();
    announced = 0;
    cm_fastq_set_release_hook(f, on_release, nullptr);
    const void *gen[4][4] = {};
    for (int b = 0; b < nb; ++b) {
        cm_fastq_batch fb;
        CHECK(cm_fastq_next(f, per, &fb) == CM_OK && fb.reads.n_pairs == (uint64_t)per);
        const void *mine[4] = {fb.reads.seq1, fb.reads.seq2, fb.reads.off1, fb.reads.off2};
        for (int k = 0; k < 4; ++k) {
            if (b >= 4) CHECK(gen[b % 4][k] == mine[k] || !live.count(gen[b % 4][k]));
            gen[b % 4][k] = mine[k];
            live.insert(mine[k]);
        }
        CHECK(fb.reads.off1[per] == (uint64_t)per * (40 + 60 * (uint64_t)b) && fb.reads.seq2[fb.reads.off2[per] - 1] == (uint8_t)"ACGT"[(per - 1) % 4]);
    }
    CHECK(announced >= 8);
    const int before = announced;
    cm_fastq_close(f);
    CHECK(announced > before && live.empty());
    unsetenv("CM_FASTQ_SERIAL");
}

// ---- cm_write_pam on several threads ------------------------------------------------------------------------------------------
static std::string slurp(const std::string &path) {
    std::string s;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return s;
    char buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, k);
    fclose(f);
    return s;
}
static void pam_rows() {
    const int n = 70000;
    std::string text;
    for (int i = 0; i < n; ++i) text += "@q" + std::to_string(i) + "\nACGT\n+\nIIII\n";
    const std::string p = put("pam.fq", text);
    std::mt19937_64 rng(3);
    std::vector<cm_mapped_read> st;
    for (int i = 0; i < n; ++i) st.push_back(i % 4 ? some_state(rng) : fresh_state());
    std::vector<uint64_t> sel;
    for (int i = 0; i < n; i += 3) sel.push_back((uint64_t)i);
    setenv("CM_FASTQ_THREADS", "4", 1);
    cm_fastq *f = nullptr;
    cm_fastq_batch b;
    CHECK(cm_fastq_open(p.c_str(), p.c_str(), CHRS, 3, 4, &f) == CM_OK);
    if (!f) return;
    CHECK(cm_fastq_next(f, (uint64_t)n, &b) == CM_OK && b.reads.n_pairs == (uint64_t)n);
    std::string out[2];
    for (int k = 0; k < 2; ++k) {
        setenv("CM_WRITER_THREADS", k ? "5" : "1", 1);
        const std::string path = dir + (k ? "/o5.pam" : "/o1.pam");
        cm_writer *w = nullptr;
        CHECK(cm_writer_open(path.c_str(), nullptr, CHRS, 3, &w) == CM_OK);
        if (!w) continue;
        CHECK(cm_write_pam(w, &b, st.data(), nullptr, 0) == CM_OK);
        CHECK(cm_write_pam(w, &b, st.data(), sel.data(), sel.size()) == CM_OK);
        CHECK(cm_writer_flush(w) == CM_OK);
        cm_writer_close(w);
        out[k] = slurp(path);
    }
    CHECK(out[0] == out[1] && (size_t)std::count(out[0].begin(), out[0].end(), '\n') == (size_t)n + sel.size());
    CHECK(out[0].compare(0, 3, "q0\t") == 0);
    cm_fastq_close(f);
    unsetenv("CM_WRITER_THREADS");
    unsetenv("CM_FASTQ_THREADS");
}

int main() {
    char tmpl[] = "/tmp/fastq_reader_san_XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    dir = tmpl;
    // 9000 pairs in batches of 5000: above the sizes at which the plain path's loops go to their threads
    const Input in = make_input(12, 9000, 3, true, 20, 300, true);
    const std::string plain[2] = {put("a_1.fq", in.text[0]), put("a_2.fq", in.text[1])};
    const std::string gz[2] = {put("a_1.fq.gz", in.text[0], true), put("a_2.fq.gz", in.text[1], true)};
    CHECK(in.any_carried && in.rec[0].size() == 9000 && in.rec[1].size() == 9003);
    for (const char *threads : {"1", "6"}) {                   // the plain path
        setenv("CM_FASTQ_THREADS", threads, 1);
        whole_files(in, plain, 5000);
        whole_files(in, plain, 777);
        shards(in, plain);
    }
    unsetenv("CM_FASTQ_THREADS");
    setenv("CM_FASTQ_SERIAL", "1", 1);                         // the record path: on the same files, and on gzip input
    whole_files(in, plain, 5000);
    unsetenv("CM_FASTQ_SERIAL");
    whole_files(in, gz, 777);
    shards(in, gz);
    text_blocks(in, plain);
    malformed_tails();
    growing_reads(false);
    growing_reads(true);
    pam_rows();
    const std::string rm = "rm -rf '" + dir + "'";
    if (system(rm.c_str()) != 0) printf("could not remove %s\n", dir.c_str());
    printf("%d mismatches\n", mismatches);
    return mismatches ? 1 : 0;
}
