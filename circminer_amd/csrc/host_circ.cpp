// Stage 2 (ProcessCirc), first and last step only -- SURVEY.md §8(f) row N3 is NOT complete: the per-candidate
// back-splice-junction calling in between (call_circ_single_split / call_circ_double_split, check_split_map,
// split_realignment, src/process_circ.cpp:334-1552) is not built yet.  What is here is host code a later round keeps:
//
//   * cm_sort_remain  : ProcessCirc::sort_fq (src/process_circ.cpp:179-193), the
//                       `cat f | paste - - - - | sort -k2,2n | tr "\t" "\n" > f.srt` pipeline on the last round's remain
//                       FASTQ: records ordered by the numeric value of the second blank-separated field of the header
//                       (genome_spos; a non-numeric field counts as 0), ties by the bytes of the whole pasted line
//                       (GNU sort's last-resort comparison in the C locale -- the reference does not set a locale, see
//                       SURVEY §8(f) N3; tests compare with `LC_ALL=C sort`);
//   * cm_circ_report  : ProcessCirc::report_events + both_side_consensus (src/process_circ.cpp:1554-1631) with
//                       CircRes::operator< / operator== (src/common.cpp:479-493) and get_consensus (src/utils.cpp:771-816):
//                       std::sort of the calls, one <out>.circ_report row per (chr, spos, epos) group whose first
//                       element is of type CR.  The order of the read names inside a row is whatever libstdc++'s
//                       (unstable) std::sort leaves for the input order given, exactly as in the reference.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "circminer_hot.h"

namespace {

constexpr int CR = 20;                    // src/process_circ.h:16
const char *const CIRC_TYPE[3] = {"STC", "MTC", "NC"};   // src/process_circ.cpp:86-88

// numeric key of `sort -k2,2n`: field 2 = from the end of field 1 to the end of the next run of non-blanks; -n skips
// leading blanks, takes an optional '-' and digits (no overflow in GNU sort; genome_spos fits 63 bits)
struct NumKey {
    bool neg = false;
    std::string digits;                   // without leading zeros; empty = 0
};
NumKey key_of(const std::string &line) {
    size_t i = 0;
    const size_t n = line.size();
    auto blank = [](char c) { return c == ' ' || c == '\t'; };
    while (i < n && blank(line[i])) ++i;           // field 1: leading blanks + non-blanks
    while (i < n && !blank(line[i])) ++i;
    size_t j = i;                                  // field 2 starts here (leading blanks belong to it)
    while (j < n && blank(line[j])) ++j;
    NumKey k;
    if (j < n && line[j] == '-') {
        k.neg = true;
        ++j;
    }
    size_t d = j;
    while (d < n && line[d] >= '0' && line[d] <= '9') ++d;
    while (j < d && line[j] == '0') ++j;
    k.digits.assign(line, j, d - j);
    if (k.digits.empty()) k.neg = false;           // "-0", "-", "*" ... compare as 0
    return k;
}
int cmp_key(const NumKey &a, const NumKey &b) {
    if (a.neg != b.neg) return a.neg ? -1 : 1;
    int c;
    if (a.digits.size() != b.digits.size()) c = a.digits.size() < b.digits.size() ? -1 : 1;
    else c = a.digits.compare(b.digits);
    c = c < 0 ? -1 : (c > 0 ? 1 : 0);
    return a.neg ? -c : c;
}

struct Call {                             // CircRes, src/common.h:406-423
    std::string chr, rname, start_signal, end_signal, start_bp_ref, end_bp_ref;
    uint32_t spos = 0, epos = 0;
    int type = 0;
    bool operator<(const Call &r) const {
        if (chr != r.chr) return chr < r.chr;
        if (spos != r.spos) return spos < r.spos;
        if (epos != r.epos) return epos < r.epos;
        return type < r.type;
    }
    bool same_event(const Call &r) const { return chr == r.chr && spos == r.spos && epos == r.epos; }
};

std::string consensus(const std::vector<const std::string *> &v) {          // get_consensus(vector<string>)
    std::string res;
    if (v.empty()) return res;
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i]->size() != v[i - 1]->size()) return res;
    const char nuc[4] = {'A', 'C', 'G', 'T'};
    for (size_t i = 0; i < v[0]->size(); ++i) {
        unsigned cnt[4] = {0, 0, 0, 0};
        for (const std::string *s : v) {
            switch ((*s)[i]) {
                case 'A': case 'a': ++cnt[0]; break;
                case 'C': case 'c': ++cnt[1]; break;
                case 'G': case 'g': ++cnt[2]; break;
                case 'T': case 't': ++cnt[3]; break;
                default: break;
            }
        }
        unsigned mx = 0;
        char ch = 'N';
        for (int k = 0; k < 4; ++k)
            if (cnt[k] > mx) {
                mx = cnt[k];
                ch = nuc[k];
            }
        res += (mx >= v.size() / 2) ? ch : 'N';
    }
    return res;
}

void report_group(FILE *f, const std::vector<const Call *> &g) {
    const Call &last = *g[0];
    if (last.type != CR) return;                       // "won't print novel events"
    std::vector<const std::string *> ss, es;
    for (const Call *c : g) {
        ss.push_back(&c->start_signal);
        es.push_back(&c->end_signal);
    }
    const std::string ss_con = consensus(ss), es_con = consensus(es);
    const bool pass = ss_con == last.start_bp_ref && es_con == last.end_bp_ref;
    fprintf(f, "%s\t%u\t%u\t%d\t%s\t%s-%s\t%s-%s\t%s\t", last.chr.c_str(), last.spos, last.epos, (int)g.size(), CIRC_TYPE[last.type - CR], ss_con.c_str(),
            es_con.c_str(), last.start_bp_ref.c_str(), last.end_bp_ref.c_str(), pass ? "Pass" : "Fail");
    for (size_t j = 0; j + 1 < g.size(); ++j) fprintf(f, "%s,", g[j]->rname.c_str());
    fprintf(f, "%s\n", g.back()->rname.c_str());
}

}  // namespace

// RegionalHashTable::create_table / hash_val / add_loc (src/hash_table.cpp:58-112): every window_size-mer of the gene region
// seq[0..len), location = start + offset; stage 2 uses ws = 8 (src/circminer.cpp:348) and probes it every 3 bases of the
// unmapped part of a read.  Flattened: bucket hv owns loc[off[hv] .. off[hv + 1]) in ascending location.  A bucket that
// would hold more than MAXHIT = 1000 locations is emptied, a window with a byte outside ACGTacgt has no hash value.
extern "C" int cm_regional_table_build(const uint8_t *seq, uint32_t start, int32_t len, int32_t window_size, uint32_t **off_out, uint32_t **loc_out) {
    if (!off_out || !loc_out || window_size < 1 || window_size > 12 || (len > 0 && !seq)) return CM_EINVAL;
    constexpr uint32_t MAXHIT = 1000;
    const size_t size = (size_t)1 << (2 * window_size);
    std::vector<uint32_t> cnt(size + 1, 0);
    std::vector<int32_t> hv_at;
    const int n_win = len >= window_size ? len - window_size + 1 : 0;
    hv_at.resize((size_t)n_win);
    auto code = [](uint8_t ch) -> int {
        switch (ch) {
            case 'A': case 'a': return 0;
            case 'C': case 'c': return 1;
            case 'G': case 'g': return 2;
            case 'T': case 't': return 3;
            default: return -1;
        }
    };
    for (int i = 0; i < n_win; ++i) {
        int32_t hv = 0;
        for (int k = 0; k < window_size; ++k) {
            const int c = code(seq[i + k]);
            if (c < 0) {
                hv = -1;
                break;
            }
            hv = (hv << 2) | c;
        }
        hv_at[(size_t)i] = hv;
        if (hv >= 0) ++cnt[(size_t)hv];
    }
    uint32_t *off = (uint32_t *)malloc((size + 1) * sizeof(uint32_t));
    if (!off) return CM_ENOMEM;
    uint32_t total = 0;
    for (size_t h = 0; h < size; ++h) {
        off[h] = total;
        if (cnt[h] <= MAXHIT) total += cnt[h];
        else cnt[h] = 0;                                   // frag_count > MAXHIT -> frag_count = 0
    }
    off[size] = total;
    uint32_t *loc = (uint32_t *)malloc((total ? total : 1) * sizeof(uint32_t));
    if (!loc) {
        free(off);
        return CM_ENOMEM;
    }
    std::vector<uint32_t> fill(size, 0);
    for (int i = 0; i < n_win; ++i) {
        const int32_t hv = hv_at[(size_t)i];
        if (hv < 0 || cnt[(size_t)hv] == 0) continue;
        loc[off[hv] + fill[(size_t)hv]++] = start + (uint32_t)i;
    }
    *off_out = off;
    *loc_out = loc;
    return CM_OK;
}
extern "C" void cm_regional_table_free(uint32_t *off, uint32_t *loc) {
    free(off);
    free(loc);
}

// The file is read whole; a record is located by its four line ends, keyed by the numeric value of header field 2 and -- only on a
// tie -- compared as the TAB-pasted line GNU sort sees.  The sorted order is written with one gather pass.  (The first version built
// a std::string per record: 2.7 s for the 1.6 M candidate pairs of a 33 M-pair run; this one is bound by the two copies of the file.)
namespace {
struct SortRec {
    uint64_t mag;          // |key| (saturating: 19+ digits all compare as "huge", ties then fall to the byte compare of equal-length digit runs)
    uint32_t idx;          // record number
    uint8_t neg, huge;
};
struct RemainFile {
    std::vector<char> buf;
    std::vector<size_t> start;      // start[r] = offset of record r; start[n] = end of the last record's bytes (incl. its newline if present)
    std::vector<uint8_t> lines;     // lines actually present in record r (4, except an incomplete last group)
};
// Two pasted lines compared as GNU sort's last resort does: pa[0 .. ra) / pb[0 .. rb) are the bytes present, la / lb the lengths of
// the pasted lines (line ends become TABs; a missing trailing line contributes its TAB, no bytes)
inline int pasted_cmp_bytes(const char *pa, size_t ra, size_t la, const char *pb, size_t rb, size_t lb) {
    const size_t m = la < lb ? la : lb;
    for (size_t k = 0; k < m; ++k) {
        unsigned char ca = k < ra ? (unsigned char)pa[k] : (unsigned char)'\t', cb = k < rb ? (unsigned char)pb[k] : (unsigned char)'\t';
        if (ca == '\n') ca = '\t';
        if (cb == '\n') cb = '\t';
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}
inline int pasted_cmp(const RemainFile &F, uint32_t a, uint32_t b) {
    auto len_of = [&](uint32_t r) {
        size_t e = F.start[r + 1];
        size_t n = e - F.start[r];
        if (n && F.buf[e - 1] == '\n') --n;            // the 4th line's newline is not part of the pasted line
        return n + (size_t)(4 - F.lines[r]);            // paste pads an incomplete group with empty fields: one TAB each
    };
    return pasted_cmp_bytes(F.buf.data() + F.start[a], F.start[a + 1] - F.start[a], len_of(a), F.buf.data() + F.start[b], F.start[b + 1] - F.start[b], len_of(b));
}
// The in-memory part of cm_sort_remain: the records of F.buf located and keyed, recs in the sorted order.  Shared by the file
// version below and by the runs' fall-back (cm_remain_runs_add_unsorted).
int order_records(RemainFile &F, std::vector<SortRec> &recs) {
    const size_t n_bytes = F.buf.size();
    {   // record boundaries: every fourth line end
        size_t pos = 0;
        int part = 0;
        F.start.push_back(0);
        while (pos < n_bytes) {
            const char *nl = (const char *)memchr(F.buf.data() + pos, '\n', n_bytes - pos);
            pos = nl ? (size_t)(nl - F.buf.data()) + 1 : n_bytes;
            if (++part == 4) {
                F.start.push_back(pos);
                F.lines.push_back(4);
                part = 0;
            }
        }
        if (part) {                                    // an incomplete last group (getline semantics: a line without a newline counts)
            F.start.push_back(n_bytes);
            F.lines.push_back((uint8_t)part);
        }
    }
    const size_t n_rec = F.lines.size();
    if (n_rec > 0xfffffff0ull) return CM_ELIMIT;
    recs.assign(n_rec, SortRec{0, 0, 0, 0});
    auto blank = [](char c) { return c == ' ' || c == '\t'; };
    for (size_t r = 0; r < n_rec; ++r) {               // key_of() on the first line (the pasted line's field 2 lies inside it unless it has one field:
        const char *p = F.buf.data() + F.start[r];     // then field 2 begins at the TAB that replaces the line end, i.e. with the second line)
        const size_t n = F.start[r + 1] - F.start[r];
        auto at = [&](size_t k) -> char { const char c = p[k]; return c == '\n' ? '\t' : c; };
        size_t i = 0;
        while (i < n && blank(at(i))) ++i;
        while (i < n && !blank(at(i))) ++i;
        size_t j = i;
        while (j < n && blank(at(j))) ++j;
        SortRec k{0, (uint32_t)r, 0, 0};
        if (j < n && at(j) == '-') {
            k.neg = 1;
            ++j;
        }
        size_t d = j;
        while (d < n && p[d] >= '0' && p[d] <= '9') ++d;
        while (j < d && p[j] == '0') ++j;
        if (d - j > 18) k.huge = 1;                    // beyond 10^18: falls back to the exact digit-string compare below
        else
            for (size_t q = j; q < d; ++q) k.mag = k.mag * 10 + (uint64_t)(p[q] - '0');
        if (d == j) k.neg = 0;                         // "-0", "-", "*" ... compare as 0
        recs[r] = k;
    }
    bool any_huge = false;
    for (const SortRec &k : recs) any_huge = any_huge || k.huge;
    if (any_huge) {                                    // never the case for genome positions; keep the exact semantics through the old path's keys
        std::vector<NumKey> keys(n_rec);
        for (size_t r = 0; r < n_rec; ++r) {
            std::string line(F.buf.data() + F.start[r], F.start[r + 1] - F.start[r]);
            for (char &c : line) if (c == '\n') c = '\t';
            keys[r] = key_of(line);
        }
        std::sort(recs.begin(), recs.end(), [&](const SortRec &a, const SortRec &b) {
            const int c = cmp_key(keys[a.idx], keys[b.idx]);
            if (c) return c < 0;
            return pasted_cmp(F, a.idx, b.idx) < 0;
        });
    } else {
        std::sort(recs.begin(), recs.end(), [&](const SortRec &a, const SortRec &b) {
            if (a.neg != b.neg) return a.neg > b.neg;                  // negative first
            if (a.mag != b.mag) return a.neg ? a.mag > b.mag : a.mag < b.mag;
            return pasted_cmp(F, a.idx, b.idx) < 0;                    // GNU sort's last resort: the whole line, C locale
        });
    }
    return CM_OK;
}
}  // namespace

extern "C" int cm_sort_remain(const char *in_path, const char *out_path) {
    if (!in_path || !out_path) return CM_EINVAL;
    FILE *in = fopen(in_path, "rb");
    if (!in) return CM_EINVAL;
    RemainFile F;
    {
        if (fseek(in, 0, SEEK_END) != 0) { fclose(in); return CM_EIO; }
        const long sz = ftell(in);
        if (sz < 0 || fseek(in, 0, SEEK_SET) != 0) { fclose(in); return CM_EIO; }
        F.buf.resize((size_t)sz);
        if (sz && fread(F.buf.data(), 1, (size_t)sz, in) != (size_t)sz) { fclose(in); return CM_EIO; }
        fclose(in);
    }
    std::vector<SortRec> recs;
    const int rc = order_records(F, recs);
    if (rc != CM_OK) return rc;
    FILE *out = fopen(out_path, "wb");
    if (!out) return CM_EINVAL;
    std::vector<char> ob;
    ob.reserve(8u << 20);
    bool bad = false;
    auto flush = [&]() {
        if (!ob.empty() && fwrite(ob.data(), 1, ob.size(), out) != ob.size()) bad = true;
        ob.clear();
    };
    for (const SortRec &k : recs) {
        const char *p = F.buf.data() + F.start[k.idx];
        size_t n = F.start[k.idx + 1] - F.start[k.idx];
        const bool has_nl = n && p[n - 1] == '\n';
        if (has_nl) --n;
        ob.insert(ob.end(), p, p + n);                 // the record's lines as they are (tr turns the pasted TABs back into line ends)
        for (int x = F.lines[k.idx]; x < 4; ++x) ob.push_back('\n');      // the TABs paste added for missing lines
        ob.push_back('\n');
        if (ob.size() > (8u << 20) - 4096) flush();
    }
    flush();
    if (fclose(out) != 0 || bad) return CM_EIO;
    return CM_OK;
}

// ---- the same order from sorted runs (cm_remain_runs, see circminer_hot.h) ----------------------------------------------------
// A run of one mate file: records of four lines each, in cm_sort_remain's order, with the signed key of each.  The merge orders by
// key, then by the pasted line (pasted_cmp_bytes: the comparator of cm_sort_remain), then by run number; records are gathered into
// the output as they are.
namespace {
struct Run {
    std::vector<char> bytes;
    std::vector<uint64_t> off;        // records + 1
    std::vector<int64_t> key;
};
// key_of() on a record's first line as a signed 64-bit value (saturating; what a key printed from 64 bits parses back to)
int64_t parsed_key(const char *p, size_t n) {
    auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\n'; };       // (the line end is paste's TAB)
    size_t i = 0;
    while (i < n && blank(p[i])) ++i;
    while (i < n && !blank(p[i])) ++i;
    while (i < n && blank(p[i])) ++i;
    bool neg = false;
    if (i < n && p[i] == '-') neg = true, ++i;
    uint64_t v = 0;
    bool sat = false;
    for (; i < n && p[i] >= '0' && p[i] <= '9'; ++i) {
        const uint64_t d = (uint64_t)(p[i] - '0');
        if (v > (0x8000000000000000ull - d) / 10) sat = true;
        else v = v * 10 + d;
    }
    if (sat) v = 0x8000000000000000ull;
    if (neg) return v >= 0x8000000000000000ull ? INT64_MIN : -(int64_t)v;
    return v >= 0x7fffffffffffffffull ? INT64_MAX : (int64_t)v;
}
}  // namespace
struct cm_remain_runs {
    std::string path[2];
    bool has_paths = false;           // opened without paths: only the memory finish is allowed
    std::vector<Run> runs[2];
    std::vector<char> merged[2];      // cm_remain_runs_finish_mem: the two merged files, kept until close
};
namespace {
// The merge of one mate file's runs, written once: records leave in the order of key, pasted line, run number, and `sink` takes
// each record's bytes as they are.  Two sinks: a buffered file (cm_remain_runs_finish) and a vector (cm_remain_runs_finish_mem).
template <class Sink> void merge_runs(const std::vector<Run> &runs, Sink sink) {
    struct Head {
        uint32_t run;
        uint64_t rec;
    };
    // a > b: a comes out later (std::*_heap keep the largest on top, so the comparator is the order reversed)
    auto later = [&](const Head &a, const Head &b) {
        const Run &A = runs[a.run], &B = runs[b.run];
        if (A.key[a.rec] != B.key[b.rec]) return A.key[a.rec] > B.key[b.rec];
        const size_t la = (size_t)(A.off[a.rec + 1] - A.off[a.rec]) - 1, lb = (size_t)(B.off[b.rec + 1] - B.off[b.rec]) - 1;
        const int c = pasted_cmp_bytes(A.bytes.data() + A.off[a.rec], la, la, B.bytes.data() + B.off[b.rec], lb, lb);
        if (c) return c > 0;
        return a.run > b.run;
    };
    std::vector<Head> heap;
    for (uint32_t k = 0; k < runs.size(); ++k)
        if (!runs[k].key.empty()) heap.push_back(Head{k, 0});
    std::make_heap(heap.begin(), heap.end(), later);
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), later);
        Head h = heap.back();
        const Run &R = runs[h.run];
        sink(R.bytes.data() + R.off[h.rec], (size_t)(R.off[h.rec + 1] - R.off[h.rec]));
        if (++h.rec < R.key.size()) {
            heap.back() = h;
            std::push_heap(heap.begin(), heap.end(), later);
        } else heap.pop_back();
    }
}
}  // namespace

extern "C" int cm_remain_runs_open(const char *srt_path1, const char *srt_path2, cm_remain_runs **out) {
    if (!out || (!srt_path1) != (!srt_path2)) return CM_EINVAL;            // both paths, or neither (memory finish only)
    *out = nullptr;
    try {
        cm_remain_runs *r = new cm_remain_runs;
        *out = r;
        if (srt_path1) {
            r->path[0] = srt_path1;
            r->path[1] = srt_path2;
            r->has_paths = true;
        }
    } catch (const std::bad_alloc &) {
        delete *out;
        *out = nullptr;
        return CM_ENOMEM;
    }
    return CM_OK;
}
extern "C" int cm_remain_runs_add(cm_remain_runs *r, const void *bytes1, const uint32_t *off1, const void *bytes2, const uint32_t *off2, const int64_t *keys,
                                  uint64_t n_records) {
    if (!r || (n_records && (!bytes1 || !off1 || !bytes2 || !off2 || !keys))) return CM_EINVAL;
    const void *bytes[2] = {bytes1, bytes2};
    const uint32_t *off[2] = {off1, off2};
    for (int m = 0; m < 2; ++m)
        for (uint64_t i = 0; i < n_records; ++i)
            if (off[m][i + 1] <= off[m][i] || ((const char *)bytes[m])[off[m][i + 1] - 1] != '\n') return CM_EINVAL;     // a record ends with its line feed
    for (uint64_t i = 1; i < n_records; ++i)
        if (keys[i] < keys[i - 1]) return CM_EINVAL;
    try {
    for (int m = 0; m < 2; ++m) {
        Run run;
        if (n_records) {
            run.bytes.assign((const char *)bytes[m] + off[m][0], (const char *)bytes[m] + off[m][n_records]);
            run.off.resize(n_records + 1);
            for (uint64_t i = 0; i <= n_records; ++i) run.off[i] = off[m][i] - off[m][0];
            run.key.assign(keys, keys + n_records);
        } else run.off.assign(1, 0);
        r->runs[m].push_back(std::move(run));
    }
    } catch (const std::bad_alloc &) {          // (a run added to file 1 only is dropped again: the two files keep the same runs)
        if (r->runs[0].size() > r->runs[1].size()) r->runs[0].pop_back();
        return CM_ENOMEM;
    }
    return CM_OK;
}
extern "C" int cm_remain_runs_add_unsorted(cm_remain_runs *r, const void *bytes1, uint64_t n1, const void *bytes2, uint64_t n2) {
    if (!r || (n1 && !bytes1) || (n2 && !bytes2)) return CM_EINVAL;
    const void *bytes[2] = {bytes1, bytes2};
    const uint64_t n[2] = {n1, n2};
    try {
    Run made[2];
    for (int m = 0; m < 2; ++m) {
        RemainFile F;
        F.buf.assign((const char *)bytes[m], (const char *)bytes[m] + n[m]);
        std::vector<SortRec> recs;
        const int rc = order_records(F, recs);
        if (rc != CM_OK) return rc;
        Run &run = made[m];
        run.bytes.reserve(F.buf.size() + 4);
        run.off.push_back(0);
        for (const SortRec &k : recs) {
            const char *p = F.buf.data() + F.start[k.idx];
            size_t len = F.start[k.idx + 1] - F.start[k.idx];
            if (len && p[len - 1] == '\n') --len;
            run.key.push_back(parsed_key(p, len));
            run.bytes.insert(run.bytes.end(), p, p + len);
            for (int x = F.lines[k.idx]; x < 4; ++x) run.bytes.push_back('\n');      // (as cm_sort_remain writes an incomplete group)
            run.bytes.push_back('\n');
            run.off.push_back(run.bytes.size());
        }
    }
    r->runs[0].reserve(r->runs[0].size() + 1);
    r->runs[1].reserve(r->runs[1].size() + 1);
    for (int m = 0; m < 2; ++m) r->runs[m].push_back(std::move(made[m]));
    } catch (const std::bad_alloc &) {
        return CM_ENOMEM;
    }
    return CM_OK;
}
extern "C" int cm_remain_runs_finish(cm_remain_runs *r) {
    if (!r || !r->has_paths) return CM_EINVAL;
    try {
    for (int m = 0; m < 2; ++m) {
        FILE *out = fopen(r->path[m].c_str(), "wb");
        if (!out) return CM_EIO;
        std::vector<char> ob;
        ob.reserve(8u << 20);
        bool bad = false;
        auto flush = [&]() {
            if (!ob.empty() && fwrite(ob.data(), 1, ob.size(), out) != ob.size()) bad = true;
            ob.clear();
        };
        merge_runs(r->runs[m], [&](const char *p, size_t n) {
            ob.insert(ob.end(), p, p + n);
            if (ob.size() > (8u << 20) - 4096) flush();
        });
        flush();
        if (fclose(out) != 0 || bad) return CM_EIO;
    }
    } catch (const std::bad_alloc &) {
        return CM_ENOMEM;
    }
    return CM_OK;
}
extern "C" int cm_remain_runs_finish_mem(cm_remain_runs *r, const void **bytes1, uint64_t *n1, const void **bytes2, uint64_t *n2) {
    if (!r || !bytes1 || !n1 || !bytes2 || !n2) return CM_EINVAL;
    try {
    for (int m = 0; m < 2; ++m) {
        std::vector<char> &ob = r->merged[m];
        ob.clear();
        size_t total = 0;
        for (const Run &run : r->runs[m]) total += run.bytes.size();
        ob.reserve(total);
        merge_runs(r->runs[m], [&](const char *p, size_t n) { ob.insert(ob.end(), p, p + n); });
    }
    } catch (const std::bad_alloc &) {
        return CM_ENOMEM;
    }
    *bytes1 = r->merged[0].data();
    *n1 = r->merged[0].size();
    *bytes2 = r->merged[1].data();
    *n2 = r->merged[1].size();
    return CM_OK;
}
extern "C" void cm_remain_runs_close(cm_remain_runs *r) { delete r; }

extern "C" int cm_circ_report(const cm_circ_res *res, uint64_t n, const char *report_path) {
    if (!report_path || (n && !res)) return CM_EINVAL;
    FILE *f = fopen(report_path, "w");                  // open_report_file: the file exists even without events
    if (!f) return CM_EINVAL;
    if (n == 0) {
        fclose(f);
        return CM_OK;
    }
    std::vector<Call> calls(n);
    for (uint64_t i = 0; i < n; ++i) {
        const cm_circ_res &r = res[i];
        Call &c = calls[i];
        c.chr = r.chr ? r.chr : "";
        c.rname = r.rname ? r.rname : "";
        c.start_signal = r.start_signal ? r.start_signal : "";
        c.end_signal = r.end_signal ? r.end_signal : "";
        c.start_bp_ref = r.start_bp_ref ? r.start_bp_ref : "";
        c.end_bp_ref = r.end_bp_ref ? r.end_bp_ref : "";
        c.spos = r.spos;
        c.epos = r.epos;
        c.type = r.type;
    }
    std::sort(calls.begin(), calls.end());
    std::vector<const Call *> group{&calls[0]};
    for (uint64_t i = 1; i < n; ++i) {
        if (calls[i].same_event(*group[0])) {
            group.push_back(&calls[i]);
        } else {
            report_group(f, group);
            group.assign(1, &calls[i]);
        }
    }
    report_group(f, group);
    const bool bad = ferror(f) != 0;
    return (fclose(f) == 0 && !bad) ? CM_OK : CM_EIO;
}
