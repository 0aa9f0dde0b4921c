// Stage 1 of CircMiner end to end, on top of the C ABI (the caller of the hot path).
//
// Mirrors mapping() + map_reads() of the reference (src/circminer.cpp:98-352, :354-400): index info -> GTF ->
// one ROUND per packed contig -> per pair the skip / print / write rules of :386-397.  What changes is the order of
// the loops.  The reference streams ALL reads through one contig, writes the survivors to <out>_<r>_remain_R?.fastq,
// loads the next contig and streams those files again.  Here every packed contig is resident in HBM (hg38: ~40 GB of
// 288 GB) and each batch of pairs goes through all rounds back to back on the device, so the only files written are
// the ones a user of the reference keeps:
//   <out>.mapping.pam | .sam            one row (two SAM lines) per pair, with the state it had when it was retired
//                                       (skip) or after the last round -- the same rows the reference prints, in
//                                       another order (the reference's order depends on its thread schedule);
//   <out>_<R>_remain_R{1,2}.fastq       R = number of packed contigs: the CHIBSJ / CHI2BSJ pairs of the last round with
//                                       their 23-token headers, stage 2's input (it sorts them itself).
// A pair retired in round r is left untouched by later rounds (cm_map_round), so its final state is the one the
// reference printed in round r.
//
// Four batches are in flight: batch k-1's rows are being written by a worker thread, batch k is on the GPU, batch k+1 is staged
// (copied over PCIe on the copy stream out of page-locked parser buffers; its first round is seeded and chained under batch k's
// last pair stage, cm_map_rounds) and batch k+2 is being parsed on another worker thread (cm_fastq_next keeps four generations).
// Only what the rows need leaves the device: with report 0 (the reference's default, src/commandline_parser.cpp:26) that is the
// (pair, state) records of the re-queued pairs and a 14-bin type histogram.
//
// With CM_FASTQ_DEVICE=1 and report 0 the parser thread only reads: raw text blocks (cm_fastq_next_text) are tokenised by the device
// (cm_reads_stage_text) and the remain rows of the re-queued pairs are sliced from the text (cm_write_remain_text); same pipeline,
// same files.  Opt-in: see DESIGN.md §7 for what it costs and gains.  With CM_REMAIN_DEVICE=1 beside it those rows are formatted by
// the device as well (cm_format_remain into two of four page-locked buffers, appended with cm_write_bytes / cm_write_bytes2): once a
// batch is staged the host needs none of its read text.  The text blocks still live as long as before; that is a later change.
//
// One process per GPU: rank r of w maps the r-th contiguous block of pairs (cm_fastq_open_shard) and writes .part<r> files;
// cm_merge_parts on rank 0 concatenates them in rank order -- the bytes one process would have written.
//
// The run is one object (Run): cm_mapping_run walks its phases, a phase returns a code, and what the phases acquired -- threads, files,
// page-locked ranges, the context, host tables -- is released by ~Run, in one order, on every way out.
//
// Which feed a run takes is a set of fields (cmrun::Paths, cm_run.h): cm_mapping_run fills them from the environment, cm_detect_run
// (host_detect.cpp) from its own rule.  cmrun::mapping_phases is the walk both share; cm_detect_run hands it a step that runs after
// the last batch and before the release, while the context, the annotation tables, the chromosome table, the sorted runs and --
// kept for it -- each contig's host sequence bytes are still there.  Keeping those bytes costs one byte per base of host memory
// (3.1 GB at hg38 size) for the length of the run; the k-mer tables' host copies go back after each upload as before.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "circminer_hot.h"
#include "cm_pinned_ranges.h"
#include "cm_row_ranges.h"
#include "cm_run.h"

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// results of batch k live in set k & 1: the writer thread of batch k reads them while batch k+1 is downloaded
struct Result {
    std::vector<cm_mapped_read> state;
    std::vector<uint8_t> active;
    std::vector<uint64_t> sel;
    std::vector<cm_record> recs;
    uint64_t n_rec = 0;
    cm_fastq_batch batch;
};
// CM_FASTQ_DEVICE=1: block k in tq[k & 3]: its text is the reader's for three more reads
struct TextBlock {
    const uint8_t *t1 = nullptr, *t2 = nullptr;
    uint64_t l1 = 0, l2 = 0;
    int e1 = 0, e2 = 0;
    cm_text_batch tb{};
    std::vector<uint64_t> rec1, rec2;
};
// one packed contig as its source hands it out: a view (its arrays, or lengths only) and, from a full-format index, the raw record
struct Contig { cm_index_view iv; cm_index_raw raw; };
struct Run;
// what differs between the three sources of the contig loop (Run::load_contigs_from has the rest)
struct ContigSource {
    const char *next_name, *load_name;
    int (*next)(Run &, Contig *, int *loaded);
    int (*load)(Run &, int slot, const Contig &);
    bool frees_host_copy;                          // the contig's arrays are malloc'ed per contig and go back after the upload
    const char *lap_first, *lap_ahead, *lap_load;
};

struct Run {
    const cm_mapping_args *const a;
    const cmrun::Paths paths;
    char *const err;
    const size_t err_cap;
    const char *what = nullptr;                    // the call that failed, for cm_mapping_run's message; null when the text is set already
    cm_mapping_stats st{};
    const double t0 = now();
    double t1 = 0.0;
    int n_threads = 1, world = 1, rank = 0;
    uint64_t batch_pairs = 0, want = 0;            // want: bytes per file and text block
    std::string part;
    const bool trace = getenv("CM_INDEX_TRACE") != nullptr;
    cm_params P;
    int32_t full = 0;
    uint32_t n_con = 0, n_chr = 0;
    std::vector<int> all;
    // ---- what the run owns (~Run) ----
    cm_chr_info *chrs = nullptr;
    cm_index_file *idx = nullptr;
    cm_ctx *cm = nullptr;
    cm_fastq *fq = nullptr;
    cm_writer *w_map = nullptr, *w_rem = nullptr;
    std::vector<cm_index_view> views;
    std::vector<cm_index_view> genomes;                          // Paths::keep_genome: contig c's sequence bytes (genome, ref_len), for stage 2's judges
    std::vector<cm_annot_view> annots, annots_early;             // _early: the GTF thread's, until load_annotation() takes or frees them
    Result res[2];
    RowBuf rows[2];                                // CM_PAM_DEVICE=1 / CM_SAM_DEVICE=1: the rows of batch k as the device formatted them, in set k & 1
    RowBuf rem_rows[2][2];                         // CM_REMAIN_DEVICE=1: the remain records of batch k, file 1 and file 2, in set k & 1
    // CM_REMAIN_SORTED=1 beside it: the same records in cm_sort_remain's order (cm_format_remain_sorted), their offsets and keys; the
    // batches' sorted runs, merged into the .srt files after the last batch
    RowBuf srt_rows[2];
    std::vector<uint32_t> srt_off[2];
    std::vector<int64_t> srt_keys;
    cm_remain_runs *srt_runs = nullptr;
    uint64_t srt_batches = 0, srt_host_batches = 0, srt_records = 0;
    // parser arrays and text blocks registered with the runtime.  The parser tells us (release hook, on its own thread) before one of
    // them is freed -- a generation's array that has to grow is allocated anew -- so that no registration outlives its block.
    PinnedRanges pins;
    std::thread writer, parser, gtf_thread, free_thread;
    // ---- what the threads use: members, so that it outlives every phase's frame until ~Run has joined them ----
    std::vector<uint32_t> clen_guess;
    int early_rc = CM_EINVAL, writer_rc = CM_OK, parser_rc = CM_OK;
    double write_s = 0.0, parse_s = 0.0;           // read after the join
    bool text_path = false, pam_device = false, sam_device = false, remain_device = false, remain_sorted = false, want_fixed = false;
    TextBlock tq[4];
    cm_fastq_batch cur{}, nxt{}, nn{};
    Run(const cm_mapping_args *args, const cmrun::Paths &pt, char *e, uint64_t cap) : a(args), paths(pt), err(e), err_cap((size_t)cap) {
        if (err && err_cap) err[0] = 0;
        pins.user = this;
        pins.reg = [](void *u, void *p, uint64_t bytes) { return cm_host_register(((Run *)u)->cm, p, bytes); };
        pins.unreg = [](void *u, void *p, const char **msg) {
            const int r = cm_host_unregister(((Run *)u)->cm, p);
            if (r != CM_OK) *msg = cm_last_error(((Run *)u)->cm);
            return r;
        };
    }
    // The order is load-bearing.  The threads first: they use everything below.  cm_sync drains the copy stream too, so no copy out
    // of the parser's arrays is in flight when they are unregistered; they are unregistered before cm_fastq_close frees them, so no
    // registration outlives its block; the context goes after the last call that needs it and before the host tables it was fed from.
    ~Run() {
        if (free_thread.joinable()) free_thread.join();
        if (gtf_thread.joinable()) gtf_thread.join();           // it reads chrs
        if (parser.joinable()) parser.join();
        if (writer.joinable()) writer.join();
        if (w_map) cm_writer_close(w_map);
        if (w_rem) cm_writer_close(w_rem);
        for (RowBuf *rb : {&rows[0], &rows[1], &rem_rows[0][0], &rem_rows[0][1], &rem_rows[1][0], &rem_rows[1][1], &srt_rows[0], &srt_rows[1]})
            if (rb->p) (void)cm_host_free(cm, rb->p);
        if (srt_runs) cm_remain_runs_close(srt_runs);
        if (cm) (void)cm_sync(cm);
        pins.clear();
        if (pins.failed)
            fprintf(stderr, "cm_mapping_run: %llu page-locked range(s) could not be unregistered; first: %s\n", (unsigned long long)pins.failed, pins.first_message.c_str());
        if (fq) cm_fastq_close(fq);
        if (cm) cm_destroy(cm);
        if (!annots.empty()) cm_host_free_annotation(annots.data(), (uint32_t)annots.size());
        if (early_rc == CM_OK && !annots_early.empty()) cm_host_free_annotation(annots_early.data(), (uint32_t)annots_early.size());
        for (auto &v : views) cm_host_free_loaded_contig(&v);
        for (auto &v : genomes) cm_host_free_loaded_contig(&v);
        if (idx) cm_host_close_index(idx);
        if (chrs) cm_host_free_index_info(chrs, n_chr);
    }
    // ---- failures: the one place the message is written ----
    int refuse(int code, const char *fmt, ...) {
        if (err && err_cap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(err, err_cap, fmt, ap);
            va_end(ap);
        }
        return code;
    }
    int failed(int rc, const char *name) { return what = name, rc; }          // `rc` of the call `name`: cm_mapping_run names the call
    void lap(const char *text, double since) const { if (trace) fprintf(stderr, "[load] %s %.3f s (at %.3f s)\n", text, now() - since, now() - t0); }
    // ---- phase 1: arguments and refusals ----
    int check_args() {
        if (!a || !a->index_path || !a->index_info_path || !a->gtf_path || !a->fastq1 || !a->fastq2 || !a->out_prefix)
            return refuse(CM_EINVAL, "cm_mapping_run: null argument");
        if (a->report < 0 || a->report > 2) return refuse(CM_EINVAL, "report must be 0 (none), 1 (PAM) or 2 (SAM)");
        n_threads = a->n_threads > 0 ? a->n_threads : 1;
        batch_pairs = a->batch_pairs ? a->batch_pairs : (1ull << 18);
        world = a->world > 1 ? a->world : 1, rank = a->world > 1 ? a->rank : 0;
        if (rank < 0 || rank >= world) return refuse(CM_EINVAL, "rank %d of %d", a->rank, a->world);
        if (world > 1) part = ".part" + std::to_string(rank);
        return CM_OK;
    }
    // ---- phase 2: index info, index file, context (genome_packer.load_index_info, checkHashTable, initLoadingHashTableMeta) ----
    int open_index() {
        int rc;
        if ((rc = cm_host_read_index_info(a->index_info_path, &chrs, &n_chr)) != CM_OK) return failed(rc, "cm_host_read_index_info");
        int32_t kmer = 0;
        uint32_t n_rec = 0;
        if ((rc = cm_host_open_index(a->index_path, &idx, &kmer, &full, &n_rec)) != CM_OK) return failed(rc, "cm_host_open_index");
        P = a->params;
        // full < 0: index_path is the packed FASTA itself, the tables are built on the device
        if (full < 0 && P.kmer == 0)
            return refuse(CM_EINVAL, "%s is a packed FASTA, not an index file: there is no k to read, params.kmer must be given", a->index_path);
        if (P.kmer == 0) P.kmer = kmer;
        if (full >= 0 && P.kmer != kmer) return refuse(CM_EINVAL, "index was built for k = %d, params ask for k = %d", kmer, P.kmer);
        if ((rc = cm_create(&P, &cm)) != CM_OK) return failed(rc, "cm_create");
        lap("index info + header + context", t0);
        return CM_OK;
    }
    // ---- phase 3: every packed contig into its own slot (loadHashTable + pac2char_whole_contig per round in the reference) ----
    // Contig c + 1 is read from the file (host threads) while contig c goes over PCIe and gets its table flattened or built and its
    // bucket descriptors made, and the GTF is parsed meanwhile on a thread of its own: the contig lengths it needs follow from the
    // .index.info rows (a packed contig ends with its last chromosome) and are checked against the index file's afterwards.
    int load_contigs() {
        for (uint32_t i = 0; i < n_chr; ++i) {
            if (chrs[i].contig_id == 0) continue;
            if (clen_guess.size() < chrs[i].contig_id) clen_guess.resize(chrs[i].contig_id, 0);
            clen_guess[chrs[i].contig_id - 1] = std::max(clen_guess[chrs[i].contig_id - 1], chrs[i].start_pos + chrs[i].len);
        }
        annots_early.resize(clen_guess.size());
        if (!clen_guess.empty())
            gtf_thread = std::thread([this]() {
                const double tg = now();
                early_rc = cm_host_build_annotation(a->gtf_path, chrs, n_chr, clen_guess.data(), (uint32_t)clen_guess.size(), P.max_read_len, annots_early.data());
                lap("GTF -> annotation tables (under the contig loads)", tg);
            });
        // no index file: the sequence is read from the packed FASTA (one host thread) and the device builds the table from it
        static const ContigSource from_sequence = {
            "cm_host_next_contig_genome", "cm_build_contig",
            [](Run &r, Contig *c, int *loaded) { return cm_host_next_contig_genome(r.idx, &c->iv, loaded); },
            [](Run &r, int slot, const Contig &c) { return cm_build_contig(r.cm, slot, c.iv.contig_num, c.iv.genome, c.iv.ref_len, nullptr); },
            true, "contig sequence read", "next contig sequence read (under the build)", "contig uploaded, table built on the device + descriptors"};
        // full-format index: the table crosses PCIe as it is in the file and the device flattens it; the host only reads and decodes
        // the bucket headers.  The view holds the lengths only: the arrays stay with the file handle.
        static const ContigSource from_full_index = {
            "cm_host_next_contig_raw", "cm_load_contig_raw",
            [](Run &r, Contig *c, int *loaded) {
                const int rc = cm_host_next_contig_raw(r.idx, r.n_threads, &c->raw, loaded);
                memset(&c->iv, 0, sizeof c->iv);
                if (rc == CM_OK && *loaded) c->iv.contig_num = c->raw.contig_num, c->iv.ref_len = c->raw.ref_len;
                return rc;
            },
            [](Run &r, int slot, const Contig &c) { return cm_load_contig_raw(r.cm, slot, &c.raw); },
            false, "contig record read", "next contig record read (under the upload)", "contig uploaded, flattened on the device + descriptors"};
        // compact index: the host decodes the table.  Its host copy is dead once it is in HBM: returned to the system after each upload,
        // while the next contig is still being decoded, rather than in one 25-GB sweep next to the FASTQ parser's first page faults
        static const ContigSource from_compact_index = {
            "cm_host_next_contig", "cm_load_contig",
            [](Run &r, Contig *c, int *loaded) { return cm_host_next_contig(r.idx, r.n_threads, &c->iv, loaded); },
            [](Run &r, int slot, const Contig &c) { return cm_load_contig(r.cm, slot, &c.iv); },
            true, "contig decoded", "next contig decoded (under the upload)", "contig uploaded + descriptors"};
        const int rc = load_contigs_from(full < 0 ? from_sequence : full ? from_full_index : from_compact_index);
        if (rc != CM_OK) return rc;
        n_con = (uint32_t)views.size();
        return n_con ? CM_OK : refuse(CM_EINVAL, "index file holds no contig");
    }
    int load_contigs_from(const ContigSource &S) {
        Contig nxt;
        int nxt_loaded = 0;
        double tl = now();
        int nxt_rc = S.next(*this, &nxt, &nxt_loaded);
        lap(S.lap_first, tl);
        for (;;) {
            if (nxt_rc != CM_OK) return failed(nxt_rc, S.next_name);
            if (!nxt_loaded) return CM_OK;
            const Contig c = nxt;
            views.push_back(c.iv);
            if (c.iv.contig_num != (int32_t)views.size() - 1)
                return refuse(CM_EINVAL, "packed contigs out of order: record %zu is contig %d", views.size(), c.iv.contig_num + 1);
            std::thread ahead([&]() {                            // (joined below, before anything it writes goes out of scope)
                const double ta = now();
                nxt_rc = S.next(*this, &nxt, &nxt_loaded);
                lap(S.lap_ahead, ta);
            });
            tl = now();
            const int lrc = S.load(*this, (int)views.size() - 1, c);
            lap(S.lap_load, tl);
            if (paths.keep_genome && lrc == CM_OK && !keep_sequence(S, c)) {
                ahead.join();
                if (S.frees_host_copy && nxt_rc == CM_OK && nxt_loaded) cm_host_free_loaded_contig(&nxt.iv);
                return refuse(CM_ENOMEM, "no memory to keep the sequence of contig %d on the host", c.iv.contig_num + 1);
            }
            if (S.frees_host_copy) cm_host_free_loaded_contig(&views.back());
            ahead.join();
            if (lrc == CM_OK) continue;
            if (S.frees_host_copy && nxt_rc == CM_OK && nxt_loaded) cm_host_free_loaded_contig(&nxt.iv);
            return failed(lrc, S.load_name);
        }
    }
    // Paths::keep_genome: the sequence bytes of the contig just uploaded stay with the run.  A source that hands out arrays of its
    // own per contig gives its sequence up (the tables still go back); the full-format source's belong to the file handle: copied.
    bool keep_sequence(const ContigSource &S, const Contig &c) {
        cm_index_view g{};
        g.contig_num = c.iv.contig_num;
        g.ref_len = c.iv.ref_len;
        if (S.frees_host_copy) {
            g.genome = views.back().genome;
            views.back().genome = nullptr;
        } else {
            uint8_t *copy = (uint8_t *)malloc((size_t)c.raw.ref_len + 1);
            if (!copy) return false;
            memcpy(copy, c.raw.genome, c.raw.ref_len);
            copy[c.raw.ref_len] = 0;
            g.genome = copy;
        }
        genomes.push_back(g);
        return true;
    }
    // ---- phase 4: GTF (gtf_parser.init / load_gtf) ----
    int load_annotation() {
        std::vector<uint32_t> clen(n_con);
        for (uint32_t c = 0; c < n_con; ++c) clen[c] = views[c].ref_len;
        if (gtf_thread.joinable()) gtf_thread.join();
        int rc = CM_OK;
        if (early_rc == CM_OK && clen == clen_guess) annots.swap(annots_early);
        else {                                        // .index.info and the index file disagree on the contig lengths: the file decides
            if (early_rc == CM_OK) cm_host_free_annotation(annots_early.data(), (uint32_t)annots_early.size());
            annots_early.clear();
            annots.resize(n_con);
            const double tg = now();
            rc = cm_host_build_annotation(a->gtf_path, chrs, n_chr, clen.data(), n_con, P.max_read_len, annots.data());
            lap("GTF -> annotation tables", tg);
        }
        if (rc != CM_OK) {
            annots.clear();
            return refuse(rc, "cm_host_build_annotation failed (%d)", rc);
        }
        const double tu = now();
        for (uint32_t c = 0; c < n_con; ++c)
            if ((rc = cm_load_annotation(cm, (int)c, &annots[c])) != CM_OK) return failed(rc, "cm_load_annotation");
        lap("annotation uploaded", tu);
        views.clear();                                              // (their arrays went back after each upload)
        // everything is in HBM: the file handle's buffers (two sets of raw records on the full-format path, ~ 19 GB for hg38)
        // are dead weight from here on -- per process, and there is one process per GPU
        // (on a thread of its own: returning that much memory takes about a second, and nothing waits for it)
        free_thread = std::thread([h = idx]() { cm_host_close_index(h); });
        idx = nullptr;
        lap("load done", t0);
        st.rounds = (int32_t)n_con;
        st.seconds_load = now() - t0;
        return CM_OK;
    }
    // ---- phase 5: outputs (FilterRead::init, src/filter.cpp:34-84; SAMOutput::init), the reader, and which of the two feeds it is ----
    int open_reader() {
        const int rc = cm_fastq_open_shard(a->fastq1, a->fastq2, chrs, n_chr, P.max_ed, rank, world, n_threads, &fq, nullptr, nullptr);
        if (rc != CM_OK) return failed(rc, "cm_fastq_open_shard");
        cm_fastq_set_release_hook(fq, [](void *user, const void *ptr, uint64_t bytes) { ((PinnedRanges *)user)->release(ptr, bytes); }, &pins);
        return CM_OK;
    }
    int open_outputs_and_reader() {
        const std::string out = a->out_prefix;
        int rc;
        if (a->report) {
            const std::string path = out + (a->report == 2 ? ".mapping.sam" : ".mapping.pam") + part;
            if ((rc = cm_writer_open(path.c_str(), nullptr, chrs, n_chr, &w_map)) != CM_OK) return failed(rc, "cm_writer_open (mapping)");
            // one header: rank 0's part comes first
            if (a->report == 2 && rank == 0 && (rc = cm_write_sam_header(w_map)) != CM_OK) return failed(rc, "cm_write_sam_header");
        }
        const std::string r1 = out + "_" + std::to_string(n_con) + "_remain_R1.fastq" + part, r2 = out + "_" + std::to_string(n_con) + "_remain_R2.fastq" + part;
        if ((rc = cm_writer_open(r1.c_str(), r2.c_str(), chrs, n_chr, &w_rem)) != CM_OK) return failed(rc, "cm_writer_open (remain)");
        if ((rc = open_reader()) != CM_OK) return rc;
        t1 = now();
        all.resize(n_con);
        for (uint32_t c = 0; c < n_con; ++c) all[c] = (int)c;
        return choose_text_path();
    }
    // The device-side tokeniser's path is opt-in and falls back to the host parser, for the run, where that one is needed.
    int choose_text_path() {
        pam_device = a->report == 1 && paths.pam_device;         // the rows of report 1 formatted on the device: needs the text path
        sam_device = a->report == 2 && paths.sam_device;         // the records of report 2 likewise
        text_path = paths.fastq_device && (a->report == 0 || pam_device || sam_device);
        remain_device = paths.remain_device;                     // the remain records formatted on the device: on the text path, in any report mode it covers
        // bytes per file and block: what batch_pairs records take, first by a guess (a 150-bp record with its name and qualities is
        // ~ 350 bytes), then by what the records of the last batch took -- a block that holds much more than a batch only grows the tail
        want = batch_pairs * 400 + (1u << 16);
        if (const char *eb = getenv("CM_FASTQ_DEVICE_BLOCK")) {
            const unsigned long long v = strtoull(eb, nullptr, 10);
            if (v >= 16) {
                want = v;
                want_fixed = true;
            }
        }
        if (!text_path) return CM_OK;
        // the sorted runs beside the remain files: one process only (the ranks' part files are not merged into one order)
        remain_sorted = remain_device && world <= 1 && paths.remain_sorted;
        const int rc = read_block(tq[0], want);
        if (rc != CM_OK && rc != CM_EINVAL) return failed(rc, "cm_fastq_next_text");
        if (rc == CM_EINVAL) return text_path = false, CM_OK;    // gzip input or a pipe: the host parser's
        // a carried state in the first R1 header (23 tokens): the host parser's, on a reader opened anew
        const uint8_t *p = tq[0].t1, *nl = tq[0].l1 ? (const uint8_t *)memchr(p, '\n', tq[0].l1) : nullptr;
        int nt = 0;
        bool in = false;
        for (const uint8_t *q = p + 1; nl && q < nl; ++q) {
            nt += (*q != ' ' && !in) ? 1 : 0;
            in = *q != ' ';
        }
        if (nt != 23) return CM_OK;
        text_path = false;
        cm_fastq_close(fq);
        fq = nullptr;
        return open_reader();
    }

    // ---- phase 6: batches: write k-1 (worker) | rounds of k (device, driven by this thread) | H2D + first round of k+1 | parse k+2 (worker) ----
    // The steps both feeds share.  Parser: started for batch k+2 if there is one to come, joined at the end of batch k's turn.
    void start_parser(bool more, std::function<int()> job) {
        parser_rc = CM_OK;
        parse_s = 0.0;
        if (more)
            parser = std::thread([this, job]() {
                const double tp = now();
                parser_rc = job();
                parse_s = now() - tp;
            });
    }
    int join_parser(const char *name) {
        if (parser.joinable()) parser.join();
        st.seconds_parse += parse_s;
        return parser_rc == CM_OK ? CM_OK : failed(parser_rc, name);
    }
    // the rows of batch k-1 are out (file order = batch order); those of batch k, if there is a job, go to a writer of their own
    int hand_to_writer(std::function<int()> job) {
        if (writer.joinable()) writer.join();
        if (writer_rc != CM_OK) return failed(writer_rc, "writer");
        if (job)
            writer = std::thread([this, job]() {
                const double tw = now();
                writer_rc = job();
                write_s += now() - tw;
            });
        return CM_OK;
    }
    // report 0: only the (pair, state) records of the re-queued pairs and the type histogram leave the device
    int collect_records(Result &R, uint64_t n) {
        int rc;
        if (R.recs.size() < n) R.recs.resize(n);
        if ((rc = cm_collect_records(cm, 0, n, R.recs.data(), &R.n_rec)) != CM_OK) return failed(rc, "cm_collect_records");
        uint64_t h[14];
        if ((rc = cm_type_histogram(cm, h)) != CM_OK) return failed(rc, "cm_type_histogram");
        for (int t = 0; t < 14; ++t) st.by_type[t] += h[t];
        return CM_OK;
    }
    // batch k's results are on the host: the staged batch becomes the resident one, and the books
    int end_device_leg(const Result &R, uint64_t n, bool more, double td) {
        const int rc = more ? cm_reads_swap(cm) : CM_OK;
        if (rc != CM_OK) return failed(rc, "cm_reads_swap");
        st.seconds_device += now() - td;
        st.pairs += n;
        st.bsj_pairs += R.n_rec;
        return CM_OK;
    }
    // page-lock the parser's arrays of a batch (they are reused every fourth batch; re-registered only when one has moved or grown)
    int stage_batch(const cm_fastq_batch &b) {
        const uint64_t n = b.reads.n_pairs;
        pins.cover(b.reads.seq1, b.reads.off1[n]);
        pins.cover(b.reads.seq2, b.reads.off2[n]);
        pins.cover(b.reads.off1, (n + 1) * sizeof(uint64_t));
        pins.cover(b.reads.off2, (n + 1) * sizeof(uint64_t));
        const int rc = cm_reads_stage(cm, &b.reads, b.prior);
        return rc == CM_OK ? CM_OK : failed(rc, "cm_reads_stage");
    }
    int host_batches() {
        int rc;
        const double tp = now();
        if ((rc = cm_fastq_next(fq, batch_pairs, &cur)) != CM_OK) return failed(rc, "cm_fastq_next");
        if (cur.reads.n_pairs && (rc = cm_fastq_next(fq, batch_pairs, &nxt)) != CM_OK) return failed(rc, "cm_fastq_next");
        st.seconds_parse += now() - tp;
        if (cur.reads.n_pairs) {
            if ((rc = stage_batch(cur)) != CM_OK) return rc;
            if ((rc = cm_reads_swap(cm)) != CM_OK) return failed(rc, "cm_reads_swap");
        }
        for (uint64_t k = 0; cur.reads.n_pairs; ++k) {
            const uint64_t n = cur.reads.n_pairs;
            Result &R = res[k & 1];
            const bool more = nxt.reads.n_pairs != 0;
            memset(&nn, 0, sizeof nn);
            start_parser(more, [this]() { return cm_fastq_next(fq, batch_pairs, &nn); });
            const double td = now();
            if (more && (rc = stage_batch(nxt)) != CM_OK) return rc;
            if ((rc = cm_map_rounds(cm, all.data(), (int)n_con, 1)) != CM_OK) return failed(rc, "cm_map_rounds");          // round r + 1 seeds while r pairs
            // results of batch k: rows of every pair (PAM / SAM) or just the re-queued pairs' records
            if (a->report) {
                R.state.resize(n);
                R.active.resize(n);
                if ((rc = cm_reads_download(cm, R.state.data(), nullptr, R.active.data())) != CM_OK) return failed(rc, "cm_reads_download");
                R.sel.clear();
                for (uint64_t i = 0; i < n; ++i) {
                    if (R.active[i]) R.sel.push_back(i);
                    const int t = R.state[i].type;
                    if (t >= 0 && t < 14) ++st.by_type[t];
                }
                R.n_rec = R.sel.size();
            } else if ((rc = collect_records(R, n)) != CM_OK) return rc;
            if ((rc = end_device_leg(R, n, more, td)) != CM_OK) return rc;
            R.batch = cur;
            // map_reads, src/circminer.cpp:386-397: printed if (skip || last round) = every pair by now;
            // written to the remain files if still active after the last round = CHIBSJ / CHI2BSJ
            rc = hand_to_writer([this, &R]() {
                int r = CM_OK;
                if (a->report == 1) r = cm_write_pam(w_map, &R.batch, R.state.data(), nullptr, 0);
                if (a->report == 2) r = cm_write_sam(w_map, &R.batch, R.state.data(), nullptr, 0);
                if (r != CM_OK || !R.n_rec) return r;
                return a->report ? cm_write_remain(w_rem, &R.batch, R.state.data(), R.sel.data(), R.sel.size())
                                 : cm_write_remain_records(w_rem, &R.batch, R.recs.data(), R.n_rec);
            });
            if (rc != CM_OK || (rc = join_parser("cm_fastq_next")) != CM_OK) return rc;
            cur = nxt;
            nxt = nn;
        }
        return CM_OK;
    }

    // ---- the device-side tokeniser's feed: read k+2 (worker) | stage k+1 | rounds of k (+ its rows with CM_PAM_DEVICE=1 / CM_SAM_DEVICE=1) | write k-1 (worker) ----
    int read_block(TextBlock &B, uint64_t bytes) { return cm_fastq_next_text(fq, bytes, &B.t1, &B.l1, &B.e1, &B.t2, &B.l2, &B.e2); }
    // block -> staged batch; B.tb.n_pairs == 0: the input is at its end.  A block that holds no whole pair is read again, larger.
    int stage_block(TextBlock &B) {
        uint64_t bytes = want;
        for (;;) {
            memset(&B.tb, 0, sizeof B.tb);
            if (B.l1 == 0 && B.e1) return CM_OK;                 // R1 is through (what is left of R2 is surplus)
            B.rec1.resize(batch_pairs + 1);
            B.rec2.resize(batch_pairs + 1);
            pins.cover(B.t1, B.l1);                              // (the same buffer handed out at another offset: widened to cover both)
            pins.cover(B.t2, B.l2);
            int r = cm_reads_stage_text(cm, B.t1, B.l1, B.t2, B.l2, batch_pairs, (B.e1 ? 1u : 0u) | (B.e2 ? 2u : 0u) | (pam_device ? 4u : 0u) | (sam_device ? 12u : 0u) | (remain_device ? 28u : 0u), B.rec1.data(), B.rec2.data(), &B.tb);
            if (r != CM_OK) return r;
            if (B.tb.n_pairs) {
                if (!want_fixed) want = std::max(B.tb.used1, B.tb.used2) / B.tb.n_pairs * batch_pairs / 100 * 101 + (1u << 16);
                return cm_fastq_text_consumed(fq, B.tb.used1, B.tb.used2);
            }
            if (B.e1 && B.e2) return CM_OK;                      // (nothing more to read: no whole pair is left)
            bytes *= 2;
            if ((r = cm_fastq_text_consumed(fq, 0, 0)) != CM_OK || (r = read_block(B, bytes)) != CM_OK) return r;
        }
    }
    // a larger page-locked buffer with what the old one holds
    int grow_rows(RowBuf &RB, uint64_t cap) {
        void *np = nullptr;
        const int r = cm_host_alloc(cm, cap, &np);
        if (r != CM_OK) return failed(r, "cm_host_alloc (rows)");
        if (RB.n) memcpy(np, RB.p, RB.n);
        if (RB.p) (void)cm_host_free(cm, RB.p);
        RB.p = np;
        RB.cap = cap;
        return CM_OK;
    }
    std::function<int(RowBuf &, uint64_t)> grower() { return [this](RowBuf &RB, uint64_t cap) { return grow_rows(RB, cap); }; }
    // Three users of format_ranges (cm_row_ranges.h: halved ranges, grown buffers).  First the PAM rows or SAM records of the resident batch's n pairs, appended to RB.
    // A SAM pair is its name and its reads twice over (~ 800 bytes for 2 x 150 bp, eight PAM rows): ranges of 2^17 pairs keep the formatter's device buffer near 100 MB.
    int format_rows(RowBuf &RB, uint64_t n) {
        const auto format = sam_device ? cm_format_sam : cm_format_pam;
        const char *const name = sam_device ? "cm_format_sam" : "cm_format_pam";
        return format_ranges(&RB, 1, &n, sam_device ? 1ull << 17 : 1ull << 22,
                             {[&](uint64_t first, uint64_t count, uint64_t got[2], uint64_t *) { return format(cm, chrs, n_chr, first, count, RB.tail(), RB.room(), got, nullptr); },
                              grower(), nullptr, [&](int r, bool) { return failed(r, name); }});
    }
    // CM_REMAIN_DEVICE=1: the remain records of the resident batch's active set, appended to the two page-locked buffers of a set
    // (file 1, file 2) -- to the end of the set in one call, whose size the first call tells.  *n_rec: that size (the run's bsj_pairs).
    int format_remain(RowBuf RM[2], uint64_t *n_rec) {
        RM[0].n = RM[1].n = 0;
        *n_rec = ~0ull;
        return format_ranges(RM, 2, n_rec, ~0ull,
                             {[&](uint64_t first, uint64_t count, uint64_t got[2], uint64_t *total) {
                                  return cm_format_remain(cm, chrs, n_chr, first, count, RM[0].tail(), RM[0].room(), RM[1].tail(), RM[1].room(), got, nullptr, total, nullptr);
                              },
                              grower(), nullptr, [&](int r, bool) { return failed(r, "cm_format_remain"); }});
    }
    // CM_REMAIN_SORTED=1: the batch's records once more, in cm_sort_remain's order, every range from the start of srt_rows into a run of srt_runs
    // (consecutive ranges of one order are runs like any other).  A batch the device refuses for a tie group is ordered here, from the unsorted records RM holds.
    int sorted_run(RowBuf RM[2], uint64_t n_rec) {
        int r;
        ++srt_batches;
        srt_records += n_rec;
        if (!n_rec) return CM_OK;
        for (int m = 0; m < 2; ++m) {
            srt_rows[m].n = 0;
            if (srt_rows[m].cap < RM[m].n && (r = grow_rows(srt_rows[m], RM[m].n + (1u << 16))) != CM_OK) return r;
        }
        return format_ranges(srt_rows, 2, &n_rec, ~0ull,
                             {[&](uint64_t first, uint64_t count, uint64_t got[2], uint64_t *) {
                                  for (auto &o : srt_off) o.resize(count + 1);
                                  srt_keys.resize(count);
                                  return cm_format_remain_sorted(cm, chrs, n_chr, first, count, srt_rows[0].p, srt_rows[0].cap, srt_rows[1].p, srt_rows[1].cap, got,
                                                                 srt_keys.data(), srt_off[0].data(), srt_off[1].data(), nullptr, nullptr);
                              },
                              grower(),
                              [&](uint64_t c) {
                                  const int a = cm_remain_runs_add(srt_runs, srt_rows[0].p, srt_off[0].data(), srt_rows[1].p, srt_off[1].data(), srt_keys.data(), c);
                                  srt_rows[0].n = srt_rows[1].n = 0;            // (the run keeps its own copy: the next range starts at byte 0 again)
                                  return a != CM_OK ? failed(a, "cm_remain_runs_add") : a;
                              },
                              [&](int r, bool tie_group) {
                                  if (!tie_group) return failed(r, "cm_format_remain_sorted");
                                  ++srt_host_batches;
                                  const int a = cm_remain_runs_add_unsorted(srt_runs, RM[0].p, RM[0].n, RM[1].p, RM[1].n);
                                  return a != CM_OK ? failed(a, "cm_remain_runs_add_unsorted") : a;
                              }});
    }
    // ... and the type histogram, which collect_records delivers on the other path
    int remain_records(Result &R, RowBuf RM[2]) {
        int rc;
        if ((rc = format_remain(RM, &R.n_rec)) != CM_OK) return rc;
        if (remain_sorted && (rc = sorted_run(RM, R.n_rec)) != CM_OK) return rc;
        uint64_t h[14];
        if ((rc = cm_type_histogram(cm, h)) != CM_OK) return failed(rc, "cm_type_histogram");
        for (int t = 0; t < 14; ++t) st.by_type[t] += h[t];
        return CM_OK;
    }
    int text_batches() {
        int rc;
        bool more = false;
        const double td0 = now();
        if ((rc = stage_block(tq[0])) != CM_OK) return failed(rc, "cm_reads_stage_text");
        st.seconds_device += now() - td0;
        if (remain_sorted) {
            const std::string base = std::string(a->out_prefix) + "_" + std::to_string(n_con) + "_remain_R";
            rc = paths.srt_files ? cm_remain_runs_open((base + "1.fastq.srt").c_str(), (base + "2.fastq.srt").c_str(), &srt_runs) : cm_remain_runs_open(nullptr, nullptr, &srt_runs);
            if (rc != CM_OK) return failed(rc, "cm_remain_runs_open");
        }
        if (tq[0].tb.n_pairs) {
            if ((rc = cm_reads_swap(cm)) != CM_OK) return failed(rc, "cm_reads_swap");
            const double tp = now();
            if ((rc = read_block(tq[1], want)) != CM_OK) return failed(rc, "cm_fastq_next_text");
            st.seconds_parse += now() - tp;
            more = true;
        }
        for (uint64_t k = 0; tq[k & 3].tb.n_pairs; ++k) {
            TextBlock &B = tq[k & 3], &N = tq[(k + 1) & 3];
            const uint64_t n = B.tb.n_pairs;
            ++st.device_parsed_batches;
            Result &R = res[k & 1];
            RowBuf &RB = rows[k & 1];
            const double td = now();
            if (more) {
                if ((rc = stage_block(N)) != CM_OK) return failed(rc, "cm_reads_stage_text");
                more = N.tb.n_pairs != 0;
            } else memset(&N.tb, 0, sizeof N.tb);
            start_parser(more, [this, k]() { return read_block(tq[(k + 2) & 3], want); });
            if ((rc = cm_map_rounds(cm, all.data(), (int)n_con, 1)) != CM_OK) return failed(rc, "cm_map_rounds");
            RB.n = 0;
            if ((pam_device || sam_device) && (rc = format_rows(RB, n)) != CM_OK) return rc;
            RowBuf *const RM = rem_rows[k & 1];
            if ((rc = remain_device ? remain_records(R, RM) : collect_records(R, n)) != CM_OK || (rc = end_device_leg(R, n, more, td)) != CM_OK) return rc;
            rc = hand_to_writer([this, &R, &B, &RB, RM]() {
                int r = (pam_device || sam_device) ? cm_write_bytes(w_map, RB.p, RB.n) : CM_OK;
                if (r != CM_OK || !R.n_rec) return r;
                if (!remain_device) return cm_write_remain_text(w_rem, B.t1, B.rec1.data(), B.t2, B.rec2.data(), R.recs.data(), R.n_rec);
                return (r = cm_write_bytes(w_rem, RM[0].p, RM[0].n)) != CM_OK ? r : cm_write_bytes2(w_rem, RM[1].p, RM[1].n);
            });
            if (rc != CM_OK || (rc = join_parser("cm_fastq_next_text")) != CM_OK) return rc;
        }
        return CM_OK;
    }
    // ---- phase 7: the last rows, and the books (a full disk is an error, not a short file) ----
    int finish(cm_mapping_stats *stats) {
        int rc;
        if ((rc = hand_to_writer(nullptr)) != CM_OK) return rc;
        if (w_map && (rc = cm_writer_flush(w_map)) != CM_OK) return failed(rc, "writing the mapping file");
        if ((rc = cm_writer_flush(w_rem)) != CM_OK) return failed(rc, "writing the remain files");
        if (srt_runs && paths.srt_files) {
            const double tm = now();
            if ((rc = cm_remain_runs_finish(srt_runs)) != CM_OK) return failed(rc, "cm_remain_runs_finish (the .srt files)");
            if (getenv("CM_REMAIN_TRACE"))
                fprintf(stderr, "[remain] sorted runs: %llu batches, %llu sorted on the host, %llu records, merge %.3f s\n", (unsigned long long)srt_batches,
                        (unsigned long long)srt_host_batches, (unsigned long long)srt_records, now() - tm);
        }
        st.seconds_map = now() - t1;
        st.seconds_write = write_s;
        if (stats) *stats = st;
        return CM_OK;
    }
    // ---- phase 8 (cm_detect_run only): the caller's step, with everything stage 2 needs still held ----
    int hand_over(const cmrun::Then &then) {
        // finish() has flushed the files; they are closed here because stage 2 may read the remain files
        if (w_map) cm_writer_close(w_map);
        if (w_rem) cm_writer_close(w_rem);
        w_map = w_rem = nullptr;
        const cmrun::Resident R{cm, &P, n_con, n_chr, chrs, genomes.size() == n_con ? genomes.data() : nullptr, annots.data(), srt_runs,
                                srt_batches, srt_host_batches, srt_records, n_threads};
        std::string msg;
        const int rc = then(R, msg);
        return rc == CM_OK ? CM_OK : refuse(rc, "%s", msg.c_str());
    }
};

}  // namespace

cmrun::Paths cmrun::paths_from_environment(int32_t report) {
    auto is_one = [](const char *name) {
        const char *e = getenv(name);
        return e && atoi(e) == 1;
    };
    Paths p;
    p.fastq_device = is_one("CM_FASTQ_DEVICE");
    p.pam_device = report == 1 && is_one("CM_PAM_DEVICE");
    p.sam_device = report == 2 && is_one("CM_SAM_DEVICE");
    p.remain_device = is_one("CM_REMAIN_DEVICE");
    p.remain_sorted = p.srt_files = is_one("CM_REMAIN_SORTED");
    return p;
}

int cmrun::mapping_phases(const cm_mapping_args *a, cm_mapping_stats *stats, char *err, uint64_t err_cap, const Paths &paths, const Then *then) {
    Run run(a, paths, err, err_cap);
    int rc;
    if ((rc = run.check_args()) == CM_OK && (rc = run.open_index()) == CM_OK && (rc = run.load_contigs()) == CM_OK &&
        (rc = run.load_annotation()) == CM_OK && (rc = run.open_outputs_and_reader()) == CM_OK &&
        (rc = run.text_path ? run.text_batches() : run.host_batches()) == CM_OK && (rc = run.finish(stats)) == CM_OK && then)
        rc = run.hand_over(*then);
    // a call that failed is named here, with what the context says of it, while there still is a context; ~Run releases the rest
    if (rc != CM_OK && run.what) run.refuse(rc, "%s failed (%d)%s%s", run.what, rc, run.cm ? ": " : "", run.cm ? cm_last_error(run.cm) : "");
    return rc;
}

extern "C" int cm_mapping_run(const cm_mapping_args *a, cm_mapping_stats *stats, char *err, uint64_t err_cap) {
    return cmrun::mapping_phases(a, stats, err, err_cap, cmrun::paths_from_environment(a ? a->report : 0), nullptr);
}

extern "C" int cm_merge_parts(const char *out_prefix, int32_t rounds, int32_t world, int32_t report) {
    if (!out_prefix || rounds < 1 || world < 1 || report < 0 || report > 2) return CM_EINVAL;
    if (world == 1) return CM_OK;
    const std::string out = out_prefix;
    std::vector<std::string> names = {out + "_" + std::to_string(rounds) + "_remain_R1.fastq", out + "_" + std::to_string(rounds) + "_remain_R2.fastq"};
    if (report) names.push_back(out + (report == 2 ? ".mapping.sam" : ".mapping.pam"));
    std::vector<char> buf(8u << 20);
    for (const std::string &name : names) {
        FILE *dst = fopen(name.c_str(), "wb");
        if (!dst) return CM_EIO;
        for (int r = 0; r < world; ++r) {
            const std::string pn = name + ".part" + std::to_string(r);
            FILE *src = fopen(pn.c_str(), "rb");
            if (!src) {
                fclose(dst);
                return CM_EINVAL;                             // a rank has not written its part
            }
            size_t got;
            while ((got = fread(buf.data(), 1, buf.size(), src)) > 0)
                if (fwrite(buf.data(), 1, got, dst) != got) {
                    fclose(src);
                    fclose(dst);
                    return CM_EIO;
                }
            const bool bad = ferror(src) != 0;
            fclose(src);
            if (bad) {
                fclose(dst);
                return CM_EIO;
            }
        }
        if (fclose(dst) != 0) return CM_EIO;
        for (int r = 0; r < world; ++r) remove((name + ".part" + std::to_string(r)).c_str());
    }
    return CM_OK;
}

// sizeof of every struct that crosses the ABI, in the order of the header: lets a binding (ctypes, cgo, JNI) check its mirrors
extern "C" int cm_abi_sizes(uint32_t *out, uint32_t cap) {
    const uint32_t v[] = {(uint32_t)sizeof(cm_params),       (uint32_t)sizeof(cm_index_view),  (uint32_t)sizeof(cm_annot_view), (uint32_t)sizeof(cm_mapped_read),
                          (uint32_t)sizeof(cm_reads),        (uint32_t)sizeof(cm_record),      (uint32_t)sizeof(cm_chr_info),   (uint32_t)sizeof(cm_fastq_batch),
                          (uint32_t)sizeof(cm_mapping_args), (uint32_t)sizeof(cm_mapping_stats), (uint32_t)sizeof(cm_circ_res), (uint32_t)sizeof(cm_circ_args),
                          (uint32_t)sizeof(cm_circ_stats), (uint32_t)sizeof(cm_index_raw), (uint32_t)sizeof(cm_build_stats),
                          (uint32_t)sizeof(cm_dp_req), (uint32_t)sizeof(cm_dp_res), (uint32_t)sizeof(cm_annot_req), (uint32_t)sizeof(cm_annot_res)};
    const uint32_t n = (uint32_t)(sizeof v / sizeof v[0]);
    if (!out || cap < n) return CM_EINVAL;
    for (uint32_t i = 0; i < n; ++i) out[i] = v[i];
    return (int)n;
}
