// Both stages in one call: mapping() then circ_detect() of the reference's default command (src/circminer.cpp), on one run object.
//
// cm_detect_run = the phases of cm_mapping_run (cmrun::mapping_phases, host_mapping.cpp) with the feed chosen by its own rule, then
// -- before the run releases anything -- the hand-over of the remain records to stage 2 and the calling against what stage 1 left
// resident: contig c and its annotation in slot c of the one context, the host annotation tables, the chromosome table and the
// host sequence bytes kept for the judges.  Nothing is loaded twice and no second context is made.
//
// No new kernel: the device work is the tokeniser, the row and remain formatters, the per-batch sort (k_remain_*) and stage 2's
// tables and chains (k_cc_tab_*, k_cc_chain), all of which exist; what is new is residency, the chain workspace owned by the
// context, and the order of the chain calls on the mapping context (behind a cm_sync).
//
// The two hand-overs
//   memory   the run took the device tokeniser's path, so every batch left a sorted run: the runs are merged into two buffers
//            (cm_remain_runs_finish_mem) and parsed from there (cm_fastq_open_mem).  Going through the text keeps `prior` exactly
//            what the file round trip gives -- (int) lengths, the 16-bit junc_num, gm_compatible != 0, the shift -- which is why
//            no binary state is handed over.  flags bit 0 also writes the buffers out as the two .srt files.
//   files    the run took the host parser (gzip, a pipe, carried headers, or handover = 1): cm_sort_remain makes the .srt files
//            of the remain files and they are parsed, as cm_circ_run does it.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <system_error>
#include <thread>

#include "circminer_hot.h"
#include "cm_run.h"

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int write_whole(const std::string &path, const void *p, uint64_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return CM_EIO;
    const bool bad = n && fwrite(p, 1, (size_t)n, f) != (size_t)n;
    return (fclose(f) == 0 && !bad) ? CM_OK : CM_EIO;
}

}  // namespace

extern "C" int cm_detect_run(const cm_detect_args *a, cm_detect_stats *stats, char *err, uint64_t err_cap) {
    auto say = [&](int code, const char *text) {
        if (err && err_cap) snprintf(err, (size_t)err_cap, "%s", text);
        return code;
    };
    if (err && err_cap) err[0] = 0;
    if (!a) return say(CM_EINVAL, "cm_detect_run: null argument");
    if (a->map.world > 1) return say(CM_EINVAL, "cm_detect_run: world must be 0 or 1 (the ranks' runs are not merged)");
    if (a->handover < 0 || a->handover > 1) return say(CM_EINVAL, "cm_detect_run: handover must be 0 (memory) or 1 (files)");
    const int ws = a->window_size > 0 ? a->window_size : 8;
    if (ws < 6 || ws > 10) return say(CM_ELIMIT, "cm_detect_run: window size outside 6 .. 10");
    try {               // (strings and a thread are made below: what they throw does not cross the C ABI)
    const double t0 = now();
    cm_detect_stats S;
    memset(&S, 0, sizeof S);
    S.handover_used = a->handover;
    cmrun::Paths paths;
    paths.keep_genome = true;
    if (a->handover == 0) {                     // the rule: everything the device can do for the input, and the sorted runs kept in memory
        paths.fastq_device = paths.remain_device = paths.remain_sorted = true;
        paths.pam_device = a->map.report == 1;
        paths.sam_device = a->map.report == 2;
    }
    const cmrun::Then then = [&](const cmrun::Resident &R, std::string &msg) -> int {
        const std::string out = a->map.out_prefix, base = out + "_" + std::to_string(R.n_con) + "_remain_R";
        const std::string r1 = base + "1.fastq", r2 = base + "2.fastq", s1 = r1 + ".srt", s2 = r2 + ".srt";
        if (!R.genomes) return msg = "cm_detect_run: the run kept no host sequence", CM_ESTATE;
        const double th = now();
        cm_fastq *fq = nullptr;
        int rc;
        if (R.runs) {
            S.handover_used = 0;
            const void *b1 = nullptr, *b2 = nullptr;
            uint64_t n1 = 0, n2 = 0;
            if ((rc = cm_remain_runs_finish_mem(R.runs, &b1, &n1, &b2, &n2)) != CM_OK) return msg = "cm_remain_runs_finish_mem failed", rc;
            if (getenv("CM_REMAIN_TRACE"))
                fprintf(stderr, "[remain] sorted runs: %llu batches, %llu sorted on the host, %llu records, merge %.3f s\n", (unsigned long long)R.run_batches,
                        (unsigned long long)R.run_host_batches, (unsigned long long)R.run_records, now() - th);
            if ((a->flags & 1) && ((rc = write_whole(s1, b1, n1)) != CM_OK || (rc = write_whole(s2, b2, n2)) != CM_OK)) return msg = "writing the .srt files failed", rc;
            if ((rc = cm_fastq_open_mem(b1, n1, b2, n2, R.chrs, R.n_chr, R.P->max_ed, &fq)) != CM_OK) return msg = "cm_fastq_open_mem failed", rc;
        } else {
            S.handover_used = 1;
            int rc2 = CM_OK;
            std::thread other([&]() { rc2 = cm_sort_remain(r2.c_str(), s2.c_str()); });
            rc = cm_sort_remain(r1.c_str(), s1.c_str());
            other.join();
            if (rc != CM_OK || rc2 != CM_OK) return msg = "cm_sort_remain failed", rc != CM_OK ? rc : rc2;
            if ((rc = cm_fastq_open(s1.c_str(), s2.c_str(), R.chrs, R.n_chr, R.P->max_ed, &fq)) != CM_OK) return msg = "cm_fastq_open (sorted remain files) failed", rc;
        }
        cm_fastq_batch b;
        if ((rc = cm_fastq_next(fq, ~0ull >> 2, &b)) != CM_OK) {
            cm_fastq_close(fq);
            return msg = "cm_fastq_next (sorted remain records) failed", rc;
        }
        S.seconds_handover = now() - th;
        uint64_t counts[3] = {0, 0, 0};
        const std::string cand = out + ".candidates.pam", rep = out + ".circ_report";
        rc = cmrun::circ_call_resident(R.cm, R.P, a->window_size, R.n_con, R.genomes, R.annots, R.chrs, R.n_chr, &b, cand.c_str(), rep.c_str(), &S.circ,
                                       a->circ_threads > 0 ? a->circ_threads : R.n_threads, counts);
        if (rc != CM_OK) msg = std::string("cm_circ_call_resident failed: ") + cm_last_error(R.cm);
        cm_fastq_close(fq);
        S.problems = counts[0];
        S.refused = counts[1];
        S.recomputed = counts[2];
        return rc;
    };
    const int rc = cmrun::mapping_phases(&a->map, &S.map, err, err_cap, paths, &then);
    if (rc == CM_ENODEV) say(rc, "cm_detect_run: no HIP device (CM_ENODEV); both stages run on the device paths and there is no host fall-back");
    S.seconds_total = now() - t0;
    if (stats) *stats = S;
    return rc;
    } catch (const std::bad_alloc &) {
        return say(CM_ENOMEM, "cm_detect_run: out of host memory");
    } catch (const std::system_error &) {
        return say(CM_ENOMEM, "cm_detect_run: a host thread could not be started");
    }
}

extern "C" int cm_detect_abi_sizes(uint32_t *out, uint32_t cap) {
    if (!out || cap < 2) return CM_EINVAL;
    out[0] = (uint32_t)sizeof(cm_detect_args);
    out[1] = (uint32_t)sizeof(cm_detect_stats);
    return 2;
}
