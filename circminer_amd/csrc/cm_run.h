// cm_run.h — what host_mapping.cpp, host_circ_call.cpp and host_detect.cpp share without it being part of the C ABI.
//
// host_mapping.cpp owns the run object (Run): its phases, what they acquire and the one order of release.  cm_mapping_run is
// phases + release; cm_detect_run (host_detect.cpp) is the same phases, then a step of its own while everything stage 2 needs is
// still there -- the context with contig c and its annotation in slot c, the host annotation tables, the chromosome table, the
// host genome bytes and the sorted runs -- and then the same release.
#pragma once
#include <functional>
#include <string>

#include "circminer_hot.h"

namespace cmrun {

// What the path-selecting environment variables select, as fields of the run.  cm_mapping_run fills them from the environment
// (paths_from_environment), cm_detect_run from its own rule.  They are wishes: the input still decides (Run::choose_text_path) --
// gzip, a pipe or carried 23-token headers take the host parser whatever is set here.
struct Paths {
    bool fastq_device = false;       // CM_FASTQ_DEVICE: tokenise on the device
    bool pam_device = false;         // CM_PAM_DEVICE: report 1 on the tokeniser's path, rows formatted on the device
    bool sam_device = false;         // CM_SAM_DEVICE: report 2 likewise
    bool remain_device = false;      // CM_REMAIN_DEVICE: remain records formatted on the device
    bool remain_sorted = false;      // CM_REMAIN_SORTED: every batch's records also as a sorted run
    bool srt_files = false;          // ... and the runs merged into the two .srt files when the batches are through
    bool keep_genome = false;        // each contig's host sequence bytes (genome, ref_len; not the k-mer tables) stay until release
};
Paths paths_from_environment(int32_t report);

// What a run holds when its batches are through and its files are flushed.
struct Resident {
    cm_ctx *cm;
    const cm_params *P;
    uint32_t n_con, n_chr;
    const cm_chr_info *chrs;
    const cm_index_view *genomes;    // n_con views with genome and ref_len only (Paths::keep_genome), else null
    const cm_annot_view *annots;
    cm_remain_runs *runs;            // the batches' sorted runs, not merged yet; null: the run took the host parser or made none
    uint64_t run_batches, run_host_batches, run_records;
    int n_threads;
};
// then: called once after the last batch with everything above alive; its code is the run's, its message goes to `err`
using Then = std::function<int(const Resident &, std::string &err)>;
int mapping_phases(const cm_mapping_args *args, cm_mapping_stats *stats, char *err, uint64_t err_cap, const Paths &paths, const Then *then);

// cm_circ_call_resident with the judges' thread count and the counts CM_CIRC_TRACE prints (problems, refused, recomputed)
int circ_call_resident(cm_ctx *ctx, const cm_params *P, int32_t window_size, uint32_t n_contigs, const cm_index_view *contigs, const cm_annot_view *annots,
                       const cm_chr_info *chrs, uint32_t n_chr, const cm_fastq_batch *sorted, const char *candidates_path, const char *report_path,
                       cm_circ_stats *stats, int n_threads, uint64_t counts[3]);

}  // namespace cmrun
