// Minimal C++ caller of cm_detect_run (no Python, no torch): FASTQ + index file or packed FASTA + GTF -> every output of the
// reference's default command in one call -- the mapping file (pam | sam), the remain FASTQ, <out>.candidates.pam and
// <out>.circ_report -- with one context and one load of genome and GTF.  Build:
//     g++ -std=c++17 -I include examples/cm_detect.cpp -L circminer_amd/csrc -lcmhot -Wl,-rpath,$PWD/circminer_amd/csrc -o cm_detect
// Usage:  cm_detect <ref>.packed.fa.index <annotation.gtf> <R1.fastq[.gz]> <R2.fastq[.gz]> <out_prefix> [pam|sam|none] [k] [files] [srt]
//         cm_detect <ref>.packed.fa       ...                                                      [pam|sam|none]  k  [files] [srt]
//         (no index file: the k-mer tables are built on the device from the packed FASTA; <ref>.packed.fa.index.info is read as before)
//         files: hand the remain records to stage 2 through the remain / .srt files even where memory would do
//         srt:   also write the two .srt files on the memory hand-over
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "circminer_hot.h"

int main(int argc, char **argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s index gtf r1 r2 out_prefix [pam|sam|none] [k] [files] [srt]\n", argv[0]);
        return 2;
    }
    const std::string src = argv[1];
    const bool is_index = src.size() >= 6 && src.compare(src.size() - 6, 6, ".index") == 0;
    const std::string info = is_index ? src + ".info" : src + ".index.info";
    cm_detect_args a;
    memset(&a, 0, sizeof a);
    a.map.index_path = argv[1];
    a.map.index_info_path = info.c_str();
    a.map.gtf_path = argv[2];
    a.map.fastq1 = argv[3];
    a.map.fastq2 = argv[4];
    a.map.out_prefix = argv[5];
    a.map.report = argc > 6 ? (strcmp(argv[6], "sam") == 0 ? 2 : (strcmp(argv[6], "none") == 0 ? 0 : 1)) : 0;
    a.map.n_threads = 8;
    // defaults of the reference's command line (src/commandline_parser.cpp:7-33); kmer 0 = the index file's k
    a.map.params.kmer = argc > 7 ? atoi(argv[7]) : 0;
    a.map.params.seed_lim = 500;
    a.map.params.max_read_len = 300;
    a.map.params.scan_level = 0;
    a.map.params.max_ed = 4;
    a.map.params.max_sc = 7;
    a.map.params.band = 3;
    a.map.params.max_tlen = 500;
    a.map.params.max_intron = 2000000;
    a.map.params.max_chain_len = 30;
    a.map.params.device = 0;
    for (int i = 8; i < argc; ++i) {
        if (strcmp(argv[i], "files") == 0) a.handover = 1;
        if (strcmp(argv[i], "srt") == 0) a.flags |= 1;
    }
    cm_detect_stats st;
    char err[512];
    const int rc = cm_detect_run(&a, &st, err, sizeof err);
    if (rc != CM_OK) {
        fprintf(stderr, "cm_detect_run (%d): %s\n", rc, err);
        return 1;
    }
    printf("%llu pairs, %d round(s), %llu BSJ candidate pairs; load %.2fs, map %.2fs\n", (unsigned long long)st.map.pairs, st.map.rounds,
           (unsigned long long)st.map.bsj_pairs, st.map.seconds_load, st.map.seconds_map);
    printf("hand-over through %s in %.2fs; stage 2: %llu pairs, %llu problems (%llu refused, %llu recomputed), %llu candidate rows, %llu junction calls in %.2fs; %.2fs in all\n",
           st.handover_used ? "files" : "memory", st.seconds_handover, (unsigned long long)st.circ.pairs, (unsigned long long)st.problems,
           (unsigned long long)st.refused, (unsigned long long)st.recomputed, (unsigned long long)st.circ.candidate_rows, (unsigned long long)st.circ.calls,
           st.circ.seconds, st.seconds_total);
    return 0;
}
