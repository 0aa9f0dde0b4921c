/*
 * circminer_hot.h — C-ABI of the MI355X-native CircMiner mapping hot path.
 *
 * The reference (CircMiner 0.4.5) has no plugin/FFI boundary: the seam this
 * library replaces is
 *
 *     int FilterRead::process_read(int thid, Record* r1, Record* r2, int kmer_size,
 *                                  GIMatchedKmer* fl, GIMatchedKmer* bl,
 *                                  chain_list& fbc_r1, chain_list& bbc_r1,
 *                                  chain_list& fbc_r2, chain_list& bbc_r2)
 *                                                       (src/filter.h:49-52, src/filter.cpp:124-241)
 *
 * called once per read pair from map_reads (src/circminer.cpp:384), together with the
 * process-wide state it reads: the loaded mrsfast k-mer table (src/mrsfast/HashTable.c:971-1098),
 * the decoded contig string (src/match_read.cpp:288-299,334), the GTF model
 * (src/gene_annotation.{h,cpp}) and the threshold globals (src/common.h:92-103).
 *
 * Everything here is plain C: pointers, sizes, PODs.  No C++ / torch types.
 * All functions return 0 on success or a negative CM_E* code; none of them calls exit().
 */
#ifndef CIRCMINER_HOT_H
#define CIRCMINER_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- category codes: src/common.h:59-72 (the order matters) ---- */
enum {
    CM_CONCRD = 0, CM_DISCRD = 1, CM_CHIORF = 2, CM_CHIBSJ = 3, CM_CHI2BSJ = 4, CM_CONGEN = 5,
    CM_CHIFUS = 6, CM_CONGNM = 7, CM_OEA2 = 8, CM_CANDID = 9, CM_OEANCH = 10, CM_ORPHAN = 11,
    CM_NOPROC_MANYHIT = 12, CM_NOPROC_NOMATCH = 13
};

/* ---- error codes ---- */
enum {
    CM_OK = 0,
    CM_EINVAL = -1,     /* bad argument / unsupported parameter combination            */
    CM_ENODEV = -2,     /* no HIP device (the product path never falls back to the CPU) */
    CM_ENOMEM = -3,     /* host or device allocation failed                             */
    CM_EHIP = -4,       /* a HIP runtime call or kernel failed                          */
    CM_ESTATE = -5,     /* contig / annotation not loaded                               */
    CM_ELIMIT = -6,     /* a documented capacity limit of the device path was exceeded  */
    CM_EIO = -7         /* a read from an input file or a write to an output file failed */
};

#define CM_WINDOW_SIZE 14          /* WINDOW_SIZE, src/common.cpp:7                         */
#define CM_BESTCHAINLIM 30         /* BESTCHAINLIM, src/common.h:51; chain.h:14-17          */
#ifndef CM_MAX_CHAIN_FRAGS         /* (the library's second build of the kernels sets 24 for itself: reads of more than 16 seeds) */
#define CM_MAX_CHAIN_FRAGS 16      /* fragments a cm_chain of THIS ABI holds (cm_chain_batch, a test hook, is limited to reads of <= 16 seeds) */
#endif
#define CM_MAX_SEEDS_PER_READ 24   /* floor(read length / k) the mapping entry points accept: 300 bp at k = 14 is 21 (commandline_parser.cpp:14,242-247) */
#define CM_CONTIG_SIZE 1100000000u /* DEF_CONTIG_SIZE, src/common.h:81 (gspos stride)       */

/* ---- thresholds: the reference keeps these as globals (src/common.h:92-103,
 *      defaults src/commandline_parser.cpp:7-33) ---- */
typedef struct cm_params {
    int32_t kmer;            /* WINDOW_SIZE + checkSumLength, 14..22 (src/commandline_parser.cpp:242-247) */
    int32_t seed_lim;        /* seedLim       default 500     */
    int32_t max_read_len;    /* maxReadLength default 300     */
    int32_t scan_level;      /* scanLevel     default 0       */
    int32_t max_ed;          /* maxEd         default 4       */
    int32_t max_sc;          /* maxSc         default 7       */
    int32_t band;            /* bandWidth     default 3       */
    int32_t max_tlen;        /* maxTlen       default 500     */
    int32_t max_intron;      /* maxIntronLen  default 2000000 */
    int32_t max_chain_len;   /* maxChainLen   default 30 (must be <= CM_BESTCHAINLIM, see chain.h:14-17) */
    int32_t device;          /* HIP device ordinal            */
    int32_t reserved;
} cm_params;

/* ---- one packed contig of the k-mer index, as loadHashTable leaves it in memory
 *      (src/mrsfast/HashTable.c:971-1057) but flattened: bucket hv owns entries
 *      [bucket_off[hv], bucket_off[hv+1]) sorted by (checksum, pos)
 *      (src/mrsfast/Sort.c:116-117); pos is the 1-based k-mer start
 *      (HashTable.c:785-806).  genome is what pac2char serves
 *      (src/match_read.cpp:288-299): ASCII, genome[p-1] = base at 1-based p. ---- */
typedef struct cm_index_view {
    int32_t contig_num;          /* contigNum = atoi(contigName)-1, src/circminer.cpp:266-268 */
    uint32_t ref_len;            /* getRefGenLength()                                         */
    const uint8_t *genome;       /* ref_len bytes, 'A','C','G','T','N'                        */
    const uint32_t *bucket_off;  /* 4^14 + 1 offsets                                          */
    const uint16_t *checksum;    /* n_entries                                                 */
    const uint32_t *pos;         /* n_entries                                                 */
    uint64_t n_entries;
} cm_index_view;

/* ---- flattened query side of GTFParser for one packed contig
 *      (src/gene_annotation.{h,cpp}, src/interval_tree_impl.h) ---- */
typedef struct cm_annot_view {
    /* disjoint intervals, ascending (FlatIntervalTree::disjoint_intervals) */
    uint32_t n_iv;
    const uint32_t *iv_spos, *iv_epos;
    const uint32_t *iv_max_end, *iv_min_end, *iv_max_next_exon; /* interval_tree_impl.h:198-211 */
    const uint32_t *iv_seg_off;  /* n_iv+1 : CSR into iv_seg                                   */
    const uint32_t *iv_seg;      /* indices into the unique-segment tables, seg_list order     */
    /* unique segments (UniqSeg, src/common.h:227-251) */
    uint32_t n_seg;
    const uint32_t *seg_start, *seg_end, *seg_next_exon_beg, *seg_gene_id;
    const uint32_t *seg_tid_off; /* n_seg+1 : CSR into seg_tid (trans_id vector order)         */
    const uint32_t *seg_tid;
    /* transcripts */
    uint32_t n_trans;
    const int32_t *trans_start_ind;  /* get_trans_start_ind, gene_annotation.h:143-145         */
    const uint32_t *t2s_off;         /* n_trans+1 : CSR into t2s                               */
    const uint8_t *t2s;              /* trans2seg states 0/1/2/3, interval_tree_impl.h:232-241 */
    /* genes (gid2ginfo, src/gene_annotation.cpp:243-245) */
    uint32_t n_gene;
    const uint32_t *gene_start, *gene_end;
    /* position bitsets (src/common.h:117-118); bit p = contig position p, p < n_bits; each array holds (n_bits + 63) / 64 words */
    uint64_t n_bits;
    const uint64_t *near_border_bits;
    const uint64_t *intronic_bits;
    /* chromosomes packed into this contig, ascending by shift (con2chr, gene_annotation.cpp:424-457) */
    uint32_t n_chr;
    const uint32_t *chr_shift;   /* ContigLen.start_pos                                        */
    const int32_t *chr_id;       /* global chromosome ordinal (row of .index.info)             */
    /* optional accelerator for FlatIntervalTree::search (interval_tree_impl.h:136-150): iv_bucket[b] =
     * number of intervals with spos < (b << iv_bucket_shift), b = 0 .. n_iv_bucket-1 (covers n_bits + one
     * extra bucket).  NULL = plain binary search.  Results are identical either way. */
    const uint32_t *iv_bucket;
    uint32_t iv_bucket_shift, n_iv_bucket;
    /* genes_int_map (stage 2 only, never uploaded: GTFParser::get_gene_overlap, src/gene_annotation.cpp:572-585): disjoint
     * intervals over the gene spans; interval i is covered by the genes giv_gene[giv_gene_off[i] .. giv_gene_off[i+1]) in the
     * reference's seg_list order (indices into gene_start / gene_end; genes with identical spans are represented by the
     * first of them, as in the reference's map keyed by (start, end)) */
    uint32_t n_giv;
    const uint32_t *giv_spos, *giv_epos, *giv_gene_off, *giv_gene;
} cm_annot_view;

/* ---- POD mirror of MatchedRead (src/common.h:311-352); carried between rounds through the
 *      23-token FASTQ header in the reference (src/filter.cpp:413-455, fastq_parser.cpp:203-269).
 *      chr_r1 == chr_r2 always (src/common.cpp:295-296) so one chr_id is kept; -1 is "-". ---- */
typedef struct cm_mapped_read {
    uint32_t spos_r1, spos_r2, epos_r1, epos_r2;
    uint32_t qspos_r1, qspos_r2, qepos_r1, qepos_r2;
    uint32_t mlen_r1, mlen_r2;
    int32_t ed_r1, ed_r2;
    int32_t type;
    int32_t tlen;
    int32_t contig_num;
    int32_t chr_id;
    uint16_t junc_num;
    uint8_t r1_forward, r2_forward, gm_compatible, pad[3];
} cm_mapped_read;

/* ---- one chain (chain_t, src/common.h:150-154) as produced by chain_seeds_sorted_kbest ---- */
typedef struct cm_chain {
    float score;
    uint32_t chain_len;
    uint32_t rpos[CM_MAX_CHAIN_FRAGS];
    int32_t qpos[CM_MAX_CHAIN_FRAGS];   /* fragment_t.len is always kmer (src/chain.cpp:265,293) */
} cm_chain;

typedef struct cm_ctx cm_ctx;

/* Reads are passed as concatenated upper/lower-case ASCII with offsets:
 * pair i = R1 bytes [off1[i], off1[i+1]) of seq1, R2 bytes [off2[i], off2[i+1]) of seq2. */
typedef struct cm_reads {
    uint64_t n_pairs;
    const uint8_t *seq1;
    const uint64_t *off1;   /* n_pairs+1 */
    const uint8_t *seq2;
    const uint64_t *off2;   /* n_pairs+1 */
} cm_reads;

/* ---------------- context ---------------- */
int cm_create(const cm_params *p, cm_ctx **out);
void cm_destroy(cm_ctx *ctx);
const char *cm_last_error(const cm_ctx *ctx);      /* never NULL */

/* Stage one packed contig (index + decoded genome) into HBM.  Replaces loadHashTable +
 * pac2char_whole_contig (src/circminer.cpp:232,244).  slot is the caller's handle (0..15). */
int cm_load_contig(cm_ctx *ctx, int slot, const cm_index_view *iv);
/* Stage the flattened annotation of the same contig.  Replaces gtf_parser.load_gtf's
 * query-side state for contigNum (src/circminer.cpp:205-206). */
struct cm_index_raw;
/* cm_load_contig from a record as cm_host_next_contig_raw leaves it: the table goes over PCIe as it is in the file and is
 * flattened into the cm_index_view layout BY THE DEVICE (bucket offsets by two scans, entries scattered at HBM bandwidth)
 * instead of by host threads (loadHashTable's pointer table + arena, src/mrsfast/HashTable.c:1013-1034, never exists).  The
 * resident contig is the same as after cm_host_next_contig + cm_load_contig.  A malformed table (a header slot that claims
 * more entries than its bucket has slots) is CM_EINVAL. */
int cm_load_contig_raw(cm_ctx *ctx, int slot, const struct cm_index_raw *raw);
int cm_load_annotation(cm_ctx *ctx, int slot, const cm_annot_view *av);
/* cm_load_contig with the k-mer table BUILT BY THE DEVICE from the sequence alone: no host builder, no index file.  `genome`
 * is ref_len host bytes in the convention of cm_index_view.genome and is not normalised: a k-mer is indexed iff all k bases
 * are upper-case A/C/G/T (k = the context's params.kmer).  A counting sort on the device -- count per 14-mer bucket, scan,
 * scatter, then every bucket ordered by (checksum, position): few-entry buckets by one lane each, medium ones by a workgroup
 * in LDS, anything larger (homopolymers, satellite families) through a listed radix-sort path, so no bucket size is a limit.
 * The resident contig is the same as after cm_host_build_index + cm_load_contig.  CM_ENOMEM leaves the slot unloaded. */
typedef struct cm_build_stats {
    uint64_t n_entries;          /* indexed k-mer positions */
    uint32_t max_bucket;         /* entries of the fullest 14-mer bucket */
    uint32_t reserved;           /* (diagnostic: temporary device memory the build took besides the resident arrays, MiB) */
    uint64_t buckets_by_path[3]; /* non-empty buckets ordered by: lane / workgroup (LDS) / oversize path */
    double ms_device;            /* HIP-event time of the build, sequence upload and descriptors excluded */
} cm_build_stats;
int cm_build_contig(cm_ctx *ctx, int slot, int32_t contig_num, const uint8_t *genome, uint32_t ref_len,
                    cm_build_stats *stats /* nullable */);
/* The resident index arrays of a loaded slot (any of the three loaders) copied to the caller's buffers: bucket_off holds
 * 4^14 + 1 words, checksum / pos cap_entries items.  A NULL pointer skips that array (all three NULL: only *n_entries);
 * CM_ELIMIT when cap_entries is smaller than the slot's entry count. */
int cm_index_download(cm_ctx *ctx, int slot, uint32_t *bucket_off, uint16_t *checksum, uint32_t *pos,
                      uint64_t cap_entries, uint64_t *n_entries);
int cm_unload_contig(cm_ctx *ctx, int slot);

/* Upload a batch of read pairs once; they stay resident for all rounds.
 * prior may be NULL (= first round, fill_map_info's "cnt != 23" state). */
int cm_reads_upload(cm_ctx *ctx, const cm_reads *reads, const cm_mapped_read *prior);

/* Double buffering (the reference overlaps nothing: map_reads parses a block, maps it, prints it, src/circminer.cpp:354-400):
 * cm_reads_stage copies the NEXT batch into a second set of read buffers on a copy stream and returns at once when the host
 * arrays are page-locked (cm_host_alloc; pageable memory is accepted and copied synchronously by the runtime); the rounds of
 * the resident batch run meanwhile.  cm_reads_swap makes the staged batch the resident one (first-round state, or `prior`):
 * it is ordered on the device behind the staged copies and behind the work already queued for the old batch, so the host
 * does not wait.  The host arrays passed to cm_reads_stage must stay untouched until cm_reads_swap has been followed by a
 * cm_sync / download / collect, or until the next cm_reads_stage returns. */
int cm_reads_stage(cm_ctx *ctx, const cm_reads *reads, const cm_mapped_read *prior);
int cm_reads_swap(cm_ctx *ctx);

/* cm_reads_stage for FASTQ TEXT: the tokeniser runs on the device.  text1 / text2 are blocks of the two files of a pair as they
 * are on disk (page-locked -- cm_host_alloc / cm_host_register -- or pageable), both starting at a record.  They go over PCIe as
 * they are and kernels on the staging stream find the lines, check every record, build off1 / off2 and copy the bases into the
 * staged read buffers; afterwards cm_reads_swap, cm_map_rounds and the cross-batch prefetch behave exactly as after
 * cm_reads_stage(reads, NULL).  The semantics are those of cm_fastq_next on files holding the same bytes:
 *   - lines end at '\n' only ('\r' is an ordinary byte); record i is lines 4 i .. 4 i + 3, records are counted by line;
 *     a_X = lines of file X / 4, n = min(a_1, a_2, max_pairs) pairs are staged; n = 0 is CM_OK with nothing staged (the caller
 *     supplies more bytes).  What follows record n - 1 (whole records, a record cut by the end of the block) is not looked at and
 *     not consumed: used1 / used2 are the byte offsets of the first record not staged;
 *   - flags bit 0 / bit 1: text1 / text2 ends at the end of its input.  Then bytes behind the last '\n' are a last line, lines
 *     behind the last whole record are CM_EINVAL when the batch is not full without them (a_X < max_pairs), and so is an R2
 *     that ends before R1 (bit 1 with a_2 < min(a_1, max_pairs)).  Surplus R2 records at the end of the input are ignored and,
 *     unlike in cm_fastq_next, NOT validated;
 *   - CM_EINVAL, with the file and the record's index in the block in cm_last_error, for a record in [0, n) whose header line is
 *     empty or does not start with '@', whose third line is empty or does not start with '+', or whose quality line is not as
 *     long as its sequence line (an empty sequence with an empty quality line is legal, and so is a quality line that starts
 *     with '@'); for an R1 header of exactly 23 tokens (runs of bytes other than ' ': a carried MatchedRead needs the host
 *     parser, take cm_fastq_next; R2's tokens are not looked at); for a read longer than max_read_len.  CM_ELIMIT for more than
 *     CM_MAX_SEEDS_PER_READ seeds in the longest read, and for a block of more than 2^32 - 1 bytes (2^32 - 2 when its last line
 *     has no '\n'); a block that size cannot hold 2^30 pairs, the limit of a batch.
 * On any error nothing is staged; an earlier staged batch is dropped in every case, as in cm_reads_stage.  The call waits for the
 * staging stream only (one small read-back of the batch's shape and verdicts, and the record starts when asked for), never for
 * the mapping streams.  rec1 / rec2 (nullable; max_pairs + 1 words each, n + 1 are written): byte offset of each staged record's
 * '@' in its block, rec[n] = used: what cm_write_remain_text slices names and qualities from.
 *   - flags bit 2 (value 4, "keep names"): the stage also leaves on the device the R1 name of each of the n staged pairs, as
 *     cm_fastq_next would put it into names1: token 0 of the header line (tokens are runs of bytes other than ' ' behind the
 *     '@') without a trailing "/x", up to its first NUL byte; empty for a header without a token.  The names belong to the batch:
 *     they travel with its read buffers through cm_reads_swap and stay valid while the batch is resident, also while the next
 *     cm_reads_stage_text overwrites the text.  cm_format_pam, cm_format_sam and cm_format_remain are their readers.  R2 names: bit 4.
 *     Without the bit the kernels launched, the buffers and the results are those of a stage without names.
 *   - flags bit 3 (value 8, "keep qualities"): the stage also leaves on the device the quality line of every staged record of both
 *     files, in the layout of the bases: quality of read i = qual[off[i] .. off[i + 1]), sharing off1 / off2 (the stage has checked
 *     that the lines are as long).  The qualities belong to the batch exactly as the names do: they travel with its read buffers
 *     through cm_reads_swap and the cross-batch prefetch and outlive the text.  cm_format_sam is their reader (cm_quals_peek, a
 *     test hook, copies them back).  HBM: the bytes of the bases once more, in each of the two buffer sets, allocated only when
 *     the bit is given.  Bits 2 and 3 are independent; without bit 3 the kernels launched, the buffers and the results are those
 *     of a stage without it.
 *   - flags bit 4 (value 16, "keep R2 names"): the stage also leaves on the device the R2 name of each staged pair, by the rule of
 *     bit 2 applied to file 2's header lines, in arrays of their own.  They belong to the batch exactly as the R1 names do (through
 *     cm_reads_swap and the cross-batch prefetch, outliving the text).  cm_format_remain, which needs bits 2, 3 and 4, is their
 *     reader.  HBM: the bytes of the names and a word per pair, in each of the two buffer sets, allocated only when the bit is
 *     given.  Bit 4 is independent of bits 2 and 3; without it the kernels launched, the buffers and the results are those of a
 *     stage without it. */
typedef struct cm_text_batch {
    uint64_t n_pairs;        /* pairs staged */
    uint64_t used1, used2;   /* bytes of text1 / text2 consumed = start of the first record not staged */
    int32_t  max_len;        /* longest read of the batch */
    int32_t  reserved;       /* (diagnostic: after cm_prof_enable(ctx, 1) the tokeniser kernels' time in microseconds, HIP events, copies excluded) */
} cm_text_batch;
int cm_reads_stage_text(cm_ctx *ctx, const uint8_t *text1, uint64_t len1, const uint8_t *text2, uint64_t len2,
                        uint64_t max_pairs, uint32_t flags, uint64_t *rec1, uint64_t *rec2, cm_text_batch *out);

/* One mapping round of the resident batch against contig `slot`:
 * FilterRead::process_read for every pair still active + the skip rule of
 * map_reads (src/circminer.cpp:386-397).  Pairs whose carried state says they were
 * retired in an earlier round (active[i]==0) are left untouched.
 * Asynchronous on the ctx stream; cm_sync() or cm_reads_download() waits. */
int cm_map_round(cm_ctx *ctx, int slot, int is_last_round);

/* Several rounds of the resident batch in one call: rounds slots[0 .. n_rounds) in that order, the last one with
 * is_last_round = last_is_final -- the rounds loop of mapping() (src/circminer.cpp:229-308) for contigs that are all resident.
 * Results are those of n_rounds cm_map_round calls.  What differs is the schedule: seeds and chains of a round depend on the
 * reads and the contig only (the carried MatchedRead enters in the pair stage), so round r + 1 is seeded and chained on the
 * main streams while the pair stage of round r still runs on a second pair of streams; chain buffers and active flags are
 * double-buffered.  Asynchronous like cm_map_round.  A batch of more than 2^20 pairs is mapped in tiles (two of up to 2^21 pairs,
 * more for batches beyond 2^22; ~46 KB of HBM workspace per pair of a tile), walked round by round
 * (every tile through round r, then every tile through round r + 1), so a tile's seeding sees the flags its previous pair stage
 * wrote and only pairs still active are seeded and chained.
 * Across batches: when last_is_final is set and a batch is staged (cm_reads_stage) that fits the workspace of the resident
 * one, its first tile's first round against slots[0] is seeded and chained under this batch's last pair stage; after cm_reads_swap the next
 * cm_map_rounds takes that work over if its slots[0] is the same slot, still holding the same contig and annotation
 * (otherwise it is discarded and redone: results never depend on it). */
int cm_map_rounds(cm_ctx *ctx, const int *slots, int n_rounds, int last_is_final);

/* Copy back the carried state, the per-pair return value of process_read in the last
 * cm_map_round (state[i], -1 if the pair was inactive) and the active flags after it. */
int cm_reads_download(cm_ctx *ctx, cm_mapped_read *out_state, int32_t *out_category, uint8_t *out_active);

/* Convenience wrapper = upload + one round + download (the literal batched process_read). */
int cm_map_batch(cm_ctx *ctx, int slot, int is_last_round, const cm_reads *reads,
                 const cm_mapped_read *prior, cm_mapped_read *out_state, int32_t *out_category);

/* Waits for everything the context has in flight -- the mapping streams and the staging copy of cm_reads_stage -- and reports
 * device-side capacity flags (CM_ELIMIT).  After it returns no host array handed to an earlier call is read any more. */
int cm_sync(cm_ctx *ctx);

/* Put the resident batch back into its first-round state (fill_map_info's "cnt != 23" state,
 * every pair active) without touching the read bytes: lets a caller re-run all rounds on reads
 * that are already in HBM. */
int cm_reads_reset(cm_ctx *ctx);

/* Compact the pairs that are still active into host buffers: after the last round these are the
 * CHIBSJ / CHI2BSJ pairs that write_read_category hands to stage 2 (src/circminer.cpp:395-397);
 * after an earlier round, the pairs re-queued for the next contig.  Ascending pair index.
 * Returns CM_ELIMIT (and the needed count in *out_n) if cap is too small. */
int cm_collect_active(cm_ctx *ctx, uint64_t cap, uint64_t *out_idx, cm_mapped_read *out_state, uint64_t *out_n);
/* The same pairs as self-contained records (global pair index = index_base + index in the batch, then the state):
 * what a rank hands to the BSJ gather, assembled on the device so the host does no packing. */
typedef struct cm_record {
    uint64_t pair;
    cm_mapped_read state;
} cm_record;
int cm_collect_records(cm_ctx *ctx, uint64_t index_base, uint64_t cap, cm_record *out, uint64_t *out_n);
/* Same records, left in device memory the caller owns (`d_out`: cap * sizeof(cm_record) bytes on ctx's device; complete
 * when the call returns): the multi-GPU hand-off gathers them to rank 0 over RCCL straight from HBM
 * (circminer_amd/dist.py) and only rank 0 copies anything to the host. */
int cm_collect_records_device(cm_ctx *ctx, uint64_t index_base, uint64_t cap, void *d_out, uint64_t *out_n);

/* Page-locked host memory for the buffers that cross PCIe (read batches, downloaded states, collected
 * records): the copies in cm_reads_upload / cm_reads_download / cm_collect_active are direct DMA for such
 * buffers instead of staged pageable copies.  Optional: every entry point also accepts ordinary memory. */
int cm_host_alloc(cm_ctx *ctx, uint64_t bytes, void **out);
/* The same for memory the caller already owns (e.g. the batch arrays cm_fastq_next returns): page-locks [p, p + bytes) until
 * cm_host_unregister(p); the range must stay allocated meanwhile. */
int cm_host_register(cm_ctx *ctx, void *p, uint64_t bytes);
int cm_host_unregister(cm_ctx *ctx, void *p);
/* MatchedRead::type histogram of the resident batch (CM_CONCRD .. CM_NOPROC_NOMATCH), counted on the device. */
int cm_type_histogram(cm_ctx *ctx, uint64_t out[14]);
int cm_host_free(cm_ctx *ctx, void *p);

/* ---------------- finer-grained entry points used by the parity tests ---------------- */
/* Seeds (GenomeSeeder::split_match_hash, src/match_read.cpp:270-286) of the resident batch:
 * for probe q = ((pair*2 + mate)*2 + orient)*n_slots + s (orient 0 = forward, 1 = reverse
 * complement; s = seed ordinal, qpos = s*kmer):
 *   out_start[q] = index of first hit in the contig's entry arrays (valid if cnt>0 or high)
 *   out_cnt[q]   = frag_count after the seedLim rule (0 if > seedLim)
 *   out_raw[q]   = occurrence count before the rule (0 = frags==NULL)
 * n_slots = max over the batch of floor(len/kmer); returned through out_n_slots. */
int cm_seed_batch(cm_ctx *ctx, int slot, uint32_t *out_start, uint32_t *out_cnt, uint32_t *out_raw,
                  uint32_t cap_probes, uint32_t *out_n_slots);
/* Chains (chain_seeds_sorted_kbest, src/chain.cpp:73-301) of the resident batch: problem
 * r = (pair*2 + mate)*2 + orient; out_nchain[r] chains stored at out_chains[r*CM_BESTCHAINLIM ...],
 * out_high[r] = high_hits of get_best_chains (src/filter.cpp:478-481). */
int cm_chain_batch(cm_ctx *ctx, int slot, cm_chain *out_chains, int32_t *out_nchain, int32_t *out_high);
/* The three alignment DPs behind every extension, one request at a time on the device (kernel k_dp_probe, one wave per
 * workgroup).  Needs a context, but no contig, annotation or reads; `P` is the request batch's own parameter set (band, max_ed
 * and max_sc are what the DPs read).  A string is a view into `arena`: character i is arena[off + i * step] (step +1 / -1),
 * complemented when mode == 1, NUL when mode == 2. */
typedef struct cm_dp_req {
    int32_t kind;                      /* 0 one_side_banded, 1 local_alignment_side, 2 local_alignment_sc (cm_core.h) */
    int32_t s_off, s_step, s_mode, n;  /* the first string (for kind 1, 2 the reference window) */
    int32_t t_off, t_step, t_mode, m;  /* the second string (the read residual) */
    int32_t arg;                       /* kind 0: w (0 .. band, m == n + w);  kind 1: rev;  kind 2: unused */
} cm_dp_req;
typedef struct cm_dp_res {
    int32_t ret, sc_len, indel, score; /* the wrapper's return value and outputs (0 where the kind has none) */
    int32_t err;                       /* the request's own device-capacity bits (8: a string longer than str_cap) */
} cm_dp_res;
/* str_cap: characters per staging buffer, a multiple of 8 in 8..1016 (the pair kernels' LDS layout: 2 buffers x 64 lanes).
 * lds_fill: what every word of the workgroup's LDS holds before its first request.  grid: workgroups (0: one per 64 requests).
 * arrangement 0: lane l of workgroup v runs requests 64 v + l, + 64 * grid, ...: the wrapper named by `kind`, as the pair
 * kernels call it (closed forms, capacity check, staging, DP), 64 different requests in flight.
 * arrangement 1 (kind 2 only, P->band == 3): the resumable form of the heavy-pair pipeline's DP kernel: lanes draw requests from
 * a shared cursor when 16 or more are idle, stage, and advance their DPs in bursts of 4.
 * Every view, extended by 64 bytes (the staging loads' pad) on both sides, must lie inside the arena: CM_EINVAL otherwise, and
 * for a request that is none of the above.  Synchronous. */
int cm_dp_batch(cm_ctx *ctx, const cm_params *P, const uint8_t *arena, uint64_t arena_len, const cm_dp_req *req, uint32_t n_req,
                int str_cap, uint32_t lds_fill, int arrangement, uint32_t grid, cm_dp_res *out);
/* The annotation look-ups behind every chain and every pairing decision (cm_core.h), one request per lane on the device (kernel
 * k_annot_probe, one wave per workgroup), against the annotation resident in `slot` -- the records, the bucket table and the
 * pair_reach that cm_load_annotation made, not a second upload.  Needs no reads and no index; CM_ESTATE without an annotation.
 * `P` supplies max_ed and scan_level.  Fields a kind does not name are 0.
 *   kind  call                                                          request                           result
 *   0     iv_find_ind(pos)                                              p0 = pos                          ret, aux = ind
 *   1     overlap_ind(pos)                                              p0 = pos                          ret, aux = ind
 *   2     upper_bound(spos, mlen, rlen)                                 p0, p1, p2                        ret, aux = ol, u0 = max_end
 *   3     upper_bound_lookup(spos, mlen, rlen) (no bit test)            p0, p1, p2                        ret, aux = ol, u0 = max_end
 *   4     check_junction(s1, s2, ol, kmer, read_dist)                   p0, p1, i0, i1, i2                ret, aux = trans_dist
 *   5     chr_row(loc)                                                  p0 = loc                          ret
 *   6     bit_at(near_border_bits, p), bit_at(intronic_bits, p)         p0 = p                            ret, aux
 *   7     same_gene_span(iv, s, e)                                      i0 = iv, p0 = s, p1 = e           ret
 *   8     share_gene(a, b)                                              i0 = a, i1 = b                    ret
 *   9     common_tids(s, r), s or r may be -1                           i0 = s, i1 = r                    ret = ids kept, aux = more,
 *         u0 = size of the whole intersection, u1 = order-sensitive fold of all its ids (both from common_tids_from(skip = 0)),
 *         the kept ids in out_tids[64 * request ...]
 *   10    calc_tlen of sm (epos = p0, matched_len = p1) and lm (spos = p2, matched_len = p3), p0 <= p2, after overlap_to_epos(sm)
 *         and overlap_to_spos(lm), called only if both hit (as concordant_explanation does)   ret, aux = intron_num, u0 = 1 if called
 *   11    pair_code of chains [p0, p1) and [p2, p3) with the intervals of overlap(p0), overlap(p2), saved_type = i0      ret
 * Interval indices lie in [-1, n_iv); kinds 4, 7, 8 take none below 0, except ol (kind 4).  mlen (kinds 2, 3: p1) is not 0.  Any
 * 32-bit position is legal.  A slot whose bucket table has iv_bucket_shift 0 or above 31 is not asked.  CM_EINVAL otherwise.  out_tids: 64 words per request (zero where not written).  Synchronous. */
typedef struct cm_annot_req {
    int32_t kind;
    uint32_t p0, p1, p2, p3;
    int32_t i0, i1, i2;
} cm_annot_req;
typedef struct cm_annot_res {
    int32_t ret, aux;                  /* ret: the call's return value (a uint32_t return as its bit pattern) */
    uint32_t u0, u1;
} cm_annot_res;
int cm_annot_batch(cm_ctx *ctx, int slot, const cm_params *P, const cm_annot_req *req, uint32_t n_req, cm_annot_res *out, uint32_t *out_tids);

/* The resident batch's read bytes and offsets copied back (what cm_reads_upload / cm_reads_swap made resident): off1 / off2 take
 * n_pairs + 1 words, seq1 / seq2 off[n_pairs] bytes (CM_ELIMIT when cap1 / cap2 is smaller).  A NULL pointer skips that array; all
 * four NULL return only *n_pairs. */
int cm_reads_peek(cm_ctx *ctx, uint8_t *seq1, uint64_t cap1, uint64_t *off1, uint8_t *seq2, uint64_t cap2, uint64_t *off2,
                  uint64_t *n_pairs);
/* test hook: the qualities kept by cm_reads_stage_text (flag bit 3) for the resident batch copied back, off1[n] / off2[n] bytes
 * (CM_ELIMIT when cap1 / cap2 is smaller; a NULL pointer skips that array).  CM_ESTATE: no resident batch, or one without them. */
int cm_quals_peek(cm_ctx *ctx, uint8_t *qual1, uint64_t cap1, uint8_t *qual2, uint64_t cap2);
/* test hook, the counterpart of cm_reads_download: overwrite the carried states of the resident batch (n_pairs records), behind
 * everything queued for it.  CM_ESTATE without a resident batch.  Flags and categories are not touched. */
int cm_state_poke(cm_ctx *ctx, const cm_mapped_read *states);
/* test hook for the scripts of tests/diag: the pair kernels' lane times in 100 MHz ticks, recorded for a batch uploaded with
 * CM_LANE_CLK in the environment: n_pairs words, 33 n_pairs in a -DCM_DIAG build of the library (the scripts name the rows);
 * CM_EINVAL when nothing was recorded. */
int cm_debug_lane_clk(cm_ctx *ctx, unsigned long long *out);
/* test hook for the scripts of tests/diag: the 32 raw counter words of which cm_prof_counters returns the first 8; from word 8 on
 * what a diagnostic build (-DCM_CHAIN_DIAG, -DCM_DIAG_CNT) accumulates there.  Word 7 (every build): chaining problems with hits
 * that cm_map_rounds left unchained because the pair's other mate has no hit, since the last cm_prof_reset(). */
int cm_debug_counters(cm_ctx *ctx, unsigned long long *out);

/* ---------------- timing hooks for bench.py (HIP events on the ctx stream) ---------------- */
/* Milliseconds spent in each kernel class since the last cm_prof_reset(), and launch counts:
 * [0]=k_seed [1]=k_chain (light problems) [2]=k_pair (light pairs) [3]=k_scan_* [4]=k_pair_heavy
 * [5]=class / counting-sort kernels [6]=k_chain_heavy [7]=the row formatters: the kernels of cm_format_pam, cm_format_sam and cm_format_remain (no
 * launch count); launches[7] = first
 * rounds taken over from the cross-batch prefetch of cm_map_rounds.  [1] and [2] are timed up to the join with the second
 * stream, on which the heavy kernels [6] / [4] run concurrently. */
int cm_prof_enable(cm_ctx *ctx, int on);
int cm_prof_reset(cm_ctx *ctx);
int cm_prof_get(cm_ctx *ctx, double ms[8], uint64_t launches[8]);
/* Algorithmic byte counters of SURVEY §8(d) accumulated by the kernels since cm_prof_reset():
 * [0]=probes [1]=binary-search touches [2]=hits consumed (cnt<=seedLim) [3]=pair-rounds; [4]=pair-rounds that needed the re-run
 * launch (a device capacity the reference does not have, e.g. more than 8 memoised exon pieces in one extension: mapped again
 * with room for 2048, results identical); [5]=pair-rounds the heavy-pair pipeline handed whole to its fall-back kernel (their
 * mate-pair tasks or unpaired chains did not fit the pipeline's arrays, or CM_HP_ATTEMPTS=1), [6]=those of [5] handed over in
 * the second orientation attempt; [7] reserved (0). */
int cm_prof_counters(cm_ctx *ctx, uint64_t c[8]);

/* ---------------- host-side builders (the k-mer index has a device-side builder too: cm_build_contig) ---- */
/* In-memory equivalent of generateHashTableOnDisk for one contig
 * (src/mrsfast/HashTable.c:257-380,769-839): caller frees with cm_host_free_index. */
int cm_host_build_index(const uint8_t *genome, uint32_t ref_len, int32_t kmer, int32_t contig_num,
                        int n_threads, cm_index_view *out);
void cm_host_free_index(cm_index_view *iv);
/* Hit multiplicity of an index: over all indexed k-mer positions of the contig, how many share their k-mer with at least one
 * other position (out[1]) and with more than seed_lim - 1 others, i.e. a probe of that k-mer returns more than seed_lim hits and
 * the seed is dropped (src/match_read.cpp:231,259-263) (out[2]); out[0] = indexed positions, out[3] = distinct k-mers.  The two
 * fractions out[1] / out[0] and out[2] / out[0] characterise a workload's repeat content. */
int cm_host_index_stats(const cm_index_view *iv, int32_t seed_lim, int n_threads, uint64_t out[4]);

/* GTF -> flattened annotation for every packed contig (GTFParser::load_gtf,
 * src/gene_annotation.cpp:191-399).  chromosome table = rows of .index.info
 * (src/genome.cpp:147-167): name, packed contig id (1-based), start_pos.
 * out must point to n_contigs views; free with cm_host_free_annotation. */
typedef struct cm_chr_info {
    const char *name;
    uint32_t contig_id;   /* 1-based */
    uint32_t start_pos;   /* shift   */
    uint32_t len;
} cm_chr_info;
int cm_host_build_annotation(const char *gtf_path, const cm_chr_info *chrs, uint32_t n_chr,
                             const uint32_t *contig_len, uint32_t n_contigs, int32_t max_read_len,
                             cm_annot_view *out);
void cm_host_free_annotation(cm_annot_view *av, uint32_t n_contigs);
/* get_gene_overlap(pos, use_mask = false): the genes whose span covers contig position pos (n_genes = 0: none) */
int cm_host_gene_overlap(const cm_annot_view *av, uint32_t pos, const uint32_t **genes, uint32_t *n_genes);

/* ---------------- on-disk genome / index formats of stock CircMiner ------ */
/* FASTA -> <ref>.packed.fa + <ref>.packed.fa.index.info (GenomePacker::pack_genome,
 * src/genome.cpp:96-146): chromosomes concatenated with a 50-N spacer while they fit contig_size
 * (DEF_CONTIG_SIZE = CM_CONTIG_SIZE in the reference). */
int cm_host_pack_genome(const char *fasta_path, const char *packed_fa_path, const char *index_info_path,
                        uint32_t contig_size);
/* rows of .index.info (GenomePacker::load_index_info, src/genome.cpp:147-167); names are owned by the
 * array: release with cm_host_free_index_info. */
int cm_host_read_index_info(const char *path, cm_chr_info **out, uint32_t *n);
void cm_host_free_index_info(cm_chr_info *chrs, uint32_t n);
/* packed FASTA -> mrsfast index file: full table (generateHashTableOnDisk, src/mrsfast/HashTable.c:257-380,
 * magic 3) or compact (generateHashTable, :383-474, magic 2: the table is rebuilt at load time). */
int cm_host_write_index(const char *packed_fa_path, const char *index_path, int32_t kmer, int compact,
                        int n_threads);
/* Reader (checkHashTable / initLoadingHashTable / loadHashTable, HashTable.c:485-509, 618-700, 971-1098):
 * open parses the header; every cm_host_next_contig call loads the next packed contig -- genome decoded to
 * ASCII and the table flattened into a cm_index_view ready for cm_load_contig -- and sets *loaded = 0
 * after the last one.  Views are released with cm_host_free_loaded_contig.
 * A packed FASTA (<ref>.packed.fa, first byte '>') is accepted as a table-less source: *is_full = -1, *kmer = 0, and only
 * cm_host_next_contig_genome serves its records (one FASTA record = one contig, contig_num = name - 1, bases upper-cased,
 * anything but A/C/G/T -> N: the bytes the index file written from it holds); cm_host_next_contig and
 * cm_host_next_contig_raw return CM_EINVAL.  Such contigs are made resident with cm_build_contig. */
typedef struct cm_index_file cm_index_file;
int cm_host_open_index(const char *index_path, cm_index_file **out, int32_t *kmer, int32_t *is_full,
                       uint32_t *n_records);
int cm_host_next_contig(cm_index_file *f, int n_threads, cm_index_view *out, int *loaded);
/* The same record with its k-mer table stepped over: only genome / ref_len / contig_num of *out are set (ProcessCirc::load_genome,
 * src/process_circ.cpp:1659-1680: loadCompressedRefGenome, the sequence alone); stage 2 uses this. */
/* The same record left as it is in the file, for cm_load_contig_raw: decoded genome, the (hv, count14) pair of every non-empty
 * bucket in file order, and the table itself (GeneralIndex slots of 8 bytes: per bucket a header slot whose info = number of
 * valid entries, then count14 slots).  Full-format index files only (CM_EINVAL for the compact format: take
 * cm_host_next_contig).  The arrays belong to the file handle and stay valid until the call after next (two sets take turns, so
 * the next record can be read while this one uploads) or cm_host_close_index. */
typedef struct cm_index_raw {
    int32_t contig_num;
    uint32_t ref_len;
    const uint8_t *genome;       /* ref_len bytes                                   */
    uint32_t n_buckets;          /* non-empty 14-mer buckets                        */
    const uint32_t *hv;          /* ascending                                       */
    const uint32_t *count14;     /* slots of bucket i = count14[i] + 1              */
    const void *table;           /* table_slots x 8 bytes, as in the file           */
    uint64_t table_slots;
} cm_index_raw;
int cm_host_next_contig_raw(cm_index_file *f, int n_threads, cm_index_raw *out, int *loaded);
int cm_host_next_contig_genome(cm_index_file *f, cm_index_view *out, int *loaded);
void cm_host_free_loaded_contig(cm_index_view *iv);
void cm_host_close_index(cm_index_file *f);

/* ---------------- FASTQ ingest, carry-over header, PAM / remain writers ---------- */
/* One batch of parsed pairs in the layout cm_reads_upload takes.  All pointers belong to the parser and stay
 * valid over the next THREE cm_fastq_next calls (four generations of storage take turns: batch k-1 can be with a writer
 * thread, batch k on the GPU and batch k+1 staged for it while batch k+2 is parsed) or until cm_fastq_close.  names*: NUL-terminated read names (first header token,
 * trailing "/x" cut: FASTQParser::extract_map_info, src/fastq_parser.cpp:178-198), name i at names + name_off[i].
 * prior: the MatchedRead each pair carried in its 23-token header (fill_map_info, :200-269) or NULL when no
 * pair of the batch carried one (fresh reads: cm_reads_upload's default state). */
typedef struct cm_fastq_batch {
    cm_reads reads;
    const uint8_t *qual1, *qual2;        /* same offsets as reads.seq1 / reads.seq2 */
    const char *names1, *names2;
    const uint64_t *name_off1, *name_off2;
    const cm_mapped_read *prior;
} cm_fastq_batch;
typedef struct cm_fastq cm_fastq;
/* plain or gzip FASTQ (gzread, as src/fastq_parser.cpp:84-98); chrs = rows of .index.info (chromosome
 * names of the carried headers -> chr_id); max_ed = maxEd of the run (state of unmapped carried reads). */
int cm_fastq_open(const char *r1_path, const char *r2_path, const cm_chr_info *chrs, uint32_t n_chr, int32_t max_ed,
                  cm_fastq **out);
/* One rank's contiguous block of pairs of a paired FASTQ ("rank r gets pairs [r*N/W, (r+1)*N/W)"): both files
 * are cut at the same record, found by counting the newlines of the files in blocks on n_threads threads (no parsing).
 * gzip files (the reference reads .gz everywhere, src/fastq_parser.cpp:84-98) cannot be entered in the middle: their records are
 * counted with one inflate pass over R1 and every rank inflates from the start, stepping over the blocks of the ranks before it --
 * the same blocks and output bytes as plain text, at zlib's speed.  A pipe cannot be read twice: CM_EINVAL when world > 1.
 * first_pair / n_pairs (nullable): the block's position in the whole input.  Every rank of a node can open its share at the same time. */
/* The same reader over two texts in memory: cm_fastq_next returns the batches it returns for two files that hold these bytes
 * (reads, qualities, names, `prior`), with the same verdict on malformed text in the same call.  The text stays the caller's and
 * must outlive the reader; it is read record by record, as gzip input is.  cm_fastq_next_text does not serve it (CM_EINVAL).
 * n1 / n2 == 0 with a null text is an empty file. */
int cm_fastq_open_mem(const void *text1, uint64_t n1, const void *text2, uint64_t n2, const cm_chr_info *chrs, uint32_t n_chr,
                      int32_t max_ed, cm_fastq **out);
int cm_fastq_open_shard(const char *r1_path, const char *r2_path, const cm_chr_info *chrs, uint32_t n_chr, int32_t max_ed,
                        int32_t rank, int32_t world, int n_threads, cm_fastq **out, uint64_t *first_pair, uint64_t *n_pairs);
int cm_fastq_next(cm_fastq *f, uint64_t max_pairs, cm_fastq_batch *out);   /* out->reads.n_pairs == 0 at the end; CM_ENOMEM when a batch array cannot grow */
/* A caller that page-locks the arrays of a batch (cm_host_register on reads.seq1/seq2/off1/off2, prior) must know when one of
 * them goes away: `fn(user, ptr, bytes)` is called -- on whichever thread runs cm_fastq_next / cm_fastq_close -- right BEFORE the
 * block starting at `ptr` is freed (a generation's array that has to grow is allocated anew, never moved in place), so that the
 * caller can unregister it first.  No copy out of that block may still be in flight then: the block belongs to the generation
 * handed out four cm_fastq_next calls ago. */
void cm_fastq_set_release_hook(cm_fastq *f, void (*fn)(void *user, const void *ptr, uint64_t bytes), void *user);
/* Raw-block mode, for cm_reads_stage_text: the next block of both files as text, nothing parsed.  A block is what the caller has
 * not consumed of the block before it (cm_fastq_text_consumed; without that call: all of it) followed by fresh bytes, about
 * want_bytes per file in all -- half of want_bytes fresh at least, so a caller whose block held no whole pair gets more by
 * asking again; *eofX: the block ends at the end of the reader's share of file X (cm_fastq_open_shard's byte range is respected).
 * Regular plain-text files only: CM_EINVAL for gzip input and pipes (which stay on cm_fastq_next), and on a reader that
 * cm_fastq_next has read from.  Four generations of blocks take turns: a block stays valid over the next three calls.  The tail
 * is copied into head room in front of the fresh bytes; the blocks are malloc'ed, the release hook announces one that goes. */
int cm_fastq_next_text(cm_fastq *f, uint64_t want_bytes, const uint8_t **text1, uint64_t *len1, int *eof1,
                       const uint8_t **text2, uint64_t *len2, int *eof2);
int cm_fastq_text_consumed(cm_fastq *f, uint64_t used1, uint64_t used2);
void cm_fastq_close(cm_fastq *f);

/* Writers.  cm_write_remain = FilterRead::write_read_category PE (src/filter.cpp:413-455) into
 * <out>_<round>_remain_R1.fastq / _R2.fastq; cm_write_pam = SAMOutput::write_pam_rec_pe
 * (src/output.cpp:279-299) into <out>.mapping.pam (path2 = NULL).  sel = indices of the pairs to write
 * (NULL: all): map_reads writes PAM rows for (skip || last round) and remain records for the pairs
 * cm_collect_active returns (src/circminer.cpp:386-397). */
typedef struct cm_writer cm_writer;
int cm_writer_open(const char *path1, const char *path2, const cm_chr_info *chrs, uint32_t n_chr, cm_writer **out);
int cm_write_remain(cm_writer *w, const cm_fastq_batch *b, const cm_mapped_read *states, const uint64_t *sel, uint64_t n_sel);
/* cm_write_remain for (pair index, state) records as cm_collect_records delivers them (index_base 0): only the re-queued
 * pairs' states have to leave the device. */
int cm_write_remain_records(cm_writer *w, const cm_fastq_batch *batch, const cm_record *recs, uint64_t n);
/* The bytes of cm_write_remain_records for a batch that went through cm_reads_stage_text: name (first header token, trailing
 * "/x" cut), bases and quality of pair recs[k].pair are sliced from the blocks' text at rec1 / rec2, the record starts that call
 * returned. */
int cm_write_remain_text(cm_writer *w, const uint8_t *text1, const uint64_t *rec1, const uint8_t *text2, const uint64_t *rec2,
                         const cm_record *recs, uint64_t n_rec);
int cm_write_pam(cm_writer *w, const cm_fastq_batch *b, const cm_mapped_read *states, const uint64_t *sel, uint64_t n_sel);
/* <out>.mapping.pam rows (cm_write_pam / SAMOutput::write_pam_rec_pe, src/output.cpp:279-299) of pairs [first, first + count)
 * of the resident batch, formatted BY THE DEVICE from the states in HBM and the names kept by cm_reads_stage_text (flag bit 2):
 * the bytes cm_write_pam writes for the same pairs, in pair order -- "%u" / "%d" as there (mlen_* through (int), junc_num a
 * uint16, gm_compatible as != 0), the unmapped form (21 "*" fields and the type) for every type outside CONCRD, DISCRD, CHIORF,
 * CHIBSJ, CHI2BSJ, CONGNM, CONGEN (negative or > 13 included), "-" for a chr_id outside [0, n_chr).  chrs: the chromosome table
 * (names only are used); it is uploaded when it differs from the one last given to this context.
 * Ordering is that of cm_collect_records: the work is queued behind everything queued for the resident batch (pair stages, the
 * re-run launch, fall-backs) and the call returns when the bytes are in out (page-locked or pageable, cap bytes); it neither
 * waits for nor disturbs the staging stream or a cross-batch prefetch in flight.
 * CM_ESTATE: no resident batch, or one without names (cm_reads_upload, cm_reads_stage, cm_reads_stage_text without bit 2).
 * CM_EINVAL: first + count > n_pairs, or out == NULL with cap > 0.  CM_ELIMIT with the needed size in *out_bytes and nothing
 * written: cap is too small; CM_ELIMIT also when the rows of one call come to 2^32 bytes or more (offsets are 32 bits: format in
 * ranges).  count == 0 is CM_OK with *out_bytes == 0.  A refusal leaves the resident batch as it was.
 * stats (nullable): [0] rows, [1] bytes, [2] / [3] spans of 64 rows (one wave each) that were formatted in the wave's LDS window
 * and streamed out as whole words / that were larger than the window (long names) and stored byte by byte by their lanes.
 * After cm_prof_enable(ctx, 1) the formatter's kernels are timed by HIP events into ms[7] of cm_prof_get. */
int cm_format_pam(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count,
                  void *out, uint64_t cap, uint64_t *out_bytes, uint64_t stats[4] /* nullable */);
/* <out>.mapping.sam records (cm_write_sam / write_sam_rec_pe) of pairs [first, first + count) of the resident batch, formatted BY
 * THE DEVICE from the states in HBM, the names (flag bit 2) and qualities (flag bit 3) kept by cm_reads_stage_text and the bases in
 * the read buffers: the bytes cm_write_sam writes for the same pairs, in pair order, two records per pair (mate 1, then mate 2;
 * QNAME is the R1 name in both) -- a pair is mapped for type <= CM_CHIORF || type == CM_CONGEN || type == CM_CONGNM (signed),
 * TLEN is "%u" of the int32 with the sign by spos_r1 < spos_r2, a record with the reverse flag prints the reverse complement cut at
 * the first byte outside ACGTNacgtn and the reversed qualities, "-" for a chr_id outside [0, n_chr).  One value differs in
 * principle: for tlen == INT_MIN the host's negation is signed overflow; the device negates in unsigned arithmetic and prints
 * 2147483648 for both mates.  The header is not formatted here: cm_write_sam_header.  chrs: as for cm_format_pam (one table per
 * context, shared by both formatters).
 * Ordering is that of cm_collect_records: the work is queued behind everything queued for the resident batch (pair stages, the
 * re-run launch, fall-backs) and the call returns when the bytes are in out (page-locked or pageable, cap bytes); it neither
 * waits for nor disturbs the staging stream or a cross-batch prefetch in flight.
 * CM_ESTATE: no resident batch, or one staged without bit 2 or without bit 3 (cm_last_error names which).
 * CM_EINVAL: first + count > n_pairs, or out == NULL with cap > 0.  CM_ELIMIT with the needed size in *out_bytes and nothing
 * written: cap is too small; CM_ELIMIT also when the records of one call come to 2^32 bytes or more (offsets are 32 bits: format
 * in ranges).  count == 0 is CM_OK with *out_bytes == 0.  A refusal leaves the resident batch as it was.
 * stats (nullable): [0] records (2 count), [1] bytes, [2] / [3] spans of 16 records (one wave each) that were put together in the
 * wave's LDS window and streamed out as whole words / that were larger than the window (long names, long reads) and stored to the
 * output directly.  After cm_prof_enable(ctx, 1) the formatter's kernels are timed by HIP events into ms[7] of cm_prof_get. */
int cm_format_sam(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count,
                  void *out, uint64_t cap, uint64_t *out_bytes, uint64_t stats[4] /* nullable */);
/* <out>_<R>_remain_R1.fastq / _R2.fastq records (cm_write_remain_records / write_read_category, src/filter.cpp:413-455) of
 * records [first, first + count) of the resident batch's ACTIVE SET -- the pairs cm_collect_records delivers, in ascending pair
 * index --, formatted BY THE DEVICE from the states in HBM, the R1 names (flag bit 2), the qualities (bit 3) and the R2 names
 * (bit 4) kept by cm_reads_stage_text and the bases in the read buffers: into out1 the bytes cm_write_remain_records writes to the
 * first file for the same records, into out2 those of the second.  A record is '@', the mate's name, the header fields (the same
 * in both files), '\n', the bases, "\n+\n", the qualities, '\n'.  The fields of a type among CONCRD, DISCRD, CHIORF, CHIBSJ,
 * CHI2BSJ, CONGNM, CONGEN: " %lld %d %s %u %u %d %u %u %c %d %s %u %u %d %u %u %c %d %d %d %d %d" with
 * gspos = (uint64)(int64)contig_num * CM_CONTIG_SIZE + (uint32)(spos_r1 + shift) printed signed, shift = start_pos of chr_id inside
 * [0, n_chr) and 0 outside (where the chromosome prints "-"), mlen_* through (int), junc_num a uint16, gm_compatible as != 0; of
 * every other type " * <type>" and 20 times " *".  The names end at their first NUL byte, as those of a host-parsed batch do
 * (cm_write_remain_text does not cut there: the one input on which the two writers of the device tokeniser's path differ).
 * count == ~0ull: to the end of the set.  chrs: names and start_pos are used (one table per context, shared with cm_format_pam and
 * cm_format_sam).  n_records (nullable) receives the size of the active set: also for count == 0 and on every refusal for which a
 * resident batch exists.  out_keys (nullable, count words): out_keys[k] is what `sort -k2,2n` orders record first + k by (key_of
 * in stage 2): gspos for a type that prints its fields, 0 for the star form -- the value, not a parse: for a name that holds a
 * blank the text's second field is something else.
 * Ordering is that of cm_collect_records: the work is queued behind everything queued for the resident batch and the call returns
 * when the bytes are in out1 / out2 (page-locked or pageable); it neither waits for nor disturbs the staging stream or a
 * cross-batch prefetch in flight.
 * CM_ESTATE: no resident batch, or one staged without bit 2, 3 or 4 (cm_last_error names which).  CM_EINVAL: first + count beyond
 * the set, or out1 / out2 == NULL with a cap > 0.  CM_ELIMIT with the needed sizes in out_bytes[0] / [1] and nothing written:
 * either cap is too small; CM_ELIMIT also when a file's records of one call come to 2^32 bytes or more (format in ranges).
 * count == 0 is CM_OK with out_bytes == {0, 0}.  A refusal leaves the resident batch as it was.
 * stats (nullable): [0] records of both files (2 count), [1] bytes of both, [2] / [3] spans of 16 records (one wave each, both
 * files) that were put together in the wave's LDS window and streamed out as whole words / that were larger than the window (long
 * names, reads of 250 - 300 bases) and stored to the output directly.  After cm_prof_enable(ctx, 1) the formatter's kernels are
 * timed by HIP events into ms[7] of cm_prof_get. */
int cm_format_remain(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count,
                     void *out1, uint64_t cap1, void *out2, uint64_t cap2, uint64_t out_bytes[2], int64_t *out_keys,
                     uint64_t *n_records, uint64_t stats[4] /* out_keys, n_records, stats: nullable */);
/* cm_format_remain with the records in the order cm_sort_remain gives the files it writes: records [first, first + count) of the
 * active set ordered by key (out_keys' value, ascending, signed) and, among equal keys, per file by the bytes of the record as
 * `paste - - - -` joins it (the first three line feeds read as TAB, the last left out; unsigned bytes, a proper prefix first;
 * identical lines in the order of the active set).  Inside a group of equal keys file 1 and file 2 may therefore hold the pairs in
 * different orders, as two separately sorted files do; a range that cuts such a group holds each file's own members of it.  The
 * key's VALUE orders, where cm_sort_remain parses the text's second field: for a name that holds a TAB the two differ (see
 * out_keys above), and such names are outside this call's promise.
 * Everything else is cm_format_remain's contract -- arguments, refusals, count == ~0ull, n_records, the stream, "a refusal leaves
 * the resident batch as it was" -- with these additions: out_keys is non-decreasing and serves both files; out_off1 / out_off2
 * (nullable, count + 1 words each) receive the byte offset of every record in out1 / out2 and the files' sizes in their last word;
 * CM_ELIMIT with nothing written and out_bytes == {0, 0} when more than 4096 records share a key (the ranking inside a group is
 * quadratic; cm_last_error names the group's size and the cap; CM_REMAIN_TIE_CAP=<n> in the environment, a test knob read by every
 * call, lowers the cap): the caller orders such a batch on the host.  The set is sorted again by every call, so a caller that
 * formats in ranges (32-bit offsets) pays the sort per range.  ms[7] of cm_prof_get covers the sort's kernels too. */
int cm_format_remain_sorted(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count,
                            void *out1, uint64_t cap1, void *out2, uint64_t cap2, uint64_t out_bytes[2], int64_t *out_keys,
                            uint32_t *out_off1, uint32_t *out_off2, uint64_t *n_records,
                            uint64_t stats[4] /* out_keys, out_off1, out_off2, n_records, stats: nullable */);
/* Appends n raw bytes to the writer's first file through its buffer (the rows cm_format_pam / cm_format_sam deliver, the first
 * file's records of cm_format_remain); CM_EIO like the other cm_write_* calls. */
int cm_write_bytes(cm_writer *w, const void *p, uint64_t n);
/* ... to the writer's second file; CM_EINVAL for a writer opened without one. */
int cm_write_bytes2(cm_writer *w, const void *p, uint64_t n);
/* <out>.mapping.sam (--sam): header = SAMOutput::print_header (src/output.cpp:301-311, one @SQ per row of the chromosome
 * table), records = write_sam_rec_pe with set_flag_pe / set_output_pe (src/output.cpp:118-277): two lines per pair,
 * CIGAR "*", MAPQ 255, tags AT / NM / JC / TC; TLEN is printed with %u like the reference does. */
int cm_write_sam_header(cm_writer *w);
int cm_write_sam(cm_writer *w, const cm_fastq_batch *b, const cm_mapped_read *states, const uint64_t *sel, uint64_t n_sel);
/* Pushes buffered rows to the file(s); CM_EIO if any write since the writer was opened came up short (the cm_write_* calls
 * report the same as soon as they notice).  cm_writer_close flushes too but cannot report. */
int cm_writer_flush(cm_writer *w);
void cm_writer_close(cm_writer *w);

/* ---------------- stage 1 end to end: the caller of the hot path ---------------- */
/* mapping() + map_reads() of the reference (src/circminer.cpp:98-352, :354-400) over the entry points above: reads
 * <ref>.packed.fa.index(.info) and the GTF, keeps every packed contig resident, takes the paired FASTQ through all
 * rounds batch by batch, and writes what the reference leaves behind for the user and for stage 2:
 *   <out>.mapping.pam (report 1) or <out>.mapping.sam (report 2): the rows map_reads prints (skip || last round);
 *   <out>_<R>_remain_R1.fastq / _R2.fastq, R = number of packed contigs: the CHIBSJ / CHI2BSJ pairs (:395-397).
 * The per-round remain files of the reference (its way of carrying pairs from one contig to the next) are not
 * written: the carried state stays in HBM.  params.kmer == 0 takes the index file's k.
 * index_path may name the packed FASTA itself (no index file on disk): every contig's table is built on the device
 * (cm_build_contig) while the next contig's sequence is read; params.kmer must be given then (0 is CM_EINVAL).
 * With CM_FASTQ_DEVICE=1 in the environment, report == 0 and two regular plain-text FASTQ files of fresh reads (any rank / world)
 * the batches are tokenised on the device: cm_fastq_next_text -> cm_reads_stage_text -> cm_write_remain_text, the same files
 * byte for byte; in every other case (PAM / SAM rows without their own variable, below, need every pair's name on the host; gzip,
 * pipes and carried 23-token headers need the host parser) and with the variable unset the host parser feeds the device as before.  CM_FASTQ_DEVICE_BLOCK=<bytes>
 * (a test knob) sets the bytes per file and block; the default is sized for batch_pairs.
 * With CM_PAM_DEVICE=1 in addition to CM_FASTQ_DEVICE=1 the device tokeniser's path also covers report == 1 (same conditions on
 * the input): the batches are staged with their names (flag bit 2), the PAM rows of a batch are formatted on the device
 * (cm_format_pam, into one of two page-locked buffers) and the writer thread appends them with cm_write_bytes -- the same
 * <out>.mapping.pam byte for byte.
 * With CM_SAM_DEVICE=1 in addition to CM_FASTQ_DEVICE=1 the path covers report == 2 in the same way: the batches are staged with
 * their names and qualities (flag bits 2 | 3), the SAM records of a batch are formatted on the device (cm_format_sam, in ranges of
 * at most 2^17 pairs, into one of two page-locked buffers that hold a batch's records) and the writer thread appends them behind
 * the header -- the same <out>.mapping.sam byte for byte.  Without its variable a report mode stays with the host parser.
 * With CM_REMAIN_DEVICE=1 in addition to CM_FASTQ_DEVICE=1 the remain records of the path are formatted on the device too, in every
 * report mode the path covers: the batches are staged with flag bits 2 | 3 | 4 on top of what the report mode asks for, after a
 * batch's last round cm_format_remain puts the records of the pairs still active into two of four page-locked buffers (two sets of
 * two) and the writer thread appends them with cm_write_bytes / cm_write_bytes2 in place of cm_write_remain_text -- the same remain
 * files byte for byte (names with a NUL byte excepted, see cm_format_remain), the same statistics, for one process and for rank /
 * world part files.  Where the host parser's path is taken the variable has no effect.
 * With CM_REMAIN_SORTED=1 beside CM_FASTQ_DEVICE=1 CM_REMAIN_DEVICE=1 and world <= 1 the run also leaves
 * <out>_<R>_remain_R{1,2}.fastq.srt, the files cm_sort_remain makes of the remain files (which are written exactly as without the
 * variable): every batch's active set goes through cm_format_remain_sorted into page-locked buffers and into a cm_remain_runs, a
 * batch the device refuses for a tie group is ordered on the host from its unsorted records (cm_remain_runs_add_unsorted), and
 * cm_remain_runs_finish writes both files after the last batch.  CM_REMAIN_TRACE=1 prints one line to stderr: batches, batches
 * ordered on the host, records, seconds of the merge.  With world > 1, or off the device tokeniser's path, the variable has no
 * effect. */
typedef struct cm_mapping_args {
    const char *index_path;        /* <ref>.packed.fa.index        */
    const char *index_info_path;   /* <ref>.packed.fa.index.info   */
    const char *gtf_path;
    const char *fastq1, *fastq2;   /* plain or gzip                */
    const char *out_prefix;        /* outputFilename               */
    cm_params params;
    int32_t report;                /* reportMapping: 0 none, 1 PAM, 2 SAM */
    int32_t n_threads;             /* host threads for the index loader   */
    uint64_t batch_pairs;          /* pairs per resident batch, 0 = 2^18  */
    /* One process per GPU: rank `rank` of `world` maps the rank-th contiguous block of pairs
     * (cm_fastq_open_shard) on device params.device and writes <file>.part<rank> instead of <file> for every output;
     * cm_merge_parts on rank 0 then makes the files of an unsharded run (same bytes: blocks are contiguous, rows are in
     * input order).  world 0 or 1: one process, final file names. */
    int32_t rank, world;
} cm_mapping_args;
typedef struct cm_mapping_stats {
    uint64_t pairs, bsj_pairs;
    uint64_t by_type[14];          /* final MatchedRead::type histogram (CM_CONCRD ... ) */
    int32_t rounds;
    int32_t device_parsed_batches; /* batches tokenised on the device (CM_FASTQ_DEVICE=1, see cm_mapping_run); 0 on the host parser's path */
    double seconds_load, seconds_map;
    /* where seconds_map went, summed over the batches (the three overlap, so they add up to more than seconds_map):
     * parsing FASTQ (parser thread), driving the device (stage + rounds + results + swap, calling thread), writing rows
     * (writer thread) */
    double seconds_parse, seconds_device, seconds_write;
} cm_mapping_stats;
int cm_mapping_run(const cm_mapping_args *args, cm_mapping_stats *stats, char *err, uint64_t err_cap);
/* After every rank's cm_mapping_run(rank, world) has returned: <out>_<rounds>_remain_R{1,2}.fastq and the mapping file
 * (report 1 / 2) are concatenated from their .part<r> files in rank order, the parts are removed.  The result is what one
 * process writes for the whole input; cm_circ_run takes it from there (stage 2 runs once, on the host of rank 0). */
int cm_merge_parts(const char *out_prefix, int32_t rounds, int32_t world, int32_t report);

/* ---------------- stage 2: ProcessCirc, src/process_circ.cpp -- host code, no GPU involved -------- */
/* ProcessCirc::sort_fq (src/process_circ.cpp:179-193): the remain FASTQ of the last round ordered like
 * `paste - - - - | sort -k2,2n | tr "\t" "\n"` does in the C locale (key = genome_spos, ties by the whole pasted line). */
int cm_sort_remain(const char *in_path, const char *out_path);
/* The same order made from sorted runs: every run is the records of one cm_format_remain_sorted call (or any records in
 * cm_sort_remain's order with their keys), `finish` merges the runs of file 1 into srt_path1 and, independently, those of file 2
 * into srt_path2 -- by key, then by the pasted line (cm_sort_remain's comparator), then by run number -- so that the two files
 * are what cm_sort_remain makes of the concatenated runs.  bytes1 / bytes2: the records of the run, off1 / off2: n_records + 1
 * byte offsets (the last is the run's size), keys: n_records values serving both files.  `add` copies; n_records == 0 is fine.
 * The runs stay in host memory until `finish` (the remain records of the whole run: about 5 % of the pairs at about 820 bytes a
 * pair); spilling them to disk is not built.  CM_EIO: a file cannot be opened or a write came up short.  `close` frees; it does
 * not write. */
typedef struct cm_remain_runs cm_remain_runs;
int cm_remain_runs_open(const char *srt_path1, const char *srt_path2, cm_remain_runs **out);
int cm_remain_runs_add(cm_remain_runs *r, const void *bytes1, const uint32_t *off1, const void *bytes2, const uint32_t *off2,
                       const int64_t *keys, uint64_t n_records);
int cm_remain_runs_finish(cm_remain_runs *r);
/* The same merge into two buffers in host memory instead of the two files: *bytes1 / *n1 and *bytes2 / *n2 are what `finish`
 * would have written to srt_path1 / srt_path2.  The buffers belong to `r` until `close` (a second call makes them anew).
 * cm_remain_runs_open(NULL, NULL, &r) opens runs without paths for this finish alone; `finish` on them is CM_EINVAL. */
int cm_remain_runs_finish_mem(cm_remain_runs *r, const void **bytes1, uint64_t *n1, const void **bytes2, uint64_t *n2);
void cm_remain_runs_close(cm_remain_runs *r);
/* A run made on the host from UNSORTED records (the fall-back for a batch cm_format_remain_sorted refuses): the two files' bytes
 * as cm_format_remain delivers them are ordered by the in-memory body of cm_sort_remain -- the key parsed from the text -- and
 * added as one run. */
int cm_remain_runs_add_unsorted(cm_remain_runs *r, const void *bytes1, uint64_t n1, const void *bytes2, uint64_t n2);
/* RegionalHashTable::create_table (src/hash_table.cpp:58-78) flattened: the window_size-mers of a gene region, bucket hv =
 * loc[off[hv] .. off[hv+1]) ascending, location = start + offset in seq; buckets above MAXHIT = 1000 are emptied. */
int cm_regional_table_build(const uint8_t *seq, uint32_t start, int32_t len, int32_t window_size, uint32_t **off, uint32_t **loc);
void cm_regional_table_free(uint32_t *off, uint32_t *loc);
/* ProcessCirc::report_events (src/process_circ.cpp:1570-1631): the BSJ calls of stage 2 (CircRes, src/common.h:406-423;
 * type 20 = CR, 21 = NCR, 22 = MCR, src/process_circ.h:16-18) -> <out>.circ_report rows
 * chr, start, end, read count, "STC", consensus start-end signal, reference start-end signal, Pass|Fail, read names. */
typedef struct cm_circ_res {
    const char *chr, *rname;
    uint32_t spos, epos;
    int32_t type, reserved;
    const char *start_signal, *end_signal, *start_bp_ref, *end_bp_ref;
} cm_circ_res;
int cm_circ_report(const cm_circ_res *res, uint64_t n, const char *report_path);
/* The back-splice-junction calling between the two (ProcessCirc::do_process, src/process_circ.cpp:195-331: call_circ_single_split /
 * call_circ_double_split :360-645, chaining of 8-mer seeds inside the overlapping genes :677-737 + src/chain.cpp:310-539,
 * find_exact_coord :739-789, check_split_map :892-1134, final_check :1136-1341, split_realignment :1343-1486,
 * rescue_overlapping_bsj :1488-1552) over records that are already in the order of the sorted remain files: `sorted` is one
 * batch from cm_fastq_next on <out>_<R>_remain_R{1,2}.fastq.srt (its `prior` = the MatchedRead each pair carries in its header).
 * Writes <out>.candidates.pam rows (print_split_mapping :1670-1708 + type) to candidates_path and the <out>.circ_report rows
 * (report_events) to report_path.  window_size 0 = 8 (circ_detect, src/circminer.cpp:347-352).  Pairs are called on all host
 * cores (CM_CIRC_THREADS overrides; cm_circ_run uses its n_threads); the files do not depend on the number of threads. */
typedef struct cm_circ_stats {
    uint64_t pairs, candidate_rows, calls;
    double seconds;
} cm_circ_stats;
int cm_circ_call(const cm_params *p, int32_t window_size, uint32_t n_contigs, const cm_index_view *contigs, const cm_annot_view *annots,
                 const cm_chr_info *chrs, uint32_t n_chr, const cm_fastq_batch *sorted, const char *candidates_path,
                 const char *report_path, cm_circ_stats *stats);
/* circ_detect() of the reference (src/circminer.cpp:347-352) from files to files: sorts <out>_<last_round>_remain_R{1,2}.fastq
 * (-> .srt), loads the packed genome from the index file and the GTF, calls the junctions, writes <out>.candidates.pam and
 * <out>.circ_report.  params.kmer == 0 takes the index file's k.  index_path may be the packed FASTA (stage 2 needs the sequence only).
 * With CM_CIRC_PRESORTED=1 in the environment the two .srt files are taken as they are (cm_mapping_run with CM_REMAIN_SORTED=1
 * leaves them) and cm_sort_remain is not called; a .srt file that cannot be opened is CM_EIO, and err names it. */
typedef struct cm_circ_args {
    const char *index_path, *index_info_path, *gtf_path, *out_prefix;
    cm_params params;
    int32_t last_round;            /* number of packed contigs = suffix of the remain files */
    int32_t window_size;           /* 0 = 8 */
    int32_t n_threads, reserved;
} cm_circ_args;
int cm_circ_run(const cm_circ_args *args, cm_circ_stats *stats, char *err, uint64_t err_cap);

/* ---------------- stage 2, seeds and chains of many problems at once (opt-in device path) ----------------
 * One problem = what ProcessCirc::chaining (src/process_circ.cpp:677-737) does for one gene and one unmapped part of an oriented
 * mate: the 8-mer seeds every 3 bases of [qs, qe] (1-based, inclusive) looked up in the gene's regional table
 * (RegionalHashTable::create_table, src/hash_table.cpp:58-112) and chained k-best (chain_seeds_sorted_kbest2, src/chain.cpp:310-539).
 * gene_start / gene_end: contig coordinates, 1-based inclusive; seq_off / seq_len: the oriented mate in the byte arena `seqs`,
 * as the reference holds it in Record::seq / Record::rcseq (a reverse complement has NUL for a byte outside ACGTN); qe <= seq_len. */
typedef struct cm_circ_chain_req {
    uint32_t gene_start, gene_end;
    uint64_t seq_off;
    uint32_t seq_len, qs, qe;
    uint32_t tag;            /* the caller's word, not read by the chaining (cm_circ_chain_list: the piece, 0 or 1) */
} cm_circ_chain_req;
/* n_chains: chains the reference keeps (<= max_chain_len); n_stored = min(n_chains, 10), all a consumer reads (TOPCHAIN,
 * src/process_circ.cpp:19); listed: seeds with a valid code; flags bit 0: the problem was refused (it does not fit the device
 * workspace) and nothing else of it is written; chain_off: its first chain in the chain arrays.  Chain c has score[c] (the float
 * of the fp64 score), len[c] fragments and its fragments at rpos / qpos[frag_off[c] ..): contig position of the hit, 0-based
 * offset of the seed on the mate.  All offsets are running sums in request order, so equal answers are equal bytes. */
typedef struct cm_circ_chain_res {
    uint32_t n_chains, n_stored, listed, flags;
    uint64_t chain_off;
} cm_circ_chain_res;
#define CM_CIRC_CHAIN_REFUSED 1u
/* All problems of a batch on the device, against the annotation loaded in `slot` (cm_load_annotation).  genome: host bytes in the
 * cm_index_view.genome convention (only the merged spans of the listed genes are uploaded); NULL takes the contig resident in the
 * slot (CM_EINVAL if there is none; ref_len is then the resident one).  window_size 0 = 8, 6 .. 10 accepted, else CM_ELIMIT.
 * Capacities are the caller's: cap_chains >= sum of n_stored, cap_frags >= sum of fragments (10 * listed per request always
 * suffice); too small is CM_ELIMIT and the context stays usable.  *n_chains_out / *n_frags_out: what was used.
 * Tables are built once per distinct gene; their memory per pass is bounded (CM_CIRC_TABLE_BYTES, default 1 GiB): the genes are
 * worked through in groups that fit, a gene that alone exceeds the bound refuses its problems.  CM_CIRC_LOG_CAP: improvement-log
 * entries per resident problem (default 65536).  A refused problem is for the caller to answer with cm_circ_chain_host.
 * The device memory of a call is the context's: grow-only buffers that a later call of the same or a smaller size reuses without
 * allocating, that a larger call or a changed CM_CIRC_LOG_CAP re-sizes, and that cm_destroy releases.  With CM_CIRC_TRACE set every
 * call prints `workspace: <n> allocations, <bytes> held` to stderr.
 * stats: distinct genes, table bytes (largest group), gene groups, DP cells, log events, refused problems, device time of the
 * tables and of the chaining from HIP events (microseconds: the array holds integers). */
int cm_circ_chain_batch(cm_ctx *ctx, int slot, int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs, uint64_t seqs_len,
                        const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                        uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                        uint64_t *n_frags_out, uint64_t stats[8]);
/* The same requests answered by the serial statement (Caller::chains_of + cm_regional_table_build) into the same layout: the
 * checker of the device path and its fall-back.  Never refuses.  stats may be NULL; [0] distinct genes, [3] cells, [4] log events,
 * [5] 0, [7] the longest log of one problem, the others 0. */
int cm_circ_chain_host(const cm_params *p, const cm_annot_view *av, int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs,
                       uint64_t seqs_len, const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                       uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                       uint64_t *n_frags_out, uint64_t stats[8]);
/* The problems cm_circ_call_device lists for the eligible pairs of contig `contig` of a sorted batch: pair-major, genes in the
 * interval's order, piece 0 (mate 1) then 1.  A CHIBSJ pair lists the unmapped side of its split mate, a CHI2BSJ pair both sides
 * (call_circ_single_split called from call_circ_double_split asks for one of the same two).  The oriented mates go to `seqs` one
 * after the other (seq_off of the requests).  pair_of[i]: the batch index of request i's pair.  Returns CM_ELIMIT with the needed
 * sizes in *n_req / *seqs_len when a capacity is too small (call with 0 capacities to size). */
int cm_circ_chain_list(const cm_params *p, int32_t window_size, const cm_annot_view *av, const cm_chr_info *chrs, uint32_t n_chr,
                       const cm_fastq_batch *sorted, int32_t contig, cm_circ_chain_req *req, uint64_t *pair_of, uint64_t cap_req, uint8_t *seqs,
                       uint64_t cap_seqs, uint64_t *n_req, uint64_t *seqs_len);
/* cm_circ_call with the seeds and chains of every pair taken from cm_circ_chain_batch (ctx, slot: the contig's annotation is
 * loaded into the slot here, contig by contig) and the rest -- split_realignment, the judges, placement -- on the host threads
 * as in cm_circ_call.  A refused problem is recomputed on the host.  ctx == NULL answers the problems with cm_circ_chain_host
 * instead (the same provider path without a device).  The two files are cm_circ_call's byte for byte, for any thread count. */
int cm_circ_call_device(cm_ctx *ctx, int slot, const cm_params *p, int32_t window_size, uint32_t n_contigs, const cm_index_view *contigs,
                        const cm_annot_view *annots, const cm_chr_info *chrs, uint32_t n_chr, const cm_fastq_batch *sorted,
                        const char *candidates_path, const char *report_path, cm_circ_stats *stats);
/* sizeof(cm_circ_chain_req), sizeof(cm_circ_chain_res): cm_abi_sizes for the two structs above (its own list is closed at 19). */
int cm_circ_chain_abi_sizes(uint32_t *out, uint32_t cap);
/* cm_circ_call_device against what a mapping context already holds: contig c and its annotation are resident in slot c of ctx
 * (cm_load_contig / cm_load_contig_raw / cm_build_contig + cm_load_annotation, as cm_mapping_run leaves them), so contig c's
 * problems go to cm_circ_chain_batch(ctx, slot = c, genome = NULL, ...): no annotation is loaded here, no second context is made
 * and no gene span is uploaded.  contigs: the HOST sequence of every contig (genome and ref_len; the tables are not read), which
 * the judges on the host threads read.  CM_ESTATE when one of the slots 0 .. n_contigs - 1 lacks its contig or its annotation
 * (nothing is written then).  The context is synchronised (cm_sync) before the first chain call; a resident batch, a staged batch
 * or a prefetch the rounds have left is neither read nor written, and cm_map_rounds works on afterwards as before.  The device
 * memory the chain calls need is the context's (grow-only, released by cm_destroy).  The two files are cm_circ_call's byte for byte. */
int cm_circ_call_resident(cm_ctx *ctx, const cm_params *p, int32_t window_size, uint32_t n_contigs, const cm_index_view *contigs,
                          const cm_annot_view *annots, const cm_chr_info *chrs, uint32_t n_chr, const cm_fastq_batch *sorted,
                          const char *candidates_path, const char *report_path, cm_circ_stats *stats);

/* ---------------- both stages in one call: mapping() then circ_detect() of the reference (src/circminer.cpp) ----------------
 * One process, one context, one load of genome and GTF.  The files it leaves are those of cm_mapping_run(args->map) followed by
 * cm_circ_run on its output with the same parameters and no environment opt-in set, byte for byte: the two remain files, the
 * mapping file of report 1 / 2, <out>.candidates.pam and <out>.circ_report.  The .srt files are the one difference, see below.
 * It always takes the device paths: no HIP device is CM_ENODEV (err says so), there is no host fall-back, and the variables that
 * select a path elsewhere (CM_FASTQ_DEVICE, CM_PAM_DEVICE, CM_SAM_DEVICE, CM_REMAIN_DEVICE, CM_REMAIN_SORTED, CM_CIRC_PRESORTED,
 * CM_CIRC_DEVICE) are not read.  The knobs and traces are: CM_FASTQ_DEVICE_BLOCK, CM_REMAIN_TIE_CAP, CM_CIRC_TABLE_BYTES,
 * CM_CIRC_LOG_CAP, CM_CIRC_THREADS, CM_REMAIN_TRACE, CM_CIRC_TRACE.
 * Memory hand-over (handover 0 and two regular plain-text FASTQ files of fresh reads -- no gzip, no pipe, no carried 23-token
 * headers): the device tokenises, formats the rows of the report mode and the remain records, and sorts every batch's records; the
 * sorted runs are merged in memory (cm_remain_runs_finish_mem), parsed from there (cm_fastq_open_mem) and called against the
 * contigs and annotations stage 1 left resident (cm_circ_call_resident).  The .srt files are written only with flags bit 0, and
 * are then the bytes cm_sort_remain makes of the remain files.
 * Files hand-over (any other input, or handover 1): the host parser feeds the device, the remain files are sorted by cm_sort_remain
 * into the .srt files, and those are parsed -- in the same process, against the same resident contigs and annotations.
 * Stage 2's judges read genome bytes on the host, so a detect run keeps each contig's sequence (not its k-mer tables) in host
 * memory until it returns: one byte per base (3.1 GB at hg38 size) that cm_mapping_run gives back after each upload.
 * map.world must be 0 or 1 (CM_EINVAL otherwise). */
typedef struct cm_detect_args {
    cm_mapping_args map;        /* as for cm_mapping_run; world must be 0 or 1 (else CM_EINVAL) */
    int32_t window_size;        /* stage 2, 0 = 8 */
    int32_t circ_threads;       /* host threads of the judges, 0 = map.n_threads */
    int32_t handover;           /* 0 = memory where the input allows it, 1 = through the remain / .srt files */
    int32_t flags;              /* bit 0: also write the two .srt files on the memory hand-over */
} cm_detect_args;
typedef struct cm_detect_stats {
    cm_mapping_stats map;
    cm_circ_stats circ;
    int32_t handover_used;      /* 0 memory, 1 files */
    int32_t reserved;
    uint64_t problems, refused, recomputed;   /* what CM_CIRC_TRACE prints today, summed over the contigs */
    double seconds_handover, seconds_total;
} cm_detect_stats;
int cm_detect_run(const cm_detect_args *args, cm_detect_stats *stats, char *err, uint64_t err_cap);
/* sizeof(cm_detect_args), sizeof(cm_detect_stats): cm_abi_sizes for the two structs above (its own list stays closed at 19). */
int cm_detect_abi_sizes(uint32_t *out, uint32_t cap);

/* sizeof of the structs above, in this order: cm_params, cm_index_view, cm_annot_view, cm_mapped_read, cm_reads, cm_record,
 * cm_chr_info, cm_fastq_batch, cm_mapping_args, cm_mapping_stats, cm_circ_res, cm_circ_args, cm_circ_stats, cm_index_raw, cm_build_stats, cm_dp_req,
 * cm_dp_res, cm_annot_req, cm_annot_res -- for a binding to
 * check its mirrors of them against the library it loaded.  Returns the number of entries written (cap must hold them). */
int cm_abi_sizes(uint32_t *out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* CIRCMINER_HOT_H */
