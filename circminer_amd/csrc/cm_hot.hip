// cm_hot.hip — gfx950 kernels + the C-ABI of include/circminer_hot.h.
//
// Launch structure of one mapping round (cm_map_round) over the resident read batch, per tile of
// pairs:  k_seed (one lane per k-mer probe)  ->  k_cells + k_scan (cells per chaining problem,
// exclusive offsets)  ->  k_chain (one lane per (mate, orientation) problem, DP cells and the
// improvement log in HBM workspace)  ->  k_pair (one lane per pair: pairing, extension,
// classification, round bookkeeping).  Index, genome, annotation, reads and per-pair state stay
// in HBM between rounds; nothing is copied back until cm_reads_download.
//
// There is no CPU path in this file: without a HIP device cm_create fails with CM_ENODEV.
#include <chrono>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>      // the oversize buckets of cm_build_contig only

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <functional>
#include <thread>
#include <vector>

#include "circminer_hot.h"
#include "cm_core.h"
#include "cm_aos.h"
#include "cm_index_build.h"
#include "cm_fastq_text.h"
#include "cm_pam_text.h"
#include "cm_remain_order.h"
#include "cm_remain_text.h"
#include "cm_sam_text.h"
#include "cm_circ_chain_ws.h"

using cmc::Core;
using cmc::KCore;

namespace {

constexpr int MAX_SLOTS = 16;
constexpr uint32_t TILE_PAIRS = 1u << 20;          // pairs per launch group (workspace sizing: ~46 KB of HBM per pair) ...
constexpr uint32_t TILE_PAIRS_MAX = 1u << 21;      // ... up to this for batches of more than two such groups (prepare_resident)
constexpr int BLK = 256;
constexpr int BLK_CHAIN = 64;
#include "cm_dp_engine.h"          // BLK_PAIR, CM_PAIR_WAVES, lbuf_bytes, lane_dp_mem, dp_queue_loop

// Profile classes: the index of cm_ctx::ms[] / launches[], of Timer, launch() and cm_prof_get (include/circminer_hot.h).  PC_NONE:
// a launch no class counts (index build, collect, the small housekeeping kernels).
enum ProfClass { PC_NONE = -1, PC_SEED = 0, PC_CHAIN = 1, PC_PAIR = 2, PC_SCAN = 3, PC_HEAVY = 4, PC_ORDER = 5, PC_CHAIN_HEAVY = 6, PC_PREFETCH = 7,
                 PC_ROWS = 7 /* the same slot: PC_PREFETCH counts launches and has no time, the row formatters (cm_format_pam, cm_format_sam) have time and count none */, PC_COUNT = 8 };
// The words of cm_ctx::d_counters.  0 - 6 are public (cm_prof_counters, include/circminer_hot.h); from 8 on what a diagnostic build
// accumulates, read by the scripts of tests/diag through cm_debug_counters at these indices.  The two diagnostic builds overlap (they
// are never one build): both write word 24.
enum Counter {
    CN_PROBES = 0 /* + 1: touches, + 2: hits (k_seed) */, CN_PAIR_ROUNDS = 3, CN_RERUN = 4 /* ... mapped by the re-run launch */,
    CN_FALL = 5, CN_FALL_2ND = 6,                    // pairs the pipeline handed to its fall-back list; those of the second attempt
    CN_DEAD_CHAINS = 7,                              // chaining problems with hits that were not chained (k_chain_cls, quad_dead): read through cm_debug_counters
    // -DCM_CHAIN_DIAG (k_chain_heavy): lane sums [5], wave time per phase [3], wave time per DP step [4], shape of the back-tracking
    CN_CD_LANE = 8, CN_CD_PHASE = 13, CN_CD_WAVE = 16, CN_CD_EVENTS = 20, CN_CD_LEVELS = 21, CN_CD_PROBLEMS = 22, CN_CD_PASSES = 23, CN_CD_CELLS = 24,
    CN_CD_REGLOG = 25, CN_CD_BATCHES = 26, CN_CD_PRE_USED = 27, CN_CD_PRE_UNUSED = 28,      // problems whose log fits registers, candidate batches, scores asked for ahead
    // -DCM_HP_DIAG (cm_heavy_pipe.h): list sizes per attempt [6] at CN_HP_ATTEMPT + CN_HP_STRIDE * attempt, then the fold's counts
    CN_HP_ATTEMPT = 8, CN_HP_STRIDE = 8, CN_HP_UNPAIRED = 24, CN_HP_CHAINS = 25, CN_HP_SEQ_TASKS = 26, CN_HP_EARLY = 27, CN_HP_EARLY_FIRST = 28,
    CN_WORDS = 32
};
static_assert(CN_CD_CELLS < CN_WORDS && CN_HP_EARLY_FIRST < CN_WORDS && CN_HP_ATTEMPT + CN_HP_STRIDE + 5 < CN_HP_UNPAIRED, "d_counters has CN_WORDS words");
// The 64-bit words of the page-locked landing zone of the scalar read-backs (cm_ctx::h_pin).
enum Pin {
    PIN_COLLECT_N = 0, PIN_COLLECT_ERR = 1,          // cm_collect_*: active pairs, the device error word
    PIN_DEV_ERR = 0,                                 // check_dev_err: the device error word (word 0 again: either caller waits for its copy at once)
    PIN_POOL_ERR = 2,                                // run_chain_tile: the error word behind a launch group
    PIN_HEAVY_LOAD = 4,                              // k_pair_cost's sum over the tile last sent (cm_ctx::h_pin_nt)
    PIN_CELLS = 8,                                   // + 2 * seed set: DP cells of the tile, + 1: of its largest problem
    PIN_RERUN_N = 12, PIN_FALL_N = 14,               // + chain-record set: length of the re-run list / of the pipeline's fall-back list
    PIN_TEXT = 16,                                   // cm_reads_stage_text: the result block of the tokeniser (cmft::RES_WORDS words)
    PIN_ROWS = 26,                                    // cm_format_pam / cm_format_sam: the bytes of the rows; cm_format_remain: + 1, of the second file
    PIN_TIES = 28,                                    // cm_format_remain_sorted: the tie groups' counters (three 32-bit words)
    PIN_WORDS = 32
};
constexpr size_t PIN_BYTES = PIN_WORDS * sizeof(unsigned long long);        // allocated and cleared in cm_create
static_assert(PIN_BYTES == 256 && PIN_FALL_N + 1 < PIN_TEXT && PIN_CELLS + 3 < PIN_RERUN_N && PIN_TEXT + cmft::RES_WORDS <= PIN_ROWS && PIN_ROWS + 1 < PIN_TIES && PIN_TIES + 1 < PIN_WORDS,
              "the landing zone has 32 words");
struct ReadsDev {
    const uint8_t *seq1, *seq2;
    const uint64_t *off1, *off2;
};

// ------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(BLK) k_seed(KCore kc, ReadsDev rd, const uint8_t *active, uint64_t pair0, uint32_t n_tile, int S,
                                              uint32_t *sstart, uint32_t *scnt, uint32_t *sraw, unsigned long long *counters) {
    const Core c = cmc::to_core(kc);
    __shared__ unsigned int sh[3];
    if (threadIdx.x < 3) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t q = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    const uint64_t total = (uint64_t)n_tile * 4u * (uint64_t)S;         // > 0: the grid has ceil(total / BLK) blocks
    const bool in = q < total;
    const uint64_t qc = in ? q : total - 1;                            // a lane past the end asks for what the last probe asks for
    uint32_t s;
    uint64_t r;
    if ((total >> 32) == 0) {                                          // (uniform) the usual tile: 32-bit division
        s = (uint32_t)qc % (uint32_t)S;
        r = (uint32_t)qc / (uint32_t)S;
    } else {
        s = (uint32_t)(qc % (uint64_t)S);
        r = qc / (uint64_t)S;
    }
    const int orient = (int)(r & 1u), mate = (int)((r >> 1) & 1u);
    const uint64_t p = pair0 + (r >> 2);
    // the flag and both offsets leave together (off[p + 1] exists for every pair), the branch comes after them
    const uint8_t act = active[p];
    uint64_t o[2];
    __builtin_memcpy(o, (mate ? rd.off2 : rd.off1) + p, sizeof(o));
    const int len = (int)(o[1] - o[0]);
    const int k = c.P.kmer;
    uint32_t st = 0, cn = 0, rw = 0, pt = 0;                           // pt = 1 << 16 | touches of a lane that probed
    if ((int)in & (int)(act != 0) & (int)((int)(s + 1) * k <= len)) {   // (one condition, no short cut: it needs all three loads)
        const cmc::Read R{(cmc::g_u8)((mate ? rd.seq2 : rd.seq1) + o[0]), len, orient};
        const cmc::Probe pr = cmc::seed_probe(c, R.view(), (int)s * k);
        st = pr.start;
        rw = pr.raw;
        cn = (pr.raw > (uint32_t)c.P.seed_lim) ? 0u : pr.raw;
        pt = 0x10000u | pr.touches;                                    // touches <= 2 * 32 + 2 per probe (probe_search over n < 2^32)
    }
    if (in) {
        sstart[q] = st;
        scnt[q] = cn;
        sraw[q] = rw;
    }
    // The three counters, one sum per wave: every lane of every wave is here (no lane has left, the branches above have joined),
    // so the cross-lane adds see all 64 values.  Rows of 16 by rotation, the four row sums through lane reads.
    uint32_t a = pt, b = cn;
#define CM_ROW_ADD(v, n) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 | (n), 0xF, 0xF, false)      /* DPP row_ror:n */
    CM_ROW_ADD(a, 1); CM_ROW_ADD(b, 1);
    CM_ROW_ADD(a, 2); CM_ROW_ADD(b, 2);
    CM_ROW_ADD(a, 4); CM_ROW_ADD(b, 4);
    CM_ROW_ADD(a, 8); CM_ROW_ADD(b, 8);
#undef CM_ROW_ADD
    uint32_t wa = 0, wb = 0;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        wa += (uint32_t)__builtin_amdgcn_readlane((int)a, 16 * row);
        wb += (uint32_t)__builtin_amdgcn_readlane((int)b, 16 * row);
    }
    if ((threadIdx.x & 63u) == 0 && wa) {
        atomicAdd(&sh[0], wa >> 16);
        atomicAdd(&sh[1], wa & 0xFFFFu);
        if (wb) atomicAdd(&sh[2], wb);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sh[threadIdx.x]) atomicAdd(&counters[CN_PROBES + threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

// cells per chaining problem + exclusive scan over the problems of a tile (3 phases):
// k_scan_a: per block of SCAN_ELEMS problems, cells[r] = sum of its seed counts, block-local
// exclusive offsets and the block total; k_scan_mid: one workgroup scans the block totals;
// k_scan_c: adds the block base.  out[n] = grand total.
constexpr int SCAN_T = 256;
constexpr int SCAN_ELEMS = 1024;       // 4 per thread
// A chaining problem whose chains nobody reads: it has retained hits (cells > 0), the other mate of its pair has none in either
// orientation.  process_read (cm_core.h) settles such a pair as CM_OEANCH from "has this mate a chain" alone, and a problem has a
// chain exactly when it has a retained hit (chain_kbest returns 0 only for kc <= 0; the back-tracking always emits the first event
// of the best group; max_chain_len >= 1, cm_create).  So the answer is in the seed counts, and the problem is not chained at all.
// The four problems of a pair (r = 4 t + 2 mate + orientation) are a quad of consecutive lanes: `cells` of the caller's own problem,
// all four lanes of the quad in the same state of execution.
constexpr int CHAIN_CLS_NONE = -2;      // class of a problem without a retained hit: no chain, no kernel visits it
constexpr int CHAIN_CLS_DEAD = -3;      // class of a dead problem: hits, but not chained; the pair stage sees the marker nchain = 1
__device__ inline bool quad_dead(uint32_t cells) {
    const uint32_t mate = cells + (uint32_t)__shfl_xor((int)cells, 1);         // both orientations of this problem's mate
    const uint32_t other = (uint32_t)__shfl_xor((int)mate, 2);                 // ... of the other mate
    return cells > 0 && other == 0;
}
static_assert(SCAN_T % 4 == 0 && SCAN_ELEMS % SCAN_T == 0 && BLK % 4 == 0, "a pair's four problems are one aligned quad of lanes in k_scan_a and k_chain_cls");
// skip_dead: a dead problem counts 0 cells (no DP workspace, not the tile's largest problem)
__global__ void __launch_bounds__(SCAN_T) k_scan_a(const uint32_t *scnt, int S, uint32_t n, unsigned long long *out, unsigned long long *bsum,
                                                   unsigned int *bmax, int skip_dead) {
    // element k * SCAN_T + t of the block belongs to thread t: consecutive lanes read consecutive problems
    // (28-byte stride, the S loads of a lane reuse its sectors) instead of four problems per lane
    __shared__ unsigned long long sh[SCAN_T];
    __shared__ unsigned int shmax;
    const uint32_t base = blockIdx.x * SCAN_ELEMS;
    unsigned long long run = 0;
    unsigned int my_max = 0;                     // the largest problem of the block (cells = retained hits): sizes k_chain_heavy's LDS
    if (threadIdx.x == 0) shmax = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ELEMS / SCAN_T; ++k) {
        const uint32_t r = base + k * SCAN_T + threadIdx.x;
        uint32_t c = 0;
        if (r < n)
            for (int s = 0; s < S; ++s) c += scnt[(uint64_t)r * S + s];
        if (skip_dead && quad_dead(c)) c = 0;           // (n is a multiple of 4: a quad is inside the tile or outside)
        my_max = c > my_max ? c : my_max;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (int d = 1; d < SCAN_T; d <<= 1) {
            const unsigned long long x = (threadIdx.x >= (unsigned)d) ? sh[threadIdx.x - d] : 0ull;
            __syncthreads();
            sh[threadIdx.x] += x;
            __syncthreads();
        }
        if (r < n) out[r] = run + sh[threadIdx.x] - c;
        run += sh[SCAN_T - 1];
        __syncthreads();
    }
    atomicMax(&shmax, my_max);
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = run;
        bmax[blockIdx.x] = shmax;
    }
}
// The middle kernel of both multi-block scans (this one and k_scan32_*): one workgroup scans the nb block totals in place.
// WITH_MAX: also the grand total and the largest of bmax[] -> total[0], total[1] (else neither pointer is touched).
template <class T, bool WITH_MAX>
__global__ void __launch_bounds__(1024) k_scan_mid(T *bsum, uint32_t nb, T *total, const unsigned int *bmax) {
    __shared__ T part[1024];
    __shared__ unsigned int gmax;
    const uint32_t t = threadIdx.x;
    const uint32_t chunk = (nb + 1023u) / 1024u;
    const uint32_t a = t * chunk, b = (a + chunk < nb) ? a + chunk : nb;
    T s = 0;
    unsigned int m = 0;
    if (WITH_MAX && t == 0) gmax = 0;
    if constexpr (WITH_MAX) __syncthreads();
    for (uint32_t i = a; i < b; ++i) {
        s += bsum[i];
        if constexpr (WITH_MAX) m = bmax[i] > m ? bmax[i] : m;
    }
    if constexpr (WITH_MAX) atomicMax(&gmax, m);
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const T v = (t >= d) ? part[t - d] : (T)0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    T run = t ? part[t - 1] : (T)0;
    for (uint32_t i = a; i < b; ++i) {
        const T x = bsum[i];
        bsum[i] = run;
        run += x;
    }
    if (WITH_MAX && t == 1023) {
        total[0] = part[1023];
        total[1] = gmax;                          // (every atomicMax above is followed by a barrier of the scan)
    }
}
__global__ void __launch_bounds__(SCAN_T) k_scan_c(unsigned long long *out, const unsigned long long *bsum, uint32_t n) {
    const uint32_t i = blockIdx.x * SCAN_T + threadIdx.x;
    if (i < n) out[i] += bsum[i / SCAN_ELEMS];
}

// bases of a problem's best chain left to extend on the left / right (work proxies of the pair-stage ordering):
// left in the low byte, right in the high byte, each capped at 255
__device__ inline int pack_resid(int left, int right) {
    left = left < 0 ? 0 : (left > 255 ? 255 : left);
    right = right < 0 ? 0 : (right > 255 ? 255 : right);
    return left | (right << 8);
}
#ifndef CM_CHAIN_WAVES
#define CM_CHAIN_WAVES 5
#endif
__global__ void __launch_bounds__(BLK_CHAIN, CM_CHAIN_WAVES) k_chain(KCore kc, ReadsDev rd, const uint8_t *active, uint64_t pair0, uint32_t r0, uint32_t r1, int S,
                                                     const uint32_t *sstart, const uint32_t *scnt, const uint32_t *sraw,
                                                     const unsigned long long *celloff, unsigned long long cellbase, double *dp_score,
                                                     int32_t *dp_prev, uint8_t *pool, unsigned long long pool_bytes,
                                                     unsigned long long *pool_cursor, cm_chain *chains, int32_t *nchain, int32_t *high, int *err,
                                                     uint16_t *resid, const uint32_t *perm, const unsigned int *perm_lo, const unsigned int *perm_hi,
                                                     const int8_t *cls) {
    // perm == null: problems r0..r1 in index order, but for the dead ones (cls, may be null: none is dead), whose three fields
    //               k_chain_cls / k_chain_apply have written and which have no DP cells;
    // perm != null: the light problems perm[*perm_lo .. *perm_hi), grouped by work class so that the lanes of a wave carry similar DPs
    uint32_t r = r0 + blockIdx.x * BLK_CHAIN + threadIdx.x;
    if (perm) {
        r += *perm_lo;
        if (r >= *perm_hi) return;
        r = perm[r];
    } else if (r >= r1 || (cls && cls[r] == CHAIN_CLS_DEAD)) return;
    const Core c = cmc::to_core(kc);
    const uint64_t p = pair0 + (r >> 2);
    int n = 0, hh = 0, rs = 0;
    if (active[p]) {
        const int mate = (int)((r >> 1) & 1u);
        const uint64_t o0 = mate ? rd.off2[p] : rd.off1[p], o1 = mate ? rd.off2[p + 1] : rd.off1[p + 1];
        const int len = (int)(o1 - o0);
        uint32_t st[cmc::MAX_SEEDS], cn[cmc::MAX_SEEDS];
        for (int s = 0; s < S; ++s) {
            st[s] = sstart[(uint64_t)r * S + s];
            cn[s] = scnt[(uint64_t)r * S + s];
            if (sraw[(uint64_t)r * S + s] > 0 && cn[s] == 0) ++hh;       // get_best_chains high_hits
        }
        cmc::ChainWork w;
        w.dp_score = (CM_G double *)(dp_score + (celloff[r] - cellbase));
        w.dp_prev = (CM_G int32_t *)(dp_prev + (celloff[r] - cellbase));
        w.pool = (CM_G uint8_t *)pool;
        w.pool_bytes = pool_bytes;
        w.pool_cursor = (CM_G unsigned long long *)pool_cursor;
        w.err = (cmc::g_err)err;
        n = cmc::chain_kbest(c, len, S, st, cn, w, (CM_G cm_chain *)(chains + (uint64_t)r * CM_BESTCHAINLIM));
        if (n > 0) {          // bases of the best chain left to extend (work proxy used by the pair-stage ordering)
            const cm_chain &b = chains[(uint64_t)r * CM_BESTCHAINLIM];
            rs = pack_resid(b.qpos[0], len - (b.qpos[b.chain_len - 1] + c.P.kmer));
        }
    }
    nchain[r] = n;
    high[r] = hh;
    resid[r] = (uint16_t)rs;
}

// The reference has no per-pair capacity limits inside maxReadLength (its extension memo is an unbounded std::map,
// src/extend.cpp:299,375); the device keeps 8 memo entries per extend call in registers / scratch.  A pair that would need more
// (and could observe the difference, cm_core.h memo_put) is not allowed to fail the batch: both pair kernels leave it untouched,
// append it to `list`, and a second launch of k_pair over that list -- queued behind them unconditionally, it reads `count` on
// the device -- maps it with a spill area of `spill_cap` more entries per lane in global memory and longer DP staging buffers.
struct RetryArgs {
    uint32_t *pair_err;          // one word per pair of the tile, all zero between launches
    uint32_t *list;              // pairs (tile-relative) to re-run
    unsigned int *count;
    cmc::MemoSpill *spill;       // re-run only
    int spill_cap;
    int first;                   // 1: first pass (record, skip, queue)   0: the re-run
};

// The pair stage's light kernel and its re-run (RetryArgs) are the same code: FIRST = the first pass over the tile (a pair that
// hits a device capacity is recorded, skipped and queued), !FIRST = the re-run of the queued pairs (k_pair_rerun: spill memo,
// longer staging buffers, limits fail the call).  Two kernel symbols, so that profiles tell the two launches apart.
template <bool FIRST>
__device__ __forceinline__ void pair_kernel(const KCore &kc, const ReadsDev &rd, uint64_t pair0, uint32_t n_tile, const cm_chain *chains, const int32_t *nchain,
                                            const int32_t *high, cm_mapped_read *state, uint8_t *active, int32_t *cat, int is_last,
                                            int *err, unsigned long long *counters, int str_cap, unsigned long long *lane_clk,
                                            const uint32_t *perm, const unsigned int *n_light, unsigned int *next_chunk,
                                            const RetryArgs &ra) {
    const unsigned long long clk0 = lane_clk ? wall_clock64() : 0ull;
    // per-lane staging buffers for the two DP strings, word-interleaved across the wave (lane_dp_mem)
    extern __shared__ uint32_t lds_words[];
#if defined(CM_DIAG)
    __shared__ unsigned long long tick_w[65];
    cmc::Tick tick;
    for (int i = 0; i < 32; ++i) tick.acc[i] = 0;
    tick.last = wall_clock64();
    tick.w = (CM_L unsigned long long *)tick_w;
    tick.wave_on = 1;
    for (int i = threadIdx.x; i < 65; i += BLK_PAIR) tick_w[i] = i == 0 ? tick.last : 0ull;
    __syncthreads();
    cmc::DpMem sm = lane_dp_mem((CM_S uint8_t *)lds_words, threadIdx.x, str_cap, (cmc::g_err)err, &tick);
#else
    cmc::DpMem sm = lane_dp_mem((CM_S uint8_t *)lds_words, threadIdx.x, str_cap, (cmc::g_err)err);
#endif
    if (ra.spill) {          // the exact re-run of the pairs the first pass gave up on: a memo that holds every exon piece
        sm.spill = (cmc::g_spill)(ra.spill + ((size_t)blockIdx.x * BLK_PAIR + threadIdx.x) * (size_t)ra.spill_cap);
        sm.spill_cap = ra.spill_cap;
    }
    const Core c = cmc::to_core(kc);
    // persistent grid: the launch places every workgroup at once (gridDim <= resident capacity), so the dispatcher is free
    // for the kernels of the next round that other streams run at the same time.  A wave takes the next 64 pairs of the list
    // (light pairs only, in bucket order: most expensive classes first) from a shared cursor whenever it is done with its
    // last: waves that drew cheap pairs take more of them, and all of them finish within one chunk of each other.
    const uint32_t n_l = *n_light;
    auto take = [&]() { return (uint32_t)__shfl((int)(threadIdx.x == 0 ? atomicAdd(next_chunk, 1u) : 0u), 0); };
    for (uint32_t chunk = take(); (uint64_t)chunk * BLK_PAIR < n_l; chunk = take()) {
    const uint32_t slot = chunk * BLK_PAIR + threadIdx.x;
    if (slot >= n_l) continue;
    const unsigned long long it0 = lane_clk ? wall_clock64() : 0ull;
    const uint32_t t = perm[slot];
    const uint64_t p = pair0 + t;
    const uint64_t a0 = rd.off1[p], a1 = rd.off1[p + 1], b0 = rd.off2[p], b1 = rd.off2[p + 1];
    cmc::ChainSet sets[4];
    int hh[4];
    for (int x = 0; x < 4; ++x) {
        const uint64_t r = (uint64_t)t * 4 + x;
        sets[x].ch = (cmc::g_chain)(chains + r * CM_BESTCHAINLIM);
        sets[x].n = nchain[r];
        hh[x] = high[r];
    }
    cm_mapped_read mr = state[p];
    // First pass: a device-capacity limit hit by this pair (cmc::ERR_MEMO / ERR_BAND) is recorded in the pair's own word; such
    // a pair keeps its inputs (nothing is written) and is queued for the re-run.  Re-run (ra.first == 0): limits go to the
    // launch-wide word and fail the call -- with the spill memo and the longer staging buffers none is known to be reachable.
#if defined(CM_AB_GLOBAL_ERR)          // A/B experiment only: what the per-pair error word costs (results wrong for pairs over a capacity)
    int *perr = err;
#else
    int *perr = FIRST ? (int *)(ra.pair_err + t) : err;
    sm.err = (cmc::g_err)perr;
#endif
    const int st = cmc::process_read(c, sm, (cmc::g_u8)(rd.seq1 + a0), (int)(a1 - a0), (cmc::g_u8)(rd.seq2 + b0), (int)(b1 - b0), sets, hh, mr, (cmc::g_err)perr);
    bool keep = true;
    if (FIRST) {
        if (__hip_atomic_load(ra.pair_err + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            ra.list[atomicAdd(ra.count, 1u)] = t;
            active[pair0 + t] = 1;          // until the re-run writes its flag: counted as active (the next item's seeds may be computed before that)
            keep = false;
        }
    } else ra.pair_err[t] = 0u;
    if (keep) {
        uint8_t act = 1;
        cmc::finish_round(c, st, is_last, (int)(a1 - a0), (int)(b1 - b0), mr, act);
        state[p] = mr;
        active[p] = act;
        cat[p] = st;
    }
    {   // pair-rounds counter: one atomic per wave (a pair left to the re-run is counted there)
        const unsigned long long m = __ballot(1), mk = __ballot(keep);
        if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1 && mk) {
            atomicAdd(&counters[CN_PAIR_ROUNDS], (unsigned long long)__popcll(mk));
            if (!FIRST) atomicAdd(&counters[CN_RERUN], (unsigned long long)__popcll(mk));       // pairs mapped by the re-run launch
        }
    }
#if defined(CM_DIAG)
    CM_TICK(sm, 13);
    if (lane_clk) {                                           // section timing study: 16 words per pair
        for (int i = 0; i < 15; ++i) lane_clk[p * 16 + i] = tick.acc[i];
        lane_clk[p * 16 + 15] = wall_clock64() - clk0;
        // wave-level rows behind the per-pair rows (second half of the buffer): [wave][0] = wave time, [wave][1] = lane-weighted
        const unsigned long long m = __ballot(1);
        if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1) {
            unsigned long long *wr = lane_clk + (unsigned long long)n_tile * 16 + (unsigned long long)blockIdx.x * 64;
            for (int i = 0; i < 64; ++i) wr[i] = tick_w[1 + i];
        }
    }
#else
    // diagnostic only (CM_LANE_CLK=1), in processing order (64 consecutive slots = one wave iteration): low word = the
    // wave's time for this iteration (100 MHz ticks; the clock is read after the lanes have reconverged), high word = the pair
    if (lane_clk) lane_clk[slot] = ((wall_clock64() - it0) & 0xFFFFFFFFull) | ((unsigned long long)t << 32);
#endif
    }
}


__global__ void __launch_bounds__(BLK_PAIR, CM_PAIR_WAVES) k_pair(KCore kc, ReadsDev rd, uint64_t pair0, uint32_t n_tile, const cm_chain *chains, const int32_t *nchain,
                                                   const int32_t *high, cm_mapped_read *state, uint8_t *active, int32_t *cat, int is_last,
                                                   int *err, unsigned long long *counters, int str_cap, unsigned long long *lane_clk,
                                                   const uint32_t *perm, const unsigned int *n_light, unsigned int *next_chunk,
                                                   RetryArgs ra) {
    pair_kernel<true>(kc, rd, pair0, n_tile, chains, nchain, high, state, active, cat, is_last, err, counters, str_cap, lane_clk, perm, n_light, next_chunk, ra);
}
__global__ void __launch_bounds__(BLK_PAIR, CM_PAIR_WAVES) k_pair_rerun(KCore kc, ReadsDev rd, uint64_t pair0, uint32_t n_tile, const cm_chain *chains,
                                                         const int32_t *nchain, const int32_t *high, cm_mapped_read *state, uint8_t *active, int32_t *cat,
                                                         int is_last, int *err, unsigned long long *counters, int str_cap,
                                                         unsigned long long *lane_clk, const uint32_t *perm, const unsigned int *n_light,
                                                         unsigned int *next_chunk, RetryArgs ra) {
    pair_kernel<false>(kc, rd, pair0, n_tile, chains, nchain, high, state, active, cat, is_last, err, counters, str_cap, lane_clk, perm, n_light, next_chunk, ra);
}

// ---- wave-cooperative chaining of heavy problems ----------------------------------------------
// chain_seeds_sorted_kbest (src/chain.cpp:73-301) for ONE problem per wave.  For slot ii the cells i are
// independent given the slots > ii, except for the reference's shared cursor lb_ind[jj]
// (src/chain.cpp:133-160).  That cursor only differs from upper_bound(hits of jj, hit i) when an earlier
// cell skipped the list with the maxIntronLen test, and the difference is observable only if a later
// cell's window (max_lpos_lim) reaches a hit more than maxIntronLen away, i.e. only if the annotation
// has an exon or an exon->next-exon hop longer than maxIntronLen.  cm_load_annotation checks that
// (Slot::chain_parallel_ok); if it ever fails, heavy problems stay on the sequential kernel.
// Order of the improvement log = reference insertion order (ii desc, i asc, then (jj, j) asc): each batch
// of 64 cells is evaluated twice, first to count the improvements per cell, then (after a wave scan) to
// store them at their final offsets.
template <class T> __device__ inline T wave_excl_scan(T v, int lane, T &total) {
    T x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    total = __shfl(x, 63);
    return x - v;
}
#ifndef CM_CHEAVY_LOG_REGS
#define CM_CHEAVY_LOG_REGS 4   // k_chain_heavy back-tracks a log of up to 64 x this many events from registers (a test build: 1)
#endif
struct HeavyChainCtx {
#if defined(CM_CHAIN_DIAG)
    unsigned long long *tk;      // per-lane ticks: [0] binary searches, [1] upper_bound, [2] window loops, [3] cells, [4] pair evaluations, [5] / [6] see k_chain_heavy
#endif
    const Core *c;
    CM_L const uint32_t *LP;     // hit positions of every slot, concatenated (LDS)
    CM_L const uint32_t *NB;     // near-border bit of every cell of the slots that are evaluated (LDS bitmask, see k_chain_heavy)
    CM_L const uint32_t *IM;     // "improved" bit of every cell (LDS bitmask, words per slot: heavy_im_word)
    const uint32_t *base, *cnt;  // per slot (uniform)
    int kc, seq_len;
    CM_G double *dps;
    CM_G int32_t *dpp;
};
// The improved bit of cell (s, i) lies in word heavy_im_word(base[s], s) + (i >> 5), bit i & 31: every slot starts at a 64-bit
// boundary of its own, so the bits of a batch of 64 cells are two whole words that one ballot writes (no LDS atomics).  A slot's
// words begin at or behind the flat bit position of its first cell, shifted by one 64-bit word per earlier slot: slots never
// overlap and all of them end within heavy_im_words(ncell, kc) words.
__device__ inline uint32_t heavy_im_word(uint32_t base_s, uint32_t s) { return 2u * ((base_s >> 6) + s); }
__host__ __device__ inline uint32_t heavy_im_words(uint32_t ncell, uint32_t kc) { return 2u * ((ncell >> 6) + kc + 1u); }
// evaluates cell (ii, i); returns the number of strict improvements; stores them to ev[] when ev != null.  A cell of a later slot
// that no evaluation improved still has its initial score, (double)kmer: only improved cells are in HBM (see k_chain_heavy).
__device__ inline uint32_t heavy_cell(const HeavyChainCtx &h, int ii, uint32_t i, CM_G cmc::Event *ev, double &out_score, int32_t &out_prev,
                                     double &e0, double &e1) {
    const Core &c = *h.c;
    const int kmer = c.P.kmer;
    const uint32_t read_remain = (uint32_t)(h.seq_len - ii * kmer - kmer);
    const int32_t cur_info = (int32_t)h.LP[h.base[ii] + i];
    const uint32_t seg_start = (uint32_t)cur_info, seg_end = (uint32_t)cur_info + kmer - 1;
    uint32_t max_lpos_lim = cmc::MAXUB, max_exon_end = 0;
    int ol = -1;
    double my_score = (double)kmer;
    int32_t my_prev = -1;
    uint32_t n = 0;
    // cmc::upper_bound of a hit near an exon border was resolved before the DP (k_chain_heavy) and parked in the cell's own score /
    // back-pointer slots, which nothing reads before this cell has been evaluated; asked for now, needed after the first binary search
    const uint32_t cell = h.base[ii] + i;
    const bool near = (h.NB[cell >> 5] >> (cell & 31)) & 1u;
    uint2 parked = make_uint2(0u, 0u);
    int parked_ol = -1;
    if (near) {
        parked = *(CM_G const uint2 *)(h.dps + cell);
        parked_ol = h.dpp[cell];
    }
#if defined(CM_CHAIN_DIAG)
    if (!ev) h.tk[3] += 1;
#define CD_T0 const unsigned long long cd_t = wall_clock64()
#define CD_ADD(k) h.tk[k] += wall_clock64() - cd_t
#else
#define CD_T0
#define CD_ADD(k)
#endif
    // The later slots are taken four at a time, in two passes.  The first runs the binary searches and asks for the score of each
    // slot's first hit right of this one (where it is within maxIntronLen, improved, and inside the window of a hit away from
    // every exon border: a near-border hit's window is still on its way, so its load is speculative -- the cell is one of this
    // problem's own); the second is the evaluation in the reference's (jj, j) order, which finds those scores in registers.
    // A cell with hits in three later slots waits for one round trip instead of three; further hits of a window (one evaluation
    // in eight) are loaded in place.
    const uint32_t own_lim = seg_start + read_remain + (uint32_t)c.P.max_ed;
    for (int j0 = ii + 1; j0 < h.kc; j0 += 4) {
    uint32_t g_lo[4];
    double g_sc[4];
    bool g_ok[4];
#if defined(CM_CHAIN_DIAG)
    bool g_ld[4];
#endif
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int jj = j0 + g;
        g_ok[g] = false;
        g_lo[g] = 0;
        g_sc[g] = (double)kmer;
#if defined(CM_CHAIN_DIAG)
        g_ld[g] = false;
#endif
        if (jj >= h.kc) continue;
        const uint32_t pcn = h.cnt[jj];
        if (pcn == 0) continue;
        CM_L const uint32_t *pp = h.LP + h.base[jj];
        uint32_t lo = 0, hi = pcn;                   // first hit of jj strictly right of this hit
        {
            CD_T0;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((int32_t)pp[mid] <= cur_info) lo = mid + 1;
                else hi = mid;
            }
            CD_ADD(0);
        }
        if (lo >= pcn) continue;
        const uint32_t first = pp[lo];
        if (cur_info + c.P.max_intron < (int32_t)first) continue;       // nothing within maxIntronLen
        g_ok[g] = true;
        g_lo[g] = lo;
        if ((near || first <= own_lim) && ((h.IM[heavy_im_word(h.base[jj], (uint32_t)jj) + (lo >> 5)] >> (lo & 31)) & 1u)) {
            g_sc[g] = h.dps[h.base[jj] + lo];
#if defined(CM_CHAIN_DIAG)
            g_ld[g] = true;
#endif
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (!g_ok[g]) continue;
        const int jj = j0 + g;
        const uint32_t pcn = h.cnt[jj];
        CM_L const uint32_t *pp = h.LP + h.base[jj];
        CM_L const uint32_t *im = h.IM + heavy_im_word(h.base[jj], (uint32_t)jj);
        const uint32_t lo = g_lo[g];
#if defined(CM_CHAIN_DIAG)
        bool g_used = false;
#endif
        if (max_lpos_lim == cmc::MAXUB) {           // cmc::upper_bound with its bit test hoisted (see `near`)
            CD_T0;
            if (near) {
                max_lpos_lim = parked.x;
                max_exon_end = parked.y;
                ol = parked_ol;
            } else {
                max_exon_end = 0;
                ol = -1;
                max_lpos_lim = seg_start + read_remain + (uint32_t)c.P.max_ed;
            }
            CD_ADD(1);
        }
        const int distr = (jj - ii) * kmer - kmer;
        CD_T0;
        for (uint32_t j = lo; j < pcn && pp[j] <= max_lpos_lim; ++j) {
#if defined(CM_CHAIN_DIAG)
            if (!ev) h.tk[4] += 1;
#endif
            const uint32_t pinfo = pp[j];
            int genome_dist, distt, trans_dist;
            if (max_exon_end == 0 || (pinfo + kmer - 1) <= max_exon_end) genome_dist = (int)(pinfo - seg_end - 1);
            else genome_dist = cmc::INF_I;
            if (cmc::cabs(genome_dist - distr) <= c.P.max_ed) distt = genome_dist;
            else if (cmc::check_junction(c, seg_start, pinfo, ol, kmer, distr, trans_dist)) distt = trans_dist;
            else continue;
            const int maxd = distr < distt ? distt : distr, mind = distr < distt ? distr : distt;
            const double beta = 0.1 * (double)(maxd - mind);
            const double alpha = 2e4 * (double)kmer;
            const double prev_score = j == lo ? g_sc[g] : ((im[j >> 5] >> (j & 31)) & 1u) ? h.dps[h.base[jj] + j] : (double)kmer;
#if defined(CM_CHAIN_DIAG)
            if (j == lo) g_used = true;
#endif
            const double t1 = prev_score + alpha;
            const double temp_score = t1 - beta;
            if (temp_score > my_score) {
                my_score = temp_score;
                my_prev = (int32_t)(((uint32_t)jj << 16) | j);
                if (ev) {
                    ev[n].score = temp_score;
                    ev[n].cell = ((uint32_t)ii << 16) | i;
                }
                e1 = n == 1 ? temp_score : e1;         // the first two improvements are handed back: most cells have no more,
                e0 = n == 0 ? temp_score : e0;         // and the caller then skips the second (storing) evaluation
                ++n;
            }
        }
        CD_ADD(2);
#if defined(CM_CHAIN_DIAG)
        if (!ev && g_ld[g]) h.tk[g_used ? 5 : 6] += 1;
#endif
    }
    }
    out_score = my_score;
    out_prev = my_prev;
    return n;
}

// back-tracking state of one heavy problem (LDS): the candidates of the current score, their chains as (cell, slot) lists, the
// non-first fragments of every chain emitted so far (the reference's `repeats` set, src/chain.cpp:248,274-276)
struct HeavyBackTrack {
    uint32_t base[cmc::MAX_SEEDS + 1];
    uint32_t cand[CM_BESTCHAINLIM + 2];
    uint16_t cidx[CM_BESTCHAINLIM][CM_MAX_CHAIN_FRAGS];
    uint8_t cbl[CM_BESTCHAINLIM][CM_MAX_CHAIN_FRAGS];
    uint8_t clen[CM_BESTCHAINLIM + 2];
    uint8_t emit[CM_BESTCHAINLIM + 2];
    uint32_t rep[CM_BESTCHAINLIM * (CM_MAX_CHAIN_FRAGS - 1)];
};

#ifndef CM_CHEAVY_WAVES
#define CM_CHEAVY_WAVES 3      // waves per SIMD k_chain_heavy is compiled for (144 VGPRs as it stands)
#endif
__global__ void __launch_bounds__(64, CM_CHEAVY_WAVES) k_chain_heavy(KCore kc_, ReadsDev rd, uint64_t pair0, int S, const uint32_t *sstart, const uint32_t *scnt,
                                                    const unsigned long long *celloff, double *dp_score, int32_t *dp_prev, uint8_t *pool,
                                                    unsigned long long pool_bytes, unsigned long long *pool_cursor, cm_chain *chains, int32_t *nchain,
                                                    int *err, uint16_t *resid, const uint32_t *perm, const unsigned int *n_perm, unsigned int *next_problem,
                                                    unsigned long long *counters) {
    extern __shared__ uint32_t lds_words[];
    CM_L uint32_t *LP = (CM_L uint32_t *)lds_words;
    __shared__ HeavyBackTrack BT;
    const int lane = threadIdx.x;
    const Core c = cmc::to_core(kc_);
    const int kmer = c.P.kmer;
    const uint32_t max_best = (uint32_t)c.P.max_chain_len;
    const unsigned int n_heavy = *n_perm;
    // the list starts with the heaviest class; a wave takes the next problem from a shared cursor when it is done with its last
    // A problem's header (its index in the list, perm[], then seed ranges, cell offset and read length: three round trips in a
    // row) depends on nothing the previous problem computes, so it is asked for during that problem: the index at its top, perm[]
    // before its DP, the rest at the start of its back-tracking.  Seed ranges ride one per lane (lane s: seed s) and are read back
    // lane by lane at the next turn, which makes the header wave-uniform.  Every wave ends on one index beyond the list, as before.
    auto take_raw = [&]() { return lane == 0 ? atomicAdd(next_problem, 1u) : 0u; };
    uint32_t nx_r = 0, nx_st = 0, nx_cn = 0;
    unsigned long long nx_coff = 0, nx_o0 = 0, nx_o1 = 0;
    auto ask_header = [&](uint32_t rr) {
        nx_st = lane < S ? sstart[(uint64_t)rr * S + lane] : 0u;
        nx_cn = lane < S ? scnt[(uint64_t)rr * S + lane] : 0u;
        nx_coff = celloff[rr];
        const uint64_t pp = pair0 + (rr >> 2);
        const uint64_t *of = ((rr >> 1) & 1u) ? rd.off2 : rd.off1;
        nx_o0 = of[pp];
        nx_o1 = of[pp + 1];
    };
    unsigned int hidx = (unsigned int)__builtin_amdgcn_readfirstlane((int)take_raw());
    if (hidx < n_heavy) {
        nx_r = perm[hidx];
        ask_header(nx_r);
    }
    while (hidx < n_heavy) {
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)nx_r);
        const unsigned int nx_raw = take_raw();
        const int len = __builtin_amdgcn_readfirstlane((int)(nx_o1 - nx_o0));
        const unsigned long long coff = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(nx_coff >> 32)) << 32) |
                                        (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)nx_coff);
#if defined(CM_CHAIN_DIAG)      // wave time per phase (100 MHz ticks) into counters[CN_CD_PHASE ..]: load + init, DP, back-tracking
        const unsigned long long dg0 = wall_clock64();
#endif
        uint32_t st[cmc::MAX_SEEDS], cn[cmc::MAX_SEEDS], base[cmc::MAX_SEEDS + 1];
        int kc = S;
#pragma unroll
        for (int s = 0; s < cmc::MAX_SEEDS; ++s) {         // (lanes from S on hold zeros)
            st[s] = (uint32_t)__builtin_amdgcn_readlane((int)nx_st, s);
            cn[s] = (uint32_t)__builtin_amdgcn_readlane((int)nx_cn, s);
        }
        while (kc >= 1 && cn[kc - 1] == 0) --kc;
        base[0] = 0;
        for (int s = 0; s < kc; ++s) base[s + 1] = base[s] + cn[s];
        const uint32_t ncell = base[kc];
        CM_G double *dps = (CM_G double *)(dp_score + coff);
        CM_G int32_t *dpp = (CM_G int32_t *)(dp_prev + coff);
        // hit positions -> LDS.  The cells are not initialised: a cell is written to HBM when an evaluation improves it, and its bit
        // in IM says so; every reader takes the initial value (score kmer, no back pointer) of a cell whose bit is clear from there.
        CM_L uint32_t *NB = LP + ncell;
        CM_L uint16_t *Q = (CM_L uint16_t *)(NB + 2 * ((ncell + 63) >> 6));
        CM_L uint32_t *IM = (CM_L uint32_t *)(Q + 320);
        // Where the slot has the near-border bits by index entry (Slot::entry_near), the bit of a hit comes with its position: the
        // hits of a seed are consecutive entries, so a list's bits are a few words of one sector, read beside the positions (no
        // further round trip); they ride in bit 31 of the position until the pre-pass below moves them into NB.  The position
        // bitset would cost a sector and a dependent load per hit: a list's positions are copies of a repeat all over the contig.
        const bool by_entry = c.entry_near != nullptr;
        for (int s = 0; s < kc; ++s)
            for (uint32_t i = lane; i < cn[s]; i += 64) {
                const uint32_t e = st[s] + i;
                uint32_t v = c.X.pos[e];
                if (by_entry && s < kc - 1) v |= (uint32_t)((c.entry_near[e >> 6] >> (e & 63)) & 1ull) << 31;
                LP[base[s] + i] = v;
            }
        for (uint32_t x = lane; x < heavy_im_words(ncell, (uint32_t)kc); x += 64) IM[x] = 0u;
        __threadfence_block();
        __syncthreads();
        // cmc::upper_bound of every hit the DP will evaluate (slots 0 .. kc - 2), ahead of the DP.  One hit in seven lies near an exon
        // border (60 k genes) and needs the annotation look-up, four or five dependent loads; inside the DP every batch of 64 cells
        // waited for its few such lanes (51 % of the DP's lane time, DESIGN note 30).  Here the near-border bits of all hits are read
        // first (one load each, every lane busy; they stay in LDS as a bitmask), the near hits are queued, and the look-ups run 64 to
        // a batch; the results are parked in the cells' own score / back-pointer slots (see heavy_cell).
        // (With Slot::entry_near the bits are in LDS already, see above: the first step is a read of LP.)
        {
            const uint32_t n_pre = kc >= 1 ? base[kc - 1] : 0u;
            const unsigned long long lt = (1ull << lane) - 1ull;
            uint32_t qn = 0;
            auto look_up = [&](uint32_t cnt) {
                if ((uint32_t)lane < cnt) {
                    const uint32_t x = Q[lane];
                    int ii = 0;
                    for (int s = 1; s < kc; ++s) ii += x >= base[s] ? 1 : 0;
                    const uint32_t read_remain = (uint32_t)(len - ii * kmer - kmer);
                    uint32_t mx = 0;
                    int ol = -1;
                    const uint32_t lim = cmc::upper_bound_lookup(c, LP[x], (uint32_t)kmer, read_remain, mx, ol);
                    *(CM_G uint2 *)(dps + x) = make_uint2(lim, mx);
                    dpp[x] = ol;
                }
            };
            for (uint32_t x0 = 0; x0 < n_pre; x0 += 256) {               // four bit reads in flight per lane
                bool nr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t x = x0 + 64 * u + lane;
                    if (by_entry) {
                        nr[u] = x < n_pre && (LP[x] >> 31);
                        if (nr[u]) LP[x] &= 0x7fffffffu;
                    } else nr[u] = x < n_pre && cmc::bit_at(c.A.near_border_bits, c.A.n_bits, LP[x]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t xb = x0 + 64 * u;
                    if (xb >= n_pre) break;
                    const unsigned long long m = __ballot(nr[u]);
                    if (lane == 0) NB[xb >> 5] = (uint32_t)m;
                    if (lane == 32) NB[(xb >> 5) + 1] = (uint32_t)(m >> 32);
                    if (nr[u]) Q[qn + __popcll(m & lt)] = (uint16_t)(xb + lane);
                    qn += (uint32_t)__popcll(m);
                }
                __syncthreads();
                while (qn >= 64) {                                       // (at most 63 + 256 entries queued)
                    look_up(64);
                    uint16_t keep[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) keep[u] = 64u * u + (uint32_t)lane < qn - 64 ? Q[64 + 64 * u + lane] : (uint16_t)0;
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (64u * u + (uint32_t)lane < qn - 64) Q[64 * u + lane] = keep[u];
                    qn -= 64;
                    __syncthreads();
                }
            }
            if (qn) look_up(qn);
        }
        __threadfence_block();
        __syncthreads();
#if defined(CM_CHAIN_DIAG)
        const unsigned long long dg1 = wall_clock64();
#endif
#if defined(CM_CHAIN_DIAG)
        unsigned long long tk[7] = {0, 0, 0, 0, 0, 0, 0};      // ([5], [6]: scores asked for ahead of the window loop, used / unused)
        unsigned long long wv[4] = {0, 0, 0, 0};       // wave time: first evaluation, scan + log growth, store / second evaluation, barrier
        HeavyChainCtx H{tk, &c, LP, NB, IM, base, cn, kc, len, dps, dpp};
#else
        HeavyChainCtx H{&c, LP, NB, IM, base, cn, kc, len, dps, dpp};
#endif
        const unsigned int hnext = (unsigned int)__builtin_amdgcn_readfirstlane((int)nx_raw);
        if (hnext < n_heavy) nx_r = perm[hnext];
        CM_G cmc::Event *ev = nullptr;
        uint32_t n_ev = 0, cap_ev = 0;
        bool lost = false;
        double lane_best = -1.0;      // largest final score of the cells this lane improved: a cell's events rise strictly, so the
                                      // wave's maximum is the best score of the log
        for (int ii = kc - 2; ii >= 0; --ii) {
            for (uint32_t i0 = 0; i0 < cn[ii]; i0 += 64) {
                const uint32_t i = i0 + lane;
                const bool on = i < cn[ii];
                double sc = 0, e0 = 0, e1 = 0;
                int32_t pv = -1;
#if defined(CM_CHAIN_DIAG)
                const unsigned long long w0 = wall_clock64();
#endif
                const uint32_t mine = on ? heavy_cell(H, ii, i, (CM_G cmc::Event *)nullptr, sc, pv, e0, e1) : 0u;
#if defined(CM_CHAIN_DIAG)
                const unsigned long long w1 = wall_clock64();
#endif
                {   // the improved bits of this batch: two whole words of the slot's part of IM (read by the slots below, after the barrier)
                    const unsigned long long m = __ballot(mine > 0u);
                    const uint32_t w = heavy_im_word(base[ii], (uint32_t)ii) + (i0 >> 5);
                    if (lane == 0) IM[w] = (uint32_t)m;
                    if (lane == 32) IM[w + 1] = (uint32_t)(m >> 32);
                }
                uint32_t total;
                const uint32_t off = wave_excl_scan(mine, lane, total);
                if (n_ev + total > cap_ev && !lost) {                 // grow the log (uniform decision)
                    uint32_t ncap = cap_ev ? cap_ev : 256u;
                    while (ncap < n_ev + total) ncap *= 4u;
                    const unsigned long long bytes = (unsigned long long)ncap * sizeof(cmc::Event);
                    unsigned long long o = 0;
                    if (lane == 0) o = atomicAdd(pool_cursor, bytes);
                    o = ((unsigned long long)__shfl((unsigned int)(o >> 32), 0) << 32) | (unsigned long long)__shfl((unsigned int)o, 0);
                    if (o + bytes > pool_bytes) {
                        lost = true;
                        if (lane == 0) atomicOr(err, cmc::ERR_POOL);
                    } else {
                        CM_G cmc::Event *ne = (CM_G cmc::Event *)((CM_G uint8_t *)pool + o);
                        for (uint32_t q = lane; q < n_ev; q += 64) ne[q] = ev[q];
                        ev = ne;
                        cap_ev = ncap;
                    }
                }
                if (on && mine) {               // an unimproved cell is not stored (a parked look-up may stay in it: its bit is clear)
                    if (!lost) {
                        CM_G cmc::Event *dst = ev + n_ev + off;
                        if (mine <= 2) {
                            dst[0].score = e0;
                            dst[0].cell = ((uint32_t)ii << 16) | i;
                            if (mine == 2) {
                                dst[1].score = e1;
                                dst[1].cell = ((uint32_t)ii << 16) | i;
                            }
                        } else heavy_cell(H, ii, i, dst, sc, pv, e0, e1);
                    }
                    dps[base[ii] + i] = sc;
                    dpp[base[ii] + i] = pv;
                    lane_best = sc > lane_best ? sc : lane_best;
                }
                if (!lost) n_ev += total;
#if defined(CM_CHAIN_DIAG)
                const unsigned long long w3 = wall_clock64();
                wv[0] += w1 - w0;
                wv[2] += w3 - w1;
#endif
            }
#if defined(CM_CHAIN_DIAG)
            const unsigned long long w4 = wall_clock64();
#endif
            __threadfence_block();
            __syncthreads();
#if defined(CM_CHAIN_DIAG)
            wv[3] += wall_clock64() - w4;
#endif
        }
#if defined(CM_CHAIN_DIAG)
        for (int k = 0; k < 5; ++k) atomicAdd(&counters[CN_CD_LANE + k], tk[k]);          // lane sums
        atomicAdd(&counters[CN_CD_PRE_USED], tk[5]);
        atomicAdd(&counters[CN_CD_PRE_UNUSED], tk[6]);
        if (lane == 0)
            for (int k = 0; k < 4; ++k) atomicAdd(&counters[CN_CD_WAVE + k], wv[k]);      // wave times
#endif
        // ---- back-tracking (src/chain.cpp:242-298), wave-parallel.  The reference walks the scores downwards; per score it takes
        // the first <= maxChainLen logged cells in insertion order, skips one whose start is a non-first fragment of a chain
        // already emitted (only below the best score), and emits the others until maxChainLen chains are out.  Here, per score:
        // (1) the candidates are picked out of the log with ballots, (2) every candidate's chain is walked by its own lane
        // (dependent loads of the back pointers: 30 walks overlap instead of queueing on lane 0), (3) the skip rule runs over
        // the candidates in order against the emitted fragments kept in LDS, (4) the emitted chains are written by all lanes.
        CM_G cm_chain *out = (CM_G cm_chain *)(chains + (uint64_t)r * CM_BESTCHAINLIM);
        uint32_t best_count = 0;
        int first_q0 = 0, first_qlast = 0;            // of chain 0 (for the residual key below)
        if (lane <= kc) BT.base[lane] = base[lane];   // base[] by a lane-varying slot: from LDS
        __threadfence_block();
        __syncthreads();
#if defined(CM_CHAIN_DIAG)
        const unsigned long long dg2 = wall_clock64();
#endif
        if (hnext < n_heavy) ask_header((uint32_t)__builtin_amdgcn_readfirstlane((int)nx_r));
        // The candidates of every score level are fixed once the log is complete, and a candidate's walk depends on its cell
        // alone: only the skip rule is sequential.  So the log is read once -- a log of up to 64 * CM_CHEAVY_LOG_REGS events
        // into registers (lane l: events l, l + 64, ...), where the levels are then iterated without a load -- and the
        // candidates of successive levels are gathered, in the reference's order, into one batch of up to CM_BESTCHAINLIM, whose
        // chains are walked together; the skip rule and the writes then run over the batch, every candidate under its own score.
        // A batch may end within a level (among its first maxChainLen logged cells): the next one resumes there.  A longer log is
        // read from memory once per level, as before, score and cell in one load.
        if (n_ev > 0) {
            constexpr int LR = CM_CHEAVY_LOG_REGS;
            constexpr uint32_t CAP = CM_BESTCHAINLIM;
            const unsigned long long lt = (1ull << lane) - 1ull;
            double best_score = lane_best;
            for (int o = 32; o >= 1; o >>= 1) {
                const double u = __shfl_xor(best_score, o);
                best_score = u > best_score ? u : best_score;
            }
            const bool in_regs = n_ev <= 64u * (uint32_t)LR;
            const int n_u = (int)((n_ev + 63u) >> 6);
            double es[LR];                 // (every logged score is above kmer: -1 is "no event")
            uint32_t ec[LR];
#pragma unroll
            for (int u = 0; u < LR; ++u) {
                es[u] = -1.0;
                ec[u] = 0u;
                const uint32_t q = (uint32_t)lane + 64u * (uint32_t)u;
                if (in_regs && q < n_ev) {
                    const cmc::Event e = ev[q];
                    es[u] = e.score;
                    ec[u] = e.cell;
                }
            }
            double cur = best_score;
            bool have = true;
            uint32_t n_rep = 0;
            int lv_u = 0;                        // where the iteration of level `cur` stands: the register it is at, the lanes of
            unsigned long long lv_done = 0;      // that register already taken, the candidates of the level so far
            uint32_t lv_taken = 0;
            double my_cs = 0.0;                  // score of the candidate this lane walks
#if defined(CM_CHAIN_DIAG)
            unsigned long long dg_levels = 0, dg_passes = 0, dg_batches = 0;
#endif
            while (have && best_count < max_best) {
                uint32_t n_c = 0;
#if defined(CM_CHAIN_DIAG)
                ++dg_batches;
#endif
                if (in_regs) {
#if defined(CM_CHAIN_DIAG)
                    if (dg_passes == 0) dg_passes = (unsigned long long)n_u;
#endif
                    while (have && n_c < CAP) {
                        const uint32_t n_c0 = n_c;
#if defined(CM_CHAIN_DIAG)
                        if (lv_u == 0 && lv_taken == 0 && lv_done == 0ull) ++dg_levels;
#endif
#pragma unroll
                        for (int u = 0; u < LR; ++u) {
                            if (u < lv_u || u >= n_u || lv_taken >= max_best || n_c >= CAP) continue;
                            const bool hit = es[u] == cur && !((lv_done >> lane) & 1ull);
                            const unsigned long long m = __ballot(hit);
                            const uint32_t n_m = (uint32_t)__popcll(m);
                            const uint32_t room = max_best - lv_taken < CAP - n_c ? max_best - lv_taken : CAP - n_c;
                            const bool tk = hit && (uint32_t)__popcll(m & lt) < room;
                            if (tk) BT.cand[n_c + (uint32_t)__popcll(m & lt)] = ec[u];
                            if (n_m > room) {            // the level or the batch is full: this register is resumed
                                lv_done |= __ballot(tk);
                                lv_u = u;
                                n_c += room;
                                lv_taken += room;
                            } else {
                                lv_done = 0ull;
                                lv_u = u + 1;
                                n_c += n_m;
                                lv_taken += n_m;
                            }
                        }
                        if ((uint32_t)lane >= n_c0 && (uint32_t)lane < n_c) my_cs = cur;
                        if (lv_taken >= max_best || lv_u >= n_u) {       // the level is done: the next lower score
                            double nxt = -1.0;
#pragma unroll
                            for (int u = 0; u < LR; ++u)
                                if (es[u] < cur && es[u] > nxt) nxt = es[u];
                            for (int o = 32; o >= 1; o >>= 1) {
                                const double v = __shfl_xor(nxt, o);
                                nxt = v > nxt ? v : nxt;
                            }
                            have = nxt >= 0.0;
                            cur = nxt;
                            lv_u = 0;
                            lv_done = 0ull;
                            lv_taken = 0;
                        }
                    }
                } else {
#if defined(CM_CHAIN_DIAG)
                    ++dg_levels;
                    dg_passes += (unsigned long long)n_u;
#endif
                    double nxt = -1.0;
                    for (uint32_t q0 = 0; q0 < n_ev; q0 += 64) {
                        const uint32_t q = q0 + lane;
                        cmc::Event e;
                        e.score = -1.0;
                        e.cell = 0u;
                        if (q < n_ev) e = ev[q];
                        const bool hit = q < n_ev && e.score == cur;
                        if (q < n_ev && e.score < cur && e.score > nxt) nxt = e.score;
                        const unsigned long long m = __ballot(hit);
                        if (m && n_c < max_best) {
                            const uint32_t rank = n_c + (uint32_t)__popcll(m & lt);
                            if (hit && rank < max_best) BT.cand[rank] = e.cell;
                            n_c += (uint32_t)__popcll(m);
                            if (n_c > max_best) n_c = max_best;
                        }
                    }
                    for (int o = 32; o >= 1; o >>= 1) {
                        const double v = __shfl_xor(nxt, o);
                        nxt = v > nxt ? v : nxt;
                    }
                    if ((uint32_t)lane < n_c) my_cs = cur;
                    have = nxt >= 0.0;
                    cur = nxt;
                }
                __syncthreads();
                // one lane per candidate walks its chain
                if ((uint32_t)lane < n_c) {
                    const uint32_t cell = BT.cand[lane];
                    uint32_t bl = cell >> 16, bi = cell & 0xffffu, n = 0;
                    while (true) {
                        const uint32_t x = BT.base[bl] + bi;
                        BT.cidx[lane][n] = (uint16_t)x;
                        BT.cbl[lane][n] = (uint8_t)bl;
                        ++n;
                        const bool improved = (IM[heavy_im_word(BT.base[bl], bl) + (bi >> 5)] >> (bi & 31)) & 1u;
                        const int32_t pv = improved ? dpp[x] : -1;
                        if (pv < 0 || n >= (uint32_t)CM_MAX_CHAIN_FRAGS) break;
                        bl = (uint32_t)pv >> 16;
                        bi = (uint32_t)pv & 0xffffu;
                    }
                    BT.clen[lane] = (uint8_t)n;
                }
                __syncthreads();
                // the skip rule, candidates in order
                const uint32_t first = best_count;
                uint32_t n_emit = 0;
                for (uint32_t a = 0; a < n_c && best_count < max_best; ++a) {
                    if (__shfl(my_cs, (int)a) < best_score) {
                        const uint32_t spos = LP[BT.cidx[a][0]];
                        bool mine = false;
                        for (uint32_t x = lane; x < n_rep; x += 64) mine = mine || BT.rep[x] == spos;
                        if (__ballot(mine) != 0ull) continue;
                    }
                    const uint32_t cl = BT.clen[a];
                    if (lane == 0) BT.emit[n_emit] = (uint8_t)a;
                    if ((uint32_t)lane >= 1u && (uint32_t)lane < cl) BT.rep[n_rep + lane - 1] = LP[BT.cidx[a][lane]];
                    if (best_count == 0) {
                        first_q0 = (int)BT.cbl[a][0] * kmer;
                        first_qlast = (int)BT.cbl[a][cl - 1] * kmer;
                    }
                    n_rep += cl - 1;
                    ++n_emit;
                    ++best_count;
                    __syncthreads();
                }
                __syncthreads();
                // write the chains emitted from this batch
                for (uint32_t x = lane; x < n_emit * (uint32_t)CM_MAX_CHAIN_FRAGS; x += 64) {
                    const uint32_t k = x / (uint32_t)CM_MAX_CHAIN_FRAGS, f = x % (uint32_t)CM_MAX_CHAIN_FRAGS;
                    const uint32_t a = BT.emit[k];
                    if (f < BT.clen[a]) {
                        CM_G cm_chain &ch = out[first + k];
                        ch.rpos[f] = LP[BT.cidx[a][f]];
                        ch.qpos[f] = (int32_t)BT.cbl[a][f] * kmer;
                    }
                }
                const double cs = __shfl(my_cs, (uint32_t)lane < n_emit ? (int)BT.emit[lane] : 0);
                if ((uint32_t)lane < n_emit) {
                    CM_G cm_chain &ch = out[first + lane];
                    ch.score = (float)cs;
                    ch.chain_len = BT.clen[BT.emit[lane]];
                }
                __syncthreads();
            }
#if defined(CM_CHAIN_DIAG)      // shape of the back-tracking: events, score levels walked, passes over the log (64 events each)
            if (lane == 0) {
                atomicAdd(&counters[CN_CD_EVENTS], (unsigned long long)n_ev);
                atomicAdd(&counters[CN_CD_LEVELS], dg_levels);
                atomicAdd(&counters[CN_CD_PROBLEMS], 1ull);
                atomicAdd(&counters[CN_CD_PASSES], dg_passes);
                atomicAdd(&counters[CN_CD_CELLS], (unsigned long long)ncell);
                atomicAdd(&counters[CN_CD_REGLOG], in_regs ? 1ull : 0ull);
                atomicAdd(&counters[CN_CD_BATCHES], dg_batches);
            }
#endif
        }
        if (best_count == 0) {          // singletons: no cell was improved, every score is the initial one (lane 0 emits; every lane keeps the count)
            for (int ii = kc - 1; ii >= 0; --ii)
                for (uint32_t i = 0; i < cn[ii]; ++i) {
                    if (best_count >= max_best) break;
                    if (best_count == 0) first_q0 = first_qlast = ii * kmer;
                    if (lane == 0) {
                        CM_G cm_chain &ch = out[best_count];
                        ch.rpos[0] = LP[base[ii] + i];
                        ch.qpos[0] = ii * kmer;
                        ch.score = (float)(double)kmer;
                        ch.chain_len = 1;
                    }
                    ++best_count;
                }
        }
        __threadfence_block();
        __syncthreads();
        if (lane == 0) {
            nchain[r] = (int32_t)best_count;
            int rs = 0;
            if (best_count > 0) rs = pack_resid(first_q0, len - (first_qlast + kmer));
            resid[r] = (uint16_t)rs;
#if defined(CM_CHAIN_DIAG)
            const unsigned long long dg3 = wall_clock64();
            atomicAdd(&counters[CN_CD_PHASE + 0], dg1 - dg0);
            atomicAdd(&counters[CN_CD_PHASE + 1], dg2 - dg1);
            atomicAdd(&counters[CN_CD_PHASE + 2], dg3 - dg2);
#endif
        }
        __syncthreads();
        hidx = hnext;
    }
}

// ---- light / heavy split of the pair stage -------------------------------------------------
// A pair whose chain lists can produce many mate pairs and unpaired-chain extensions (reads from
// repeats: up to 30 x 30 pairs plus 60 full-length extensions) costs 100x the median pair; as one lane
// it would hold its whole wave for milliseconds.  Such pairs are listed by k_classify and mapped a
// few per *wave* by k_pair_heavy (the 64 lanes share the pairing predicates, the mate-pair extensions and
// the unpaired-chain extensions of HG pairs; an owner lane per pair folds the outcomes in the reference's
// order).  Everything else stays one pair per lane in k_pair.
constexpr int HEAVY_COST = 6;             // hg38-like bench, ms per step at 3 / 4 / 5 / 6 / 8 / 12 / 16: 32.1 / 31.3 / 26.5 / 26.6 / 28.0 / 30.1 / 31.7
constexpr int N_BUCKETS = 7;             // residual-length buckets
constexpr int HEAVY_CLS = 15;            // class of the pairs mapped by k_pair_heavy
// class of a pair for the pair stage: -2 inactive, HEAVY_CLS heavy (k_pair_heavy), else
// (genic ? 7 : 0) + bucket of the total residual length of its best chains (bases left to extend).
// genic: some best chain starts inside an annotated exon, i.e. the pair will walk transcripts during extension
// while the others only extend on the genome.  k_pair walks the light pairs class by class so the lanes of a
// wave carry similar work; the classes are a heuristic, results do not depend on them.
// (Measured: a "some residual is inexact" flag as a further key costs as much in k_pair_cls as it saves in k_pair.)
__device__ inline int pair_class(const Core &c, const cm_chain *chains, const uint16_t *resid4, const int32_t *nchain,
                                 const uint8_t *active, uint64_t pair0, uint32_t t, int heavy_cost, int *sub) {
    const uint64_t p = pair0 + t;
    if (sub) *sub = 0;
    if (!active[p]) return -2;
    const int32_t *nc = nchain + 4 * (uint64_t)t;
    const int a = nc[0], b = nc[1], cc = nc[2], d = nc[3];
    // a pair with chains on one mate only is settled without any extension (OEANCH, src/filter.cpp:196-203): never heavy
    if ((a + b) > 0 && (cc + d) > 0 && (a * d + cc * b + a + b + cc + d) > heavy_cost) {
        if (sub) {          // heavy pairs: cost level as the first radix key, so that k_pair_heavy starts with the longest ones
            const int cost = a * d + cc * b + a + b + cc + d;
            const int lv = cost <= 12 ? 0 : cost <= 16 ? 1 : cost <= 24 ? 2 : cost <= 32 ? 3 : cost <= 48 ? 4 : cost <= 64 ? 5 : cost <= 96 ? 6 : cost <= 128 ? 7
                           : cost <= 192 ? 8 : cost <= 256 ? 9 : cost <= 384 ? 10 : cost <= 512 ? 11 : cost <= 768 ? 12 : 13;
            *sub = lv << 4;
        }
        return HEAVY_CLS;
    }
    // chains on one mate only, or on neither: settled from the chain counts (CM_OEANCH, NOPROC_*).  The cheapest light class, and no
    // look into chains[]: the records of an unchained problem (nchain is the marker 1, see ChainRecs) are not there to be read
    if ((a + b) <= 0 || (cc + d) <= 0) return 0;
    const uint16_t *q = resid4 + 4 * (uint64_t)t;
    int resid = 0;
    for (int x = 0; x < 4; ++x) resid += (q[x] & 0xff) + (q[x] >> 8);
    if (sub) {          // which of the four extensions of the main orientation have bases to extend (LL, LR, RL, RR of both_mates)
        const bool main0 = a > 0 && d > 0;                 // forward R1 / backward R2 carries chains, else the other orientation
        const uint16_t f = q[main0 ? 0 : 2], bk = q[main0 ? 3 : 1];
        *sub = ((f & 0xff) ? 1 : 0) | ((f >> 8) ? 2 : 0) | ((bk & 0xff) ? 4 : 0) | ((bk >> 8) ? 8 : 0);
        int mx = f & 0xff;                                  // longest single residual of the main orientation, 16 levels
        mx = (f >> 8) > mx ? (f >> 8) : mx;
        mx = (bk & 0xff) > mx ? (bk & 0xff) : mx;
        mx = (bk >> 8) > mx ? (bk >> 8) : mx;
        const int lv = mx < 5 ? 0 : mx < 10 ? 1 : mx < 15 ? 2 : mx < 20 ? 3 : mx < 25 ? 4 : mx < 30 ? 5 : mx < 40 ? 6 : mx < 50 ? 7 : mx < 60 ? 8 : mx < 70 ? 9
                       : mx < 80 ? 10 : mx < 90 ? 11 : mx < 100 ? 12 : mx < 115 ? 13 : mx < 130 ? 14 : 15;
        *sub |= lv << 4;
    }
    const int bucket = resid < 25 ? 0 : resid < 50 ? 1 : resid < 100 ? 2 : resid < 150 ? 3 : resid < 200 ? 4 : resid < 300 ? 5 : 6;
    bool genic = false;
    for (int x = 0; x < 4 && !genic; ++x) {
        if (nc[x] <= 0) continue;
        genic = cmc::overlap(c, chains[((uint64_t)t * 4 + x) * CM_BESTCHAINLIM].rpos[0]) >= 0;
    }
    return (genic ? N_BUCKETS : 0) + bucket;
}
// Atomic-free counting sort of the tile's pairs by class (bucket 0..7, heavy = class 8):
// k_cls_count: class per pair + per-block class histogram;  k_cls_scan: one workgroup turns the
// [class][block] histogram into exclusive bases (heaviest light bucket first) and totals;
// k_cls_place: writes perm[] (light pairs) / hlist[] (heavy pairs) at base + rank inside the block.
constexpr int CHAIN_LIGHT_CLS = 12;     // chaining classes below this are light
constexpr int CLS_T = 1024;            // elements per block of the counting sorts
constexpr int CLS_W = 256;             // threads per block: every wave takes CLS_T / CLS_W stretches of 64 elements in turn (blocks of 1024 threads waited up
                                       // to 1.4 ms for sixteen free wave slots on one CU next to the seeding kernel)
constexpr int CLS_REP = CLS_T / CLS_W;
constexpr int N_CLS = 16;                // classes a sort can use (pairs: 0..13 light + 15 heavy; chaining: 0..11 light + 12..15 heavy)
constexpr int CTR_SUM = 16, CTR_BASE = 32, CTR_WORDS = 64;
constexpr int CTR_NEXT = 48;             // spare words of the pair stage's class counters: work cursors of k_pair / k_pair_heavy, then the
constexpr int CTR_RETRY = 50;            // re-run list's length and the re-run launch's cursor (RetryArgs)
constexpr int CTR_CHAIN_NEXT = 48;       // spare word of the CHAIN stage's class counters (SeedSet::cctr, its own array): work cursor of k_chain_heavy
static_assert(CTR_CHAIN_NEXT >= CTR_BASE + N_CLS && CTR_CHAIN_NEXT < CTR_WORDS && CTR_NEXT >= CTR_BASE + N_CLS && CTR_RETRY + 1 < CTR_WORDS, "spare words");
constexpr unsigned HEAVY_GRID_MAX = 4096;   // d_hres holds the task outcomes + scratch of this many k_pair_heavy blocks
constexpr int RETRY_GRID = 8;            // blocks of the re-run launch of k_pair (pairs beyond the first pass's capacity: a handful per run, if any)
constexpr int RETRY_SPILL = 2040;        // + MEMO_N in registers: 2048 memoised exon pieces per extend call
__device__ inline void block_class_ranks(int k, unsigned int (*wcnt)[N_CLS], unsigned int &rank_in_wave, int lane, int wave) {
    // wcnt[w][c] = number of lanes of wave w with class c; rank_in_wave = rank of this lane among its class in its wave
    rank_in_wave = 0;
#pragma unroll
    for (int c = 0; c < N_CLS; ++c) {
        const unsigned long long m = __ballot(k == c);
        if (lane == 0) wcnt[wave][c] = (unsigned int)__popcll(m);
        if (k == c) rank_in_wave = (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
    }
}
// Where the light / heavy line of the pair stage goes depends on how much heavy work a tile holds.  The two pair kernels run side
// by side and the stage ends with the later one.  With little heavy work (chr21, the round-2 genome: a few percent of the pairs
// come from repeats) the heavy kernel is done long before the light one, and every multi-chain pair is best taken off the light
// kernel's waves (threshold 6: 95 vs 57 M pairs/s on chr21 against 48).  On the section-8(d) genome a sixth of the pairs are heavy,
// most of them with 30 x 30 chain pairs; the heavy kernel is the long pole and the light kernel has slack.  With one pair per wave
// in the heavy kernel the mid-cost pairs (7 .. 48) were best left to the light kernel (threshold 48: 16.7 vs 15.0 M pairs/s);
// with several pairs per wave (HG) the heavy kernel is the more efficient place for a pair with a dozen chain pairs, and the
// wide threshold is 16 (92.1 ms per step against 95.5 at 48 and 92.7 at 6).
// k_pair_cost adds up the cost beyond HEAVY_COST over the tile; k_pair_cls takes the wide threshold when that sum exceeds
// HEAVY_LOAD per pair of the tile.  Results never depend on the split.
constexpr int HEAVY_COST_WIDE = 16;
constexpr unsigned long long HEAVY_LOAD = 16;
__global__ void __launch_bounds__(BLK) k_pair_cost(const int32_t *nchain, const uint8_t *active, uint64_t pair0, uint32_t n_tile, int base_cost,
                                                  unsigned long long *sum) {
    __shared__ unsigned long long sh[BLK / 64];
    const uint32_t t = blockIdx.x * BLK + threadIdx.x;
    unsigned long long v = 0;
    if (t < n_tile && active[pair0 + t]) {
        const int32_t *nc = nchain + 4 * (uint64_t)t;
        const int a = nc[0], b = nc[1], cc = nc[2], d = nc[3];
        const int cost = a * d + cc * b + a + b + cc + d;
        if ((a + b) > 0 && (cc + d) > 0 && cost > base_cost) v = (unsigned long long)cost;
    }
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s2 = 0;
        for (int w = 0; w < BLK / 64; ++w) s2 += sh[w];
        if (s2) atomicAdd(sum, s2);
    }
}
__global__ void __launch_bounds__(BLK) k_pair_cls(KCore kc, const cm_chain *chains, const uint16_t *resid, const int32_t *nchain,
                                                 const uint8_t *active, uint64_t pair0, uint32_t n_tile, int8_t *cls, int32_t *cat, int heavy_cost,
                                                 int8_t *cls_sub, int8_t *cls_sub2, uint8_t *act_out, const unsigned long long *heavy_load) {
    const uint32_t t = blockIdx.x * BLK + threadIdx.x;
    if (t >= n_tile) return;
    const Core c = cmc::to_core(kc);
    if (heavy_load && *heavy_load > HEAVY_LOAD * (unsigned long long)n_tile) heavy_cost = HEAVY_COST_WIDE;
    int sub = 0;
    const int k = pair_class(c, chains, resid, nchain, active, pair0, t, heavy_cost, &sub);
    cls[t] = (int8_t)k;
    cls_sub[t] = (int8_t)(k < 0 ? -2 : (k == HEAVY_CLS ? 0 : (sub & 15)));    // secondary key
    cls_sub2[t] = (int8_t)(k < 0 ? -2 : (sub >> 4));                           // tertiary key (first pass of the radix sort)
    if (k == -2) {                                     // retired in an earlier round: not mapped, stays retired
        cat[pair0 + t] = -1;
        act_out[pair0 + t] = 0;
    }
}
// work class of one chaining problem: number of (hit, later hit) pairs the DP may have to examine
// skip_dead: a dead problem (quad_dead) gets the class CHAIN_CLS_DEAD, which no kernel visits, and what the pair stage reads of it:
// nchain = 1 (the marker "has hits, not chained", see ChainRecs), resid = 0, and chain_len = 0 in its first chain record, so that
// a record left from an earlier item cannot pass for a chain.  counters[CN_DEAD_CHAINS] counts them.
__global__ void __launch_bounds__(BLK) k_chain_cls(const uint32_t *scnt, const uint32_t *sraw, int S, uint32_t n_prob, int8_t *cls, int32_t *high,
                                                  unsigned long long light_w, unsigned int light_cells, int32_t *nchain, uint16_t *resid,
                                                  cm_chain *chains, const uint8_t *active, uint64_t pair0, int skip_dead,
                                                  unsigned long long *counters) {
    __shared__ unsigned int n_dead;
    const uint32_t r = blockIdx.x * BLK + threadIdx.x;
    if (threadIdx.x == 0) n_dead = 0;
    __syncthreads();
    // nchain == null: the chain records are still being read by an earlier pair stage; `high` is a scratch array of the seed set and
    // k_chain_apply carries the fields over when the records are free (the class -2 stands for "no chain, no kernel visits it")
    const bool on = r < n_prob && active[pair0 + (r >> 2)];
    if (r < n_prob && !on) {            // seeded under older flags (a superset), retired since: no chains wanted
        high[r] = 0;
        if (nchain) {
            nchain[r] = 0;
            resid[r] = 0;
        }
        cls[r] = CHAIN_CLS_NONE;
    }
    unsigned long long w = 0, suffix = 0;
    int hh = 0;
    if (on)
        for (int s = S - 1; s >= 0; --s) {
            const unsigned long long c = scnt[(uint64_t)r * S + s];
            w += c * suffix;
            suffix += c;
            if (sraw[(uint64_t)r * S + s] > 0 && c == 0) ++hh;       // get_best_chains high_hits (also for problems k_chain skips)
        }
    // (n_prob is a multiple of 4 and the four problems of a pair share its flag: a quad is on or off as a whole; off counts no cell)
    const bool dead = skip_dead && quad_dead((uint32_t)suffix);
    if (skip_dead) {                    // the count: one add per wave in LDS, one per workgroup in memory
        const unsigned long long md = __ballot(dead);
        if ((threadIdx.x & 63) == 0 && md) atomicAdd(&n_dead, (unsigned int)__popcll(md));
        __syncthreads();
        if (threadIdx.x == 0 && n_dead) atomicAdd(&counters[CN_DEAD_CHAINS], (unsigned long long)n_dead);
    }
    if (!on) return;
    high[r] = hh;
    if ((suffix == 0 || dead) && nchain) {        // no retained hit: no chain; dead: the marker.  No kernel visits either.
        nchain[r] = dead ? 1 : 0;
        resid[r] = 0;
        if (dead) chains[(uint64_t)r * CM_BESTCHAINLIM].chain_len = 0;
    }
    // classes 0..11 = light (one lane each, k_chain; grouped so the lanes of a wave carry similar DPs),
    // 12..15 = heavy (one wave each, k_chain_heavy, heaviest class first)
    const bool light = w <= light_w && suffix <= light_cells;
    const unsigned int n = (unsigned int)suffix;
    cls[r] = (int8_t)(suffix == 0 ? CHAIN_CLS_NONE
                      : dead ? CHAIN_CLS_DEAD
                      : light ? (n <= 3 ? 0 : n <= 6 ? 1 : n <= 7 ? 2 : n <= 9 ? 3 : n <= 12 ? 4 : n <= 16 ? 5 : n <= 24 ? 6 : n <= 32 ? 7 : n <= 48 ? 8 : n <= 64 ? 9
                                 : n <= 96 ? 10 : 11)
                      : w <= 4096 ? 12 : w <= 65536 ? 13 : w <= 1048576 ? 14 : 15);
}
__global__ void __launch_bounds__(BLK) k_chain_apply(uint32_t n_prob, const int8_t *cls, const int32_t *thigh, int32_t *high, int32_t *nchain, uint16_t *resid,
                                                    cm_chain *chains) {
    const uint32_t r = blockIdx.x * BLK + threadIdx.x;
    if (r >= n_prob) return;
    high[r] = thigh[r];
    const int k = cls[r];
    if (k == CHAIN_CLS_NONE || k == CHAIN_CLS_DEAD) {
        nchain[r] = k == CHAIN_CLS_DEAD ? 1 : 0;
        resid[r] = 0;
        if (k == CHAIN_CLS_DEAD) chains[(uint64_t)r * CM_BESTCHAINLIM].chain_len = 0;
    }
}
// `order` (optional): visit the elements in this order (second pass of an LSD radix sort: order = the permutation of the
// first pass, *n_order entries); the element at position i is order[i]
__global__ void __launch_bounds__(CLS_W) k_cls_hist(const int8_t *cls, uint32_t n, unsigned int *blk_cnt, uint32_t nb, const uint32_t *order,
                                                    const unsigned int *n_order) {
    __shared__ unsigned int wcnt[CLS_T / 64][N_CLS];
    const uint32_t lim = n_order ? (*n_order < n || order ? *n_order : n) : n;      // (without an order: a device-side count, at most n)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a workgroup takes the stretches of CLS_T elements blockIdx.x, blockIdx.x + gridDim.x, ... (one each when the grid has nb
    // workgroups; a smaller grid when the count is only known on the device and most of nb would have nothing to do)
    for (uint32_t vb = blockIdx.x; vb < nb; vb += gridDim.x) {
        if (!order && n_order && vb * (uint32_t)CLS_T >= lim) break;                 // (k_cls_scan is told the same count: nothing to report)
#pragma unroll
        for (int j = 0; j < CLS_REP; ++j) {
            const int vw = wave * CLS_REP + j;                 // stretch of 64 elements within the block
            const uint32_t i = vb * CLS_T + (uint32_t)vw * 64u + (uint32_t)lane;
            const int k = i < lim ? (int)cls[order ? order[i] : i] : -2;
            unsigned int r;
            block_class_ranks(k, wcnt, r, lane, vw);
        }
        __syncthreads();
        if (threadIdx.x < N_CLS) {
            unsigned int tot = 0;
            for (int w = 0; w < CLS_T / 64; ++w) tot += wcnt[w][threadIdx.x];
            blk_cnt[(size_t)threadIdx.x * nb + vb] = tot;
        }
        __syncthreads();
    }
}
// ctr[c] = total of class c, ctr[CTR_SUM] = entries placed in perm[], ctr[CTR_BASE + c] = base offset of class c in perm[]
// (highest class first); the classes in the bit mask `separate` (none: -1) go to their own lists instead
// n_dev (optional): the elements there are, on the device; only the blocks that hold some are scanned (rows keep their stride nb).
// One workgroup of four waves, four class rows each (a 1024-thread workgroup waited 0.1 - 3 ms for sixteen free wave slots on one CU).
constexpr int SCAN_CLS_T = 256;
__global__ void __launch_bounds__(SCAN_CLS_T) k_cls_scan(unsigned int *blk_cnt, uint32_t nb, unsigned int *ctr, int separate, int n_used,
                                                         const unsigned int *n_dev = nullptr) {
    // one wave per class row at a time: 64 block counts per step, exclusive scan inside the wave, running total carried on
    __shared__ unsigned int tot[N_CLS];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    if (t < N_CLS) tot[t] = 0;
    __syncthreads();
    uint32_t nb_eff = nb;
    if (n_dev) {
        const uint32_t used = (uint32_t)(((unsigned long long)*n_dev + CLS_T - 1) / CLS_T);
        nb_eff = used < nb ? used : nb;
    }
    for (int c = wave; c < N_CLS; c += SCAN_CLS_T / 64) {
        if (c >= n_used) break;                          // classes >= n_used are not produced by this caller
        unsigned int *row = blk_cnt + (size_t)c * nb;
        unsigned int run = 0;
        for (uint32_t i0 = 0; i0 < nb_eff; i0 += 64) {
            const uint32_t i = i0 + (uint32_t)lane;
            const unsigned int x = i < nb_eff ? row[i] : 0u;
            unsigned int incl = x;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (i < nb_eff) row[i] = run + incl - x;
            run += __shfl(incl, 63);
        }
        if (lane == 0) tot[c] = run;
    }
    __syncthreads();
    if (t == 0) {
        unsigned int off = 0;
        for (int c = N_CLS - 1; c >= 0; --c) {          // heaviest class first
            if (separate >= 0 && ((separate >> c) & 1)) {      // classes with their own list
                ctr[CTR_BASE + c] = 0;
                continue;
            }
            ctr[CTR_BASE + c] = off;
            off += tot[c];
        }
        ctr[CTR_SUM] = off;
        for (int c = 0; c < N_CLS; ++c) ctr[c] = tot[c];
    }
}
__global__ void __launch_bounds__(CLS_W) k_cls_place(const int8_t *cls, uint32_t n_tile, const unsigned int *blk_base, uint32_t nb,
                                                     const unsigned int *ctr, uint32_t *perm, uint32_t *hlist, const uint32_t *order,
                                                     const unsigned int *n_order) {
    __shared__ unsigned int wcnt[CLS_T / 64][N_CLS];
    const uint32_t lim = n_order ? (*n_order < n_tile || order ? *n_order : n_tile) : n_tile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t vb = blockIdx.x; vb < nb; vb += gridDim.x) {                       // (see k_cls_hist)
        if (!order && n_order && vb * (uint32_t)CLS_T >= lim) break;
        uint32_t t[CLS_REP];
        int k[CLS_REP];
        unsigned int r[CLS_REP];
#pragma unroll
        for (int j = 0; j < CLS_REP; ++j) {
            const int vw = wave * CLS_REP + j;
            const uint32_t i = vb * CLS_T + (uint32_t)vw * 64u + (uint32_t)lane;
            t[j] = i < lim ? (order ? order[i] : i) : 0u;
            k[j] = i < lim ? (int)cls[t[j]] : -2;
            block_class_ranks(k[j], wcnt, r[j], lane, vw);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CLS_REP; ++j) {
            if (k[j] < 0) continue;
            const int vw = wave * CLS_REP + j;
            unsigned int before = 0;
            for (int w = 0; w < vw; ++w) before += wcnt[w][k[j]];
            const unsigned int pos = blk_base[(size_t)k[j] * nb + vb] + before + r[j];
            if (k[j] == HEAVY_CLS && hlist) hlist[pos] = t[j];
            else perm[ctr[CTR_BASE + k[j]] + pos] = t[j];
        }
        __syncthreads();
    }
}

struct HRes {            // outcome of one mate-pair task, handed from the computing lane to the pair's owner lane
    cmc::MM r1, r2;
    int32_t row;
    int32_t pair_type;
    uint8_t ok, is_left, pad[2];
};
// k_pair_heavy maps HG heavy pairs per wave side by side.  A heavy pair has hundreds of pairing-predicate evaluations but few
// accepted mate pairs (section-8(d) genome: 5.5 per process_mates call, tests/diag/heavy_shape.py): one pair per wave left 55 of
// the 64 lanes idle through the extensions, which are four fifths of the kernel (7.9 lanes per VALU instruction, VALU issue
// saturated).  Here every phase of process_mates runs over ONE work list of the whole wave -- chain ends, predicate evaluations,
// accepted mate pairs, unpaired chains of all HG pairs, one item per lane -- and lane g < HG (the "owner" of slot g) keeps pair g's
// MatchedRead and folds its outcomes in the reference's order.  What a lane needs of a pair it reads from the pair's slot in LDS.
#ifndef CM_HEAVY_G
#define CM_HEAVY_G 6            // 4 / 6 / 8 / 16: 89.3 / 85.9 / 89.4 / 96 ms per step on the hg38-like bench (33 tasks per 64-lane batch at 6)
#endif
constexpr int HG = CM_HEAVY_G;
static_assert(HG >= 1 && HG <= 16, "the task list packs the slot in 4 bits");
constexpr int HEAVY_LIST = HG * CM_BESTCHAINLIM * CM_BESTCHAINLIM;      // accepted (i, j) of all slots, worst case
constexpr int HEAVY_SCRATCH = HEAVY_LIST * 2;     // bytes of per-block global scratch behind HRes[64]: the task list (u16)
// One pair in flight (LDS).  Written by its owner lane unless noted.  Packed: LDS is allocated in steps of 1 280 bytes on this part
// and this kernel's request (two staging buffers + six slots: 14 552 bytes = 12 steps) must not grow into the next one -- a 13th
// step costs a resident wave per CU and 6 ms per bench step (NOTES 44).
struct HSlot {
    cmc::g_u8 fseq, bseq;                // the two reads (forward read: as stored; backward read: reverse complement)
    uint32_t fch_i, bch_i;               // chain lists of this attempt (record index into the tile's chain records): forward read's, backward read's
    uint32_t t;                          // the pair (tile-relative): its capacity-limit word is pair_err[t] (RetryArgs)
    unsigned int inv_nb;                 // ceil(65536 / nb): idx / nb = idx * inv_nb >> 16 for idx < 900
    unsigned int fp, bp;                 // chains that found a mate (atomicOr by the predicate lanes)
    int ntask;                           // accepted mate pairs (atomicAdd by the predicate lanes)
    unsigned int fun, bun;               // unpaired chains to extend
    int exf, exb;                        // outcome of the unpaired-chain extensions (atomicMin)
    int16_t flen, blen;
    int16_t nf, nb;                      // chains; 0 / 0 while the slot sits an attempt out
    int16_t nfu, nbu;
    int8_t saved_type;                   // MatchedRead.type at the start of the attempt (pairing predicate)
    int8_t done;                         // the fold returned CONCRD: the slot's remaining tasks are dead
    int8_t gf, gb;                       // genic flag of each side's first unpaired chain (written by the k == 0 lane)
    int fe[CM_BESTCHAINLIM], re[CM_BESTCHAINLIM];                        // exon interval of each chain's first fragment (written by the chain-end lanes)
    uint32_t r0[2 * CM_BESTCHAINLIM], rend[2 * CM_BESTCHAINLIM];         // reference span of the chains: forward, then (from CM_BESTCHAINLIM) backward
};
__device__ inline cmc::g_chain slot_fch(CM_L const HSlot &s, const cm_chain *base) { return (cmc::g_chain)(base + s.fch_i); }
__device__ inline cmc::g_chain slot_bch(CM_L const HSlot &s, const cm_chain *base) { return (cmc::g_chain)(base + s.bch_i); }
__device__ inline cmc::g_err slot_perr(CM_L const HSlot &s, uint32_t *pair_err) { return (cmc::g_err)(pair_err + s.t); }
static_assert(sizeof(HSlot) <= 808, "six slots + two staging buffers of 72-byte rows fit 11 LDS allocation steps");

__device__ inline int nth_set_bit(uint32_t m, int k) {
    for (int x = 0; x < k; ++x) m &= m - 1;
    return __ffs((int)m) - 1;
}
// item x of a work list that concatenates the slots' items: pre[g] = items before slot g's, pre[HG] = all
__device__ inline void locate(const int (&pre)[HG + 1], int x, int &g, int &k) {
    g = 0;
    int b = 0;
#pragma unroll
    for (int s = 1; s < HG; ++s) {
        const bool ge = x >= pre[s];
        g += ge ? 1 : 0;
        b = ge ? pre[s] : b;
    }
    k = x - b;
}

#ifndef CM_HEAVY_WAVES
#define CM_HEAVY_WAVES CM_PAIR_WAVES
#endif
// process_read (src/filter.cpp:124-241) + process_mates (src/filter.cpp:244-395) for HG pairs per wave iteration.
__global__ void __launch_bounds__(BLK_PAIR, CM_HEAVY_WAVES) k_pair_heavy(KCore kc, ReadsDev rd, uint64_t pair0, const uint32_t *hlist, const unsigned int *hcount,
                                                         const cm_chain *chains, const int32_t *nchain, const int32_t *high, cm_mapped_read *state,
                                                         uint8_t *active, int32_t *cat, int is_last, int *err, unsigned long long *counters,
                                                         int str_cap, unsigned long long *dbg_rows, HRes *hres, unsigned int *next_pair,
                                                         RetryArgs ra) {
    extern __shared__ uint32_t lds_words[];
    const int lane = threadIdx.x;
    CM_L uint8_t *base = (CM_L uint8_t *)lds_words;
    const int lds_stage_bytes = 2 * lbuf_bytes(str_cap) * BLK_PAIR;
#if defined(CM_DIAG)
    __shared__ unsigned long long tick_w[65];
    cmc::Tick tick{};
    tick.w = (CM_L unsigned long long *)tick_w;
    tick.wave_on = 1;
    tick.last = wall_clock64();
    for (int i = threadIdx.x; i < 65; i += BLK_PAIR) tick_w[i] = i == 0 ? tick.last : 0ull;
    __syncthreads();
    cmc::DpMem sm = lane_dp_mem(base, lane, str_cap, (cmc::g_err)err, &tick);
#else
    cmc::DpMem sm = lane_dp_mem(base, lane, str_cap, (cmc::g_err)err);
#endif
    CM_L HSlot *S = (CM_L HSlot *)(base + lds_stage_bytes);
    CM_G HRes *res = (CM_G HRes *)(hres + (size_t)blockIdx.x * 64);
    CM_G uint16_t *list = (CM_G uint16_t *)((CM_G uint8_t *)(hres + (size_t)gridDim.x * 64) + (size_t)blockIdx.x * HEAVY_SCRATCH);
    const Core c = cmc::to_core(kc);
    const cmc::Ext ext(c, sm);
    const int kmer = c.P.kmer;
    const unsigned int n_heavy = *hcount;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t tids[cmc::MAX_TID];
    // HG pairs at a time from a shared cursor (the list starts with the most expensive pairs; neighbours cost about the same)
    auto take = [&]() { return (unsigned int)__shfl((int)(lane == 0 ? atomicAdd(next_pair, (unsigned int)HG) : 0u), 0); };
    for (unsigned int h0 = take(); h0 < n_heavy; h0 = take()) {
        // ---- owners: lane g holds pair h0 + g -------------------------------------------------------------------------
        const bool owner = lane < HG && h0 + (unsigned int)lane < n_heavy;
        uint32_t t = 0;
        uint64_t p = 0;
        int len1 = 0, len2 = 0, st = -1;
        cmc::ChainSet sets[4];
        cmc::g_u8 s1 = nullptr, s2 = nullptr;
        cm_mapped_read mr{};
        bool first = true;
        for (int x = 0; x < 4; ++x) { sets[x].ch = nullptr; sets[x].n = 0; }
        if (owner) {
            t = hlist[h0 + lane];
            p = pair0 + t;
            const uint64_t a0 = rd.off1[p], a1 = rd.off1[p + 1], b0 = rd.off2[p], b1 = rd.off2[p + 1];
            len1 = (int)(a1 - a0);
            len2 = (int)(b1 - b0);
            s1 = (cmc::g_u8)(rd.seq1 + a0);
            s2 = (cmc::g_u8)(rd.seq2 + b0);
            int hh[4];
            for (int x = 0; x < 4; ++x) {
                const uint64_t r = (uint64_t)t * 4 + x;
                sets[x].ch = (cmc::g_chain)(chains + r * CM_BESTCHAINLIM);
                sets[x].n = nchain[r];
                hh[x] = high[r];
            }
            mr = state[p];
            const int n1 = sets[0].n + sets[1].n, n2 = sets[2].n + sets[3].n;
            if (n1 + n2 <= 0) {             // unreachable for a pair classified heavy; kept for completeness
                st = ((hh[0] + hh[1] > 0) && (hh[2] + hh[3] > 0)) ? CM_NOPROC_MANYHIT : CM_NOPROC_NOMATCH;
                cmc::mr_update_type(mr, st);
            } else if (n1 <= 0 || n2 <= 0) {
                st = CM_OEANCH;
                cmc::mr_update_type(mr, st);
            } else {
                const float fc1 = sets[0].n > 0 ? sets[0].ch[0].score : 0.f, bc1 = sets[1].n > 0 ? sets[1].ch[0].score : 0.f;
                const float fc2 = sets[2].n > 0 ? sets[2].ch[0].score : 0.f, bc2 = sets[3].n > 0 ? sets[3].ch[0].score : 0.f;
                first = (fc1 + bc2) >= (fc2 + bc1);
            }
        }
        for (int attempt = 0; attempt < 2; ++attempt) {
            // ---- owners publish the attempt of their pair (process_read's loop: forward R1 / backward R2, or the other way) ----
            const bool on = owner && st < 0;
            const bool r1_fwd = (attempt == 0) == first;
            if (lane < HG) {
                CM_L HSlot &s = S[lane];
                const cmc::ChainSet &F = r1_fwd ? sets[0] : sets[2], &B = r1_fwd ? sets[3] : sets[1];
                s.fch_i = (uint32_t)(F.ch ? F.ch - (cmc::g_chain)chains : 0);
                s.bch_i = (uint32_t)(B.ch ? B.ch - (cmc::g_chain)chains : 0);
                s.fseq = r1_fwd ? s1 : s2;
                s.bseq = r1_fwd ? s2 : s1;
                s.flen = (int16_t)(r1_fwd ? len1 : len2);
                s.blen = (int16_t)(r1_fwd ? len2 : len1);
                s.t = t;
                s.nf = (int16_t)(on ? F.n : 0);
                s.nb = (int16_t)(on ? B.n : 0);
                s.inv_nb = (on && B.n > 0) ? (65536u + (unsigned int)B.n - 1u) / (unsigned int)B.n : 0u;
                s.saved_type = (int8_t)mr.type;
                s.fp = 0u;
                s.bp = 0u;
                s.ntask = 0;
                s.done = 0;
                s.nfu = 0;
                s.nbu = 0;
            }
            if (__ballot(on) == 0ull) break;                   // uniform: every pair of this iteration is settled
            __syncthreads();
            int pre[HG + 1];
            // ---- chain ends: reference span + exon interval of the first fragment, one chain per lane -------------------------
            pre[0] = 0;
#pragma unroll
            for (int g = 0; g < HG; ++g) pre[g + 1] = pre[g] + S[g].nf + S[g].nb;
            for (int x = lane; x < pre[HG]; x += 64) {
                int g, k;
                locate(pre, x, g, k);
                CM_L HSlot &s = S[g];
                const int nf = s.nf;
                const bool back = k >= nf;
                const int ci = back ? k - nf : k;
                const cmc::CHEnds e{(back ? slot_bch(s, chains) : slot_fch(s, chains)) + ci, kmer};
                s.r0[(back ? CM_BESTCHAINLIM : 0) + ci] = e.r0;
                s.rend[(back ? CM_BESTCHAINLIM : 0) + ci] = e.rend;
                (back ? s.re : s.fe)[ci] = cmc::overlap(c, e.r0);
            }
            __syncthreads();
            // ---- pairing predicate of every (i, j) of every slot; the accepted ones go to the task list in (slot, i, j) order ----
            pre[0] = 0;
#pragma unroll
            for (int g = 0; g < HG; ++g) pre[g + 1] = pre[g] + S[g].nf * S[g].nb;
            int n_task = 0;
            for (int b0 = 0; b0 < pre[HG]; b0 += 64) {
                const int x = b0 + lane;
                uint32_t code = 0;
                int g = 0, idx = 0;
                if (x < pre[HG]) {
                    locate(pre, x, g, idx);
                    CM_L HSlot &s = S[g];
                    const int i = (int)(((unsigned int)idx * s.inv_nb) >> 16), j = idx - i * s.nb;
                    const cmc::CHEnds F{s.r0[i], s.rend[i]}, R{s.r0[CM_BESTCHAINLIM + j], s.rend[CM_BESTCHAINLIM + j]};
                    code = cmc::pair_code(c, F, R, s.fe[i], s.re[j], s.saved_type);
                    if (code) {
                        atomicOr((unsigned int *)&s.fp, 1u << i);
                        atomicOr((unsigned int *)&s.bp, 1u << j);
                        atomicAdd((int *)&s.ntask, 1);
                    }
                }
                const unsigned long long m = __ballot(code != 0);
                if (code) list[n_task + __popcll(m & lt_mask)] = (uint16_t)((unsigned int)idx | (code << 10) | ((unsigned int)g << 12));
                n_task += __popcll(m);
            }
            __syncthreads();
            CM_TICK(sm, 29);
            // ---- mate-pair tasks: one per lane, 64 at a time; each owner folds its slot's outcomes in order --------------------
            int t_lo = 0, t_hi = 0;                                     // the owner's slice of the task list
            if (lane < HG) {
                for (int g = 0; g < HG; ++g) t_lo += g < lane ? S[g].ntask : 0;
                t_hi = t_lo + S[lane].ntask;
            }
            int min_ret1 = CM_ORPHAN, min_ret2 = CM_ORPHAN, g1 = 0, g2 = 0;          // meaningful on the owners
            bool early = false;
            for (int b0 = 0; b0 < n_task; b0 += 64) {
                const int x = b0 + lane;
                if (x < n_task) {
                    const unsigned int e = list[x];
                    CM_L HSlot &s = S[e >> 12];
                    if (!s.done) {
                        const uint32_t code = (e >> 10) & 3u;
                        const int idx = (int)(e & 1023u);
                        const int i = (int)(((unsigned int)idx * s.inv_nb) >> 16), j = idx - i * s.nb;
                        sm.err = slot_perr(s, ra.pair_err);
                        const cmc::TidList tl = (code == 1) ? cmc::common_tids(c, s.fe[i], s.re[j], tids) : cmc::TidList{tids, 0, -1, -1, false};
                        const cmc::CH F{slot_fch(s, chains) + i, kmer}, R{slot_bch(s, chains) + j, kmer};
                        const cmc::Read frd{s.fseq, s.flen, 0}, brd{s.bseq, s.blen, 1};
                        cmc::MM r1, r2;
                        bool il, ok;
                        int row;
                        cmc::extend_task(c, ext, F, R, tl, frd, brd, r1, r2, il, ok, row);
                        res[lane].r1 = r1;
                        res[lane].r2 = r2;
                        res[lane].row = row;
                        res[lane].pair_type = (int)code - 1;
                        res[lane].ok = ok;
                        res[lane].is_left = il;
                    }
                }
                __syncthreads();
                CM_TICK(sm, 30);
                if (on && !early) {
                    const int lo = t_lo > b0 ? t_lo : b0, hi = t_hi < b0 + 64 ? t_hi : b0 + 64;
                    for (int y = lo; y < hi; ++y) {
                        const cmc::MM r1 = res[y - b0].r1, r2 = res[y - b0].r2;
                        if (cmc::fold_task(c, r1, r2, res[y - b0].is_left != 0, res[y - b0].ok != 0, res[y - b0].row, res[y - b0].pair_type, r1_fwd, mr)) {
                            early = true;
                            S[lane].done = 1;
                            break;
                        }
                        min_ret1 = r1.type < min_ret1 ? r1.type : min_ret1;
                        min_ret2 = r2.type < min_ret2 ? r2.type : min_ret2;
                        g1 = (r1.exons_spos >= 0) || (r1.exons_epos >= 0);
                        g2 = (r2.exons_spos >= 0) || (r2.exons_epos >= 0);
                    }
                }
                __syncthreads();
                CM_TICK(sm, 31);
            }
            // ---- owners: does the pair go on to the unpaired-chain extensions? (src/filter.cpp:344-393) ------------------------
            int a = -1;                                                 // what process_mates returns
            bool do_f = false, do_b = false;
            if (on) {
                CM_L HSlot &s = S[lane];
                if (early) a = CM_CONCRD;
                else if (mr.type == CM_CONCRD || mr.type == CM_DISCRD || mr.type == CM_CHIORF || mr.type == CM_CHIBSJ || mr.type == CM_CHI2BSJ) a = mr.type;
                else {
                    const uint32_t fun = ~s.fp & (s.nf >= 32 ? 0xffffffffu : ((1u << s.nf) - 1u));
                    const uint32_t bun = ~s.bp & (s.nb >= 32 ? 0xffffffffu : ((1u << s.nb) - 1u));
                    do_f = min_ret1 != CM_CONCRD && fun != 0;
                    do_b = min_ret2 != CM_CONCRD && bun != 0;
                    if (!cmc::leftovers_matter(mr.type, min_ret1, do_f, min_ret2, do_b)) a = mr.type;
                    else {
                        s.fun = fun;
                        s.bun = bun;
                        s.nfu = (int16_t)(do_f ? __popc(fun) : 0);
                        s.nbu = (int16_t)(do_b ? __popc(bun) : 0);
                        s.exf = 99;
                        s.exb = 99;
                        s.gf = 0;
                        s.gb = 0;
                    }
                }
            }
            __syncthreads();
            // ---- unpaired chains: one full-length extension per lane.  The reference reuses one MatchedMate for all chains of a
            // side, so only the first chain's exon lookups ever happen (stale looked_up_* flags, filter.cpp:356-385): the lane
            // with k == 0 computes the genic flag of its side.
            pre[0] = 0;
#pragma unroll
            for (int g = 0; g < HG; ++g) pre[g + 1] = pre[g] + S[g].nfu + S[g].nbu;
            for (int x = lane; x < pre[HG]; x += 64) {
                int g, u;
                locate(pre, x, g, u);
                CM_L HSlot &s = S[g];
                const bool back = u >= s.nfu;
                const int k = back ? u - s.nfu : u;
                const int ci = nth_set_bit(back ? s.bun : s.fun, k);
                const cmc::CH ch{(back ? slot_bch(s, chains) : slot_fch(s, chains)) + ci, kmer};
                const cmc::Read frd{s.fseq, s.flen, 0}, brd{s.bseq, s.blen, 1};
                cmc::MM m = cmc::mm_init(c);
                sm.err = slot_perr(s, ra.pair_err);
                const int ex = ext.chain_both_sides(ch, back ? brd : frd, m, back ? -1 : 1);
                atomicMin((int *)(back ? &s.exb : &s.exf), ex);
                if (k == 0) {
                    cmc::overlap_to_spos(c, m);
                    cmc::overlap_to_epos(c, m);
                    (back ? s.gb : s.gf) = (int8_t)((m.exons_spos >= 0) || (m.exons_epos >= 0));
                }
            }
            __syncthreads();
            CM_TICK(sm, 15);
            if (on) {
                if (a < 0) {
                    CM_L HSlot &s = S[lane];
                    if (do_f) {
                        min_ret1 = s.exf < min_ret1 ? s.exf : min_ret1;
                        g1 = s.gf;
                    }
                    if (do_b) {
                        min_ret2 = s.exb < min_ret2 ? s.exb : min_ret2;
                        g2 = s.gb;
                    }
                    cmc::mr_update_type(mr, cmc::leftover_type(min_ret1, min_ret2, g1 != 0, g2 != 0));
                    a = mr.type;
                }
                if (c.P.scan_level == 0 && a == CM_CONCRD) st = CM_CONCRD;
            }
            __syncthreads();                                           // the slots are rewritten at the top of the next attempt
        }
        // the wave's own atomicOr's on the pairs' words have reached the L2 after this (a workgroup-scope fence = s_waitcnt for a
        // one-wave block; an agent-scope __threadfence() here invalidated the CU's vector L1 once per heavy pair and cost every
        // kernel on the chip 10 - 15 %)
        __threadfence_block();
        if (owner) {
            if (st < 0) st = mr.type;
            if (__hip_atomic_load(ra.pair_err + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                ra.list[atomicAdd(ra.count, 1u)] = t;          // left as it was; the re-run launch of k_pair maps it (one lane, exact)
                active[p] = 1;                                 // (its flag: active until then)
            } else {
                uint8_t act = 1;
                cmc::finish_round(c, st, is_last, len1, len2, mr, act);
                state[p] = mr;
                active[p] = act;
                cat[p] = st;
                atomicAdd(&counters[CN_PAIR_ROUNDS], 1ull);
            }
        }
        __syncthreads();
        CM_TICK(sm, 13);
    }
#if defined(CM_DIAG)
    if (dbg_rows && lane == 0)
        for (int i = 0; i < 64; ++i) dbg_rows[(size_t)blockIdx.x * 64 + i] = tick_w[1 + i];
#endif
}

#include "cm_heavy_pipe.h"

__global__ void __launch_bounds__(BLK) k_active_cls(const uint8_t *active, uint64_t n, int8_t *cls) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n) cls[i] = active[i] ? 0 : -2;
}
__global__ void __launch_bounds__(BLK) k_gather_active(const uint32_t *perm, const unsigned int *count, unsigned long long cap, const cm_mapped_read *state,
                                                       unsigned long long *out_idx, cm_mapped_read *out_state) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= *count || i >= cap) return;
    const uint32_t p = perm[i];
    out_idx[i] = p;
    out_state[i] = state[p];
}

__global__ void __launch_bounds__(BLK) k_gather_records(const uint32_t *perm, const unsigned int *count, unsigned long long cap, const cm_mapped_read *state,
                                                        unsigned long long index_base, cm_record *out) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= *count || i >= cap) return;
    const uint32_t p = perm[i];
    out[i].pair = index_base + p;
    out[i].state = state[p];
}

// final MatchedRead::type histogram of a batch (cm_type_histogram): block-private counts in LDS, 14 atomics per block
__global__ void __launch_bounds__(BLK) k_type_hist(const cm_mapped_read *state, uint64_t n, unsigned long long *hist) {
    __shared__ unsigned int h[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLK) {
        const int t = state[i].type;
        if (t >= 0 && t < 14) atomicAdd(&h[t], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 14 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}
__global__ void k_err_clear(int *err, int mask) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAnd(err, ~mask);
}
// bucket descriptors of a loaded contig (cmc::desc_pack): one thread per hash bucket
__global__ void __launch_bounds__(BLK) k_build_desc(const uint32_t *bucket_off, const uint16_t *checksum, uint64_t n_buckets, int kmer, uint32_t *desc) {
    const uint64_t hv = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (hv >= n_buckets) return;
    const uint32_t b0 = bucket_off[hv], n = bucket_off[hv + 1] - b0;
    uint32_t out[cmc::DESC_WORDS];
    cmc::desc_pack(b0, n, [&](uint32_t i) { return (uint32_t)checksum[b0 + i]; }, kmer, out);
    uint4 v;
    v.x = out[0]; v.y = out[1]; v.z = out[2]; v.w = out[3];
    ((uint4 *)desc)[hv] = v;
}
// ---- cm_load_contig_raw: the index table flattened on the device --------------------------------------------------
// Multi-block scan of uint32 (totals stay below 2^32 here: table slots / entries of one contig): k_scan32_a scans blocks of
// S32_B items (8 consecutive items per thread) and leaves the block totals, k_scan_mid scans those in one workgroup,
// k_scan32_c adds the block bases.  add = 1: the items are in[i] + 1; inclusive: out[i] includes item i.
constexpr int S32_T = 1024, S32_E = 8, S32_B = S32_T * S32_E;
__global__ void __launch_bounds__(S32_T) k_scan32_a(const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *bsum, uint32_t add, int inclusive) {
    __shared__ uint32_t wsum[S32_T / 64];
    const uint64_t base = (uint64_t)blockIdx.x * S32_B + (uint64_t)threadIdx.x * S32_E;
    uint32_t v[S32_E], run = 0;
#pragma unroll
    for (int k = 0; k < S32_E; ++k) {
        const uint64_t i = base + k;
        v[k] = i < n ? in[i] + add : 0u;
        run += v[k];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = run;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += wsum[w];
    uint32_t pre = wbase + incl - run;               // items of this block in front of this thread's
#pragma unroll
    for (int k = 0; k < S32_E; ++k) {
        const uint64_t i = base + k;
        if (i < n) out[i] = inclusive ? pre + v[k] : pre;
        pre += v[k];
    }
    if (threadIdx.x == S32_T - 1) bsum[blockIdx.x] = pre;
}
__global__ void __launch_bounds__(S32_T) k_scan32_c(uint32_t *out, uint64_t n, const uint32_t *bsum) {
    const uint32_t add = bsum[blockIdx.x];
    const uint64_t base = (uint64_t)blockIdx.x * S32_B + (uint64_t)threadIdx.x * S32_E;
    if (add)
#pragma unroll
        for (int k = 0; k < S32_E; ++k)
            if (base + k < n) out[base + k] += add;
}
struct RawEntry { uint16_t checksum, pad; int32_t info; };        // GeneralIndex as the index file holds it (8 bytes)
// bucket i of the file: header slot at start[i] (info = number of valid entries c <= count14[i]), then its slots.
// counts[hv + 1] = c (the array is zero elsewhere: its inclusive scan is bucket_off)
__global__ void __launch_bounds__(BLK) k_raw_counts(const RawEntry *tab, const uint32_t *start, const uint32_t *hv, const uint32_t *cnt14, uint32_t n_b,
                                                   uint64_t n_buckets_all, uint32_t *counts, int *bad) {
    const uint32_t i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n_b) return;
    const int32_t c = tab[start[i]].info;
    if (c < 0 || (uint32_t)c > cnt14[i] || (uint64_t)hv[i] >= n_buckets_all || (i && hv[i] <= hv[i - 1])) {
        atomicOr(bad, 1);
        return;
    }
    counts[hv[i] + 1] = (uint32_t)c;
}
__global__ void __launch_bounds__(BLK) k_raw_scatter(const RawEntry *tab, const uint32_t *start, const uint32_t *hv, uint32_t n_b, const uint32_t *bucket_off,
                                                    uint16_t *checksum, uint32_t *pos) {
    const uint32_t i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n_b) return;
    const uint32_t h = hv[i], w = bucket_off[h], c = bucket_off[h + 1] - w;
    const RawEntry *e = tab + start[i] + 1;
    for (uint32_t k = 0; k < c; ++k) {
        const RawEntry x = e[k];
        checksum[w + k] = x.checksum;
        pos[w + k] = (uint32_t)x.info;
    }
}

// ---- cm_build_contig: the k-mer table built on the device from the sequence (bodies: cm_index_build.h) --------------
// A counting sort.  k_ib_positions<false> adds 1 to the counter of every indexable k-mer's bucket; an inclusive scan turns the
// counters into the END of every bucket; k_ib_positions<true> takes a slot from the end downwards (returning atomic) and stores
// (checksum, position) there, so that the cursors finish as the bucket STARTS: the array is bucket_off and no second 1-GiB
// cursor array exists.  The order inside a bucket is arbitrary at that point; k_ib_order_* make it (checksum, position).
constexpr int IB_PER = 8, IB_TILE = BLK * IB_PER;           // k-mer starts per lane / per workgroup
constexpr int IB_HALO = CM_WINDOW_SIZE + 8 - 1;             // k - 1 bases of the next tile, k <= 22
static_assert(cmc::CM_STAGE_PAD >= 4, "k_ib_positions reads whole words up to 3 bytes past the contig");
// genome: the slot's copy (4-byte aligned, readable for CM_STAGE_PAD bytes past ref_len).  n_pos = ref_len - k + 1 starts.
template <bool SCATTER>
__global__ void __launch_bounds__(BLK) k_ib_positions(const uint8_t *genome, uint32_t ref_len, uint32_t n_pos, int k, int c, uint32_t *cursor,
                                                      uint16_t *checksum, uint32_t *pos) {
    __shared__ uint8_t codes[IB_TILE + IB_HALO + 3];
    const uint64_t t0 = (uint64_t)blockIdx.x * IB_TILE;                     // first start of the tile (a multiple of 4)
    if (t0 >= n_pos) return;
    const uint32_t tile_pos = (uint32_t)(n_pos - t0 < (uint64_t)IB_TILE ? n_pos - t0 : (uint64_t)IB_TILE);
    const uint32_t n_codes = tile_pos + (uint32_t)k - 1;                  // t0 + n_codes <= ref_len
    const uint32_t *gw = (const uint32_t *)(genome + t0);
    for (uint32_t w = threadIdx.x; w * 4 < n_codes; w += BLK) {
        const uint32_t x = gw[w];
#pragma unroll
        for (int b = 0; b < 4; ++b) codes[w * 4 + b] = (uint8_t)cmib::base_code((uint8_t)(x >> (8 * b)));
    }
    __syncthreads();
    const uint32_t first = threadIdx.x * IB_PER;
    if (first >= tile_pos) return;
    const uint32_t mine = tile_pos - first < (uint32_t)IB_PER ? tile_pos - first : (uint32_t)IB_PER;
    cmib::scan_positions(codes + first, n_codes - first, mine, k, c, [&](uint32_t j, uint32_t hv, uint32_t ck) {
        if (SCATTER) {
            const uint32_t at = atomicSub(&cursor[hv], 1u) - 1u;
            checksum[at] = (uint16_t)ck;
            pos[at] = (uint32_t)(t0 + first + j) + 1u;
        } else {
            atomicAdd(&cursor[hv], 1u);                                    // result unused: a no-return atomic
        }
    });
}
// what the ordering passes leave for the host: [0..2] non-empty buckets per path, [3] entries of the fullest bucket,
// [4] / [5] length of the workgroup list / the oversize list
enum { IB_ST_PATH = 0, IB_ST_MAX = 3, IB_ST_NMED = 4, IB_ST_NOVER = 5, IB_ST_WORDS = 6 };
// one lane per bucket: few-entry buckets are ordered here, the others go on the list of their path
__global__ void __launch_bounds__(BLK) k_ib_order_lane(const uint32_t *bucket_off, uint64_t n_buckets, uint16_t *checksum, uint32_t *pos, uint32_t lane_max,
                                                       uint32_t wg_max, uint32_t *med_list, uint32_t *over_list, unsigned long long *st) {
    __shared__ unsigned int cnt[4];
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t hv = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (hv < n_buckets) {
        const uint32_t b0 = bucket_off[hv], n = bucket_off[hv + 1] - b0;
        const int path = cmib::bucket_path(n, lane_max, wg_max);
        if (path >= 0) {
            atomicAdd(&cnt[path], 1u);
            atomicMax(&cnt[3], n);
            if (path == 0) cmib::lane_sort(checksum + b0, pos + b0, n);
            else if (path == 1) med_list[atomicAdd(&st[IB_ST_NMED], 1ull)] = (uint32_t)hv;
            else over_list[atomicAdd(&st[IB_ST_NOVER], 1ull)] = (uint32_t)hv;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&st[IB_ST_PATH + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (threadIdx.x == 3 && cnt[3]) atomicMax(&st[IB_ST_MAX], (unsigned long long)cnt[3]);
}
// one workgroup per listed bucket (n <= IB_WG_CAP): the packed keys sorted in LDS
constexpr uint32_t IB_WG_CAP = cmib::WG_MAX;
__global__ void __launch_bounds__(BLK) k_ib_order_wg(const uint32_t *bucket_off, const uint32_t *list, uint32_t n_list, uint16_t *checksum, uint32_t *pos) {
    __shared__ uint64_t keys[IB_WG_CAP];
    for (uint32_t b = blockIdx.x; b < n_list; b += gridDim.x) {
        const uint32_t hv = list[b], b0 = bucket_off[hv], n = bucket_off[hv + 1] - b0;
        if (n > IB_WG_CAP) continue;                                   // (never listed: k_ib_order_lane classifies with wg_max <= IB_WG_CAP)
        const uint32_t np2 = cmib::pow2_at_least(n);
        for (uint32_t i = threadIdx.x; i < np2; i += BLK) keys[i] = i < n ? cmib::pack_key(checksum[b0 + i], pos[b0 + i]) : ~0ull;
        __syncthreads();
        for (uint32_t size = 2; size <= np2; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t i = threadIdx.x; i < np2; i += BLK) cmib::bitonic_step(keys, i, size, stride);
                __syncthreads();
            }
        for (uint32_t i = threadIdx.x; i < n; i += BLK) {
            checksum[b0 + i] = cmib::key_checksum(keys[i]);
            pos[b0 + i] = cmib::key_pos(keys[i]);
        }
        __syncthreads();
    }
}
// oversize list: sizes of the listed buckets (scanned into `start`), their entries packed under the bucket's rank in the chunk,
// and the sorted keys put back.  Sorted by (rank, checksum, position) a bucket's keys lie where its unsorted ones lay.
__global__ void __launch_bounds__(BLK) k_ib_over_sizes(const uint32_t *bucket_off, const uint32_t *list, uint32_t n_list, uint32_t *sizes) {
    const uint32_t i = blockIdx.x * BLK + threadIdx.x;
    if (i < n_list) sizes[i] = bucket_off[list[i] + 1] - bucket_off[list[i]];
}
__global__ void __launch_bounds__(BLK) k_ib_over_pack(const uint32_t *bucket_off, const uint32_t *list, const uint32_t *start, uint32_t r0, uint32_t r1,
                                                      const uint16_t *checksum, const uint32_t *pos, uint64_t *keys) {
    const uint32_t base = start[r0];
    for (uint32_t r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        const uint32_t b0 = bucket_off[list[r]], n = start[r + 1] - start[r], at = start[r] - base;
        for (uint32_t i = threadIdx.x; i < n; i += BLK) keys[at + i] = cmib::over_key(r - r0, checksum[b0 + i], pos[b0 + i]);
    }
}
__global__ void __launch_bounds__(BLK) k_ib_over_unpack(const uint32_t *bucket_off, const uint32_t *list, const uint32_t *start, uint32_t r0, uint32_t r1,
                                                        const uint64_t *keys, uint16_t *checksum, uint32_t *pos) {
    const uint32_t base = start[r0];
    for (uint32_t r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        const uint32_t b0 = bucket_off[list[r]], n = start[r + 1] - start[r], at = start[r] - base;
        for (uint32_t i = threadIdx.x; i < n; i += BLK) {
            const uint64_t x = keys[at + i];
            checksum[b0 + i] = cmib::key_checksum(x);
            pos[b0 + i] = cmib::key_pos(x);
        }
    }
}

// Near-border bits by index entry (Slot::entry_near): bit e = the position bitset's bit of pos[e], through the function every
// other reader of the bitset calls (a position at or beyond n_bits gives 0).  One lane per entry, one store per wave.
__global__ void __launch_bounds__(BLK) k_entry_near(const uint32_t *pos, uint64_t n_entries, const uint64_t *bits, uint64_t n_bits, uint64_t *out) {
    const uint64_t e = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    const bool b = e < n_entries && cmc::bit_at((cmc::g_u64)bits, n_bits, pos[e]);
    const unsigned long long m = __ballot(b);
    if ((threadIdx.x & 63) == 0 && e < n_entries) out[e >> 6] = m;
}

__global__ void k_init_state(KCore kc, cm_mapped_read *state, uint8_t *active, int32_t *cat, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    Core c;
    c.P = kc.P;
    cmc::default_mr(c, state[i]);
    active[i] = 1;
    cat[i] = -1;
}

// ---- cm_reads_stage_text: FASTQ text tokenised on the device (bodies and the plan: cm_fastq_text.h) ----------------
constexpr int FT_T = 256;                       // threads of a tokeniser workgroup: 4 waves, one newline chunk each
constexpr int FT_WAVES = FT_T / 64;
// What the kernels behind the line tables need to know the batch: n = pair_count() of both files' lines, on the device.
struct FtShape {
    const uint32_t *nl1, *nl2;                  // newlines of the block: the grand-total slot of the scanned chunk counts
    uint32_t trail1, trail2;                    // a last line without '\n' counts (end of input)
    uint64_t max_pairs;
    __device__ uint32_t lines(int f) const { return cmft::line_count(f ? *nl2 : *nl1, (f ? trail2 : trail1) != 0); }
    __device__ uint32_t pairs() const { return cmft::pair_count(lines(0), lines(1), max_pairs); }
};
// cnt[c] = newlines of chunk c; cnt[n_chunks] = 0, the slot the exclusive scan leaves the total in
__global__ void __launch_bounds__(FT_T) k_ft_count(const uint8_t *text, uint64_t len, uint32_t n_chunks, uint32_t *cnt) {
    const uint32_t lane = threadIdx.x & 63, c = blockIdx.x * FT_WAVES + (threadIdx.x >> 6);
    if (c > n_chunks) return;                   // (the whole wave)
    uint32_t k = c < n_chunks ? cmft::popcount16(cmft::nl_mask16(text, (uint64_t)c * cmft::NL_CHUNK + lane * cmft::LANE_BYTES, len)) : 0u;
    for (int o = 32; o; o >>= 1) k += __shfl_xor(k, o);
    if (lane == 0) cnt[c] = k;
}
// the line-start table from the scanned counts: base[c] = newlines in front of chunk c
__global__ void __launch_bounds__(FT_T) k_ft_lines(const uint8_t *text, uint64_t len, uint32_t n_chunks, const uint32_t *base, uint32_t trailing, uint32_t *ls,
                                                   uint32_t ls_cap) {
    const uint32_t lane = threadIdx.x & 63, c = blockIdx.x * FT_WAVES + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ls[0] = 0;
        const uint32_t end = base[n_chunks] + 1;                    // the sentinel behind a last line without '\n'
        if (trailing && end < ls_cap) ls[end] = (uint32_t)len + 1u;
    }
    if (c >= n_chunks) return;
    const uint64_t at = (uint64_t)c * cmft::NL_CHUNK + lane * cmft::LANE_BYTES;
    const uint32_t mask = cmft::nl_mask16(text, at, len), k = cmft::popcount16(mask);
    uint32_t incl = k;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    cmft::put_line_starts(mask, at, base[c] + incl - k, ls, ls_cap);
}
// one lane per record: verdict, sequence length (0 for i in [n, nb]: the scan's input), the first malformed record and the
// longest read through one atomic per workgroup at most
__global__ void __launch_bounds__(FT_T) k_ft_records(const uint8_t *text, const uint32_t *ls, FtShape sh, int file, uint32_t nb, uint32_t *slen,
                                                     unsigned long long *res) {
    __shared__ uint32_t wmax[FT_WAVES];
    const uint32_t i = blockIdx.x * FT_T + threadIdx.x, n = sh.pairs();
    uint32_t sl = 0;
    if (i < n) {
        const uint32_t bad = cmft::check_record(text, ls, i, file == 0, &sl);
        if (bad) atomicMin(&res[cmft::RES_BAD1 + file], cmft::bad_key(i, bad));       // (malformed input only)
    }
    if (i <= nb) slen[i] = sl;
    uint32_t m = sl;
    for (int o = 32; o; o >>= 1) m = max(m, (uint32_t)__shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FT_WAVES; ++w) m = max(m, wmax[w]);
        if (m) atomicMax(&res[cmft::RES_MAX_LEN], (unsigned long long)m);
    }
}
// off[0 .. n] from the scanned lengths (soff[n] = all bases: the lengths behind record n - 1 are zero) and the record starts
__global__ void __launch_bounds__(FT_T) k_ft_offsets(const uint32_t *ls, const uint32_t *soff, FtShape sh, uint64_t len, uint64_t *off, uint64_t *rec) {
    const uint32_t i = blockIdx.x * FT_T + threadIdx.x, n = sh.pairs();
    if (i > n) return;
    off[i] = soff[i];
    const uint32_t r = ls[4 * (uint64_t)i];
    rec[i] = r > len ? len : r;                  // (the sentinel behind a last line without '\n' is len + 1)
}
// COPY_LANES lanes per record move its bases to seq_base + CM_STAGE_PAD + off[i]; workgroup 0 clears the slack on both sides
__global__ void __launch_bounds__(FT_T) k_ft_copy(const uint8_t *text, const uint32_t *ls, const uint64_t *off, FtShape sh, uint8_t *seq_base) {
    constexpr uint32_t pad = cmc::CM_STAGE_PAD;
    static_assert(pad <= FT_T && pad % 4 == 0, "one thread per byte of slack; the reads start on a word");
    const uint32_t n = sh.pairs();
    if (blockIdx.x == 0 && threadIdx.x < pad) {
        seq_base[threadIdx.x] = 0;
        seq_base[pad + off[n] + threadIdx.x] = 0;
    }
    const uint32_t groups = gridDim.x * (FT_T / cmft::COPY_LANES), lane = threadIdx.x % cmft::COPY_LANES;
    for (uint32_t i = (blockIdx.x * FT_T + threadIdx.x) / cmft::COPY_LANES; i < n; i += groups) {
        const uint32_t s = ls[4 * (uint64_t)i + 1], l = ls[4 * (uint64_t)i + 2] - 1u - s;
        cmft::copy_bases(seq_base, pad + off[i], text, s, l, (int)lane, cmft::COPY_LANES);
    }
}
__global__ void k_ft_finish(FtShape sh, const uint64_t *off1, const uint64_t *off2, const uint64_t *rec1, const uint64_t *rec2, unsigned long long *res) {
    const uint32_t n = sh.pairs();
    res[cmft::RES_LINES1] = sh.lines(0);
    res[cmft::RES_LINES2] = sh.lines(1);
    res[cmft::RES_PAIRS] = n;
    res[cmft::RES_BASES1] = off1[n];
    res[cmft::RES_BASES2] = off2[n];
    res[cmft::RES_USED1] = rec1[n];
    res[cmft::RES_USED2] = rec2[n];
}

// ---- the names (flag bit 2, the rule: cm_pam_text.h) and the qualities (flag bit 3) cm_reads_stage_text keeps -----------------
// one lane per record of file 1: where its name starts in the text and how long it is; item n is 0, the slot the scan leaves the total in
__global__ void __launch_bounds__(FT_T) k_ft_name_len(const uint8_t *text, const uint32_t *ls, uint32_t n, uint32_t *nstart, uint32_t *nlen) {
    const uint32_t i = blockIdx.x * FT_T + threadIdx.x;
    if (i > n) return;
    uint32_t s = 0, l = 0;
    if (i < n) {
        const uint32_t h = ls[4 * (uint64_t)i];
        cmpt::name_span(text + h, ls[4 * (uint64_t)i + 1] - 1u - h, &s, &l);
        s += h;
    }
    nstart[i] = s;
    nlen[i] = l;
}
// COPY_LANES lanes per record move its name to names[name_off[i] ..), word by word
__global__ void __launch_bounds__(FT_T) k_ft_name_copy(const uint8_t *text, const uint32_t *nstart, const uint32_t *name_off, uint32_t n, uint8_t *names) {
    const uint32_t groups = gridDim.x * (FT_T / cmft::COPY_LANES), lane = threadIdx.x % cmft::COPY_LANES;
    for (uint32_t i = (blockIdx.x * FT_T + threadIdx.x) / cmft::COPY_LANES; i < n; i += groups)
        cmft::copy_bases(names, name_off[i], text, nstart[i], name_off[i + 1] - name_off[i], (int)lane, cmft::COPY_LANES);
}
// flag bit 3: COPY_LANES lanes per record move its quality line (line 4 i + 3, as long as the bases) to qual[off[i] ..), word by word
__global__ void __launch_bounds__(FT_T) k_ft_qual_copy(const uint8_t *text, const uint32_t *ls, const uint64_t *off, uint32_t n, uint8_t *qual) {
    const uint32_t groups = gridDim.x * (FT_T / cmft::COPY_LANES), lane = threadIdx.x % cmft::COPY_LANES;
    for (uint32_t i = (blockIdx.x * FT_T + threadIdx.x) / cmft::COPY_LANES; i < n; i += groups)
        cmft::copy_bases(qual, off[i], text, ls[4 * (uint64_t)i + 3], (uint32_t)(off[i + 1] - off[i]), (int)lane, cmft::COPY_LANES);
}

// ---- the row formatters cm_format_pam / cm_format_sam (the plan: cm_rows_text.h; the formats: cm_pam_text.h, cm_sam_text.h) ----
// one lane per item q of the call: its length; item `items` is 0, the slot the scan leaves the total in
template <class F>
__device__ __forceinline__ void rows_len(const typename F::Src &S, const cmrt::ChrTab &ct, uint64_t first, uint32_t items, uint32_t *len) {
    cmrt::item_length<F>(S, ct, first, items, blockIdx.x * BLK + threadIdx.x, len);
}
// the 64-bit sum of the lengths (one workgroup; launched only where the items of a call could reach 2^32 bytes)
__global__ void __launch_bounds__(BLK) k_rows_total(const uint32_t *len, uint32_t count, unsigned long long *total) {
    __shared__ unsigned long long part[BLK];
    unsigned long long t = 0;
    for (uint32_t k = threadIdx.x; k < count; k += BLK) t += len[k];
    part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < BLK; ++i) t += part[i];
        *total = t;
    }
}
// a lane of the wave that runs cmrt::format_span: every step once, for itself
struct WaveLane {
    uint8_t *win, *out;
    template <class Fn>
    __device__ __forceinline__ void in_window(uint32_t, uint32_t, Fn f) { f(threadIdx.x, win); }
    template <class Fn>
    __device__ __forceinline__ void in_output(uint32_t, uint32_t, Fn f) { f(threadIdx.x, out); }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ const uint8_t *window() const { return win; }
    __device__ __forceinline__ bool first_lane() const { return threadIdx.x == 0; }
};
// One wave (a workgroup of its own) per span of F::SPAN_ITEMS items: cmrt::format_span with the wave's LDS window.
template <class F>
__device__ __forceinline__ void rows_span(const typename F::Src &S, const cmrt::ChrTab &ct, uint64_t first, uint32_t items, const uint32_t *off, uint8_t *out, uint8_t *path) {
    __shared__ uint32_t win[cmrt::WINDOW_WORDS];
    __shared__ typename F::Scratch scratch;
    WaveLane ex{(uint8_t *)win, out};
    cmrt::format_span<F>(ex, S, ct, first, items, off, blockIdx.x, cmrt::WINDOW, scratch, path);
}
// the kernels under a name per format (profiles of both stay comparable)
__global__ void __launch_bounds__(BLK) k_pam_len(cmpt::Format::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, uint32_t *len) { rows_len<cmpt::Format>(S, ct, first, items, len); }
__global__ void __launch_bounds__(BLK) k_sam_len(cmst::Format::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, uint32_t *len) { rows_len<cmst::Format>(S, ct, first, items, len); }
__global__ void __launch_bounds__(cmrt::WAVE) k_pam_rows(cmpt::Format::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, const uint32_t *off, uint8_t *out, uint8_t *path) {
    rows_span<cmpt::Format>(S, ct, first, items, off, out, path);
}
__global__ void __launch_bounds__(cmrt::WAVE) k_sam_rows(cmst::Format::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, const uint32_t *off, uint8_t *out, uint8_t *path) {
    rows_span<cmst::Format>(S, ct, first, items, off, out, path);
}

// the remain records of one mate file (cm_format_remain): the same plan over the selection list
template <uint32_t MATE>
__global__ void __launch_bounds__(BLK) k_remain_len(cmrm::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, uint32_t *len) {
    rows_len<cmrm::Format<MATE>>(S, ct, first, items, len);
}
template <uint32_t MATE>
__global__ void __launch_bounds__(cmrt::WAVE) k_remain_rows(cmrm::Src S, cmrt::ChrTab ct, uint64_t first, uint32_t items, const uint32_t *off, uint8_t *out, uint8_t *path) {
    rows_span<cmrm::Format<MATE>>(S, ct, first, items, off, out, path);
}

// the order of the sorted remain records (cm_format_remain_sorted; the bodies and the plan: cm_remain_order.h), a lane per entry
__global__ void __launch_bounds__(BLK) k_remain_keys(cmrm::Src S, uint32_t n_chr, uint32_t n, uint64_t *rkey, uint32_t *pair) {
    const uint32_t q = blockIdx.x * BLK + threadIdx.x;
    if (q < n) cmro::entry_key(S, n_chr, q, rkey, pair);
}
__global__ void __launch_bounds__(BLK) k_remain_heads(const uint64_t *rkey, uint32_t n, uint32_t *head) { cmro::group_head(rkey, n, blockIdx.x * BLK + threadIdx.x, head); }
__global__ void __launch_bounds__(BLK) k_remain_gstart(const uint32_t *ex, uint32_t n, uint32_t *gstart) { cmro::group_start(ex, n, blockIdx.x * BLK + threadIdx.x, gstart); }
// a lane per group: ctr[0] the largest group, ctr[1] the groups of two or more members, ctr[2] their members (a workgroup's share
// through LDS, one atomic per counter and workgroup that has any)
__global__ void __launch_bounds__(BLK) k_remain_gsizes(const uint32_t *gstart, const uint32_t *n_groups, unsigned int *ctr) {
    __shared__ unsigned int part[3];
    if (threadIdx.x < 3) part[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t sz = cmro::group_size(gstart, *n_groups, blockIdx.x * BLK + threadIdx.x);
    if (sz >= 2u) {
        atomicMax(&part[0], sz);
        atomicAdd(&part[1], 1u);
        atomicAdd(&part[2], sz);
    }
    __syncthreads();
    if (threadIdx.x == 0 && part[1]) {
        atomicMax(&ctr[0], part[0]);
        atomicAdd(&ctr[1], part[1]);
        atomicAdd(&ctr[2], part[2]);
    }
}
template <uint32_t MATE>
__global__ void __launch_bounds__(BLK) k_remain_rank(cmrm::Src S, cmrt::ChrTab ct, const uint32_t *by_key, const uint32_t *ex, const uint32_t *gstart, uint32_t n, uint32_t *list) {
    cmro::rank_in_group<MATE>(S, ct, by_key, ex, gstart, n, blockIdx.x * BLK + threadIdx.x, list);
}

// ------------------------------------------------------------------ host side
struct Slot {
    bool loaded = false, has_annot = false;
    uint64_t gen = 0;                    // bumped by every (un)load: work prepared against an older content of the slot is stale
    uint32_t *d_desc = nullptr;          // bucket descriptors (cmc::desc_pack), one of idx_allocs; null when switched off
    bool chain_parallel_ok = false;      // see k_chain_heavy: no annotated hop longer than maxIntronLen
    cm_index_view X{};
    cmc::AnnotDev A{};
    std::vector<void *> idx_allocs, ann_allocs;
    // near_border_bits by index entry, u64[(n_entries + 63) / 64], for k_chain_heavy.  Made from both halves of the slot: built by
    // whichever load completes the pair (make_entry_near), dropped by every (un)load of either half, owned by neither list.
    uint64_t *entry_near = nullptr;
};

struct ProfRec { hipEvent_t a, b; ProfClass cls; };

// A device buffer that knows its size and who frees it.  Grow-only (ensure()); `Life` says when the memory goes: with the batch
// (an empty cm_reads_upload, cm_destroy -- release(ctx, BATCH)) or with the context (cm_destroy only).  A buffer is declared once,
// in cm_ctx (which is heap-allocated and never moves): the first time it allocates it enters the context's list of its lifetime
// class, and releasing a class walks that list.
enum Life { BATCH = 0, CONTEXT = 1 };
struct DevMem {
    void *p = nullptr;
    size_t cap = 0;                            // bytes behind p
    std::vector<DevMem *> *listed = nullptr;   // the lifetime list this buffer has entered
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
};
// pointer and capacity change places, the buffers stay where they are declared: one that has never allocated joins the other's list
inline void swap(DevMem &a, DevMem &b) {
    std::swap(a.p, b.p);
    std::swap(a.cap, b.cap);
    if (!a.listed && b.listed) (a.listed = b.listed)->push_back(&a);
    if (!b.listed && a.listed) (b.listed = a.listed)->push_back(&b);
}
template <class T, Life L>
struct DevBuf : DevMem {
    operator T *() const { return (T *)p; }
};
template <class T> using BatchBuf = DevBuf<T, BATCH>;
template <class T> using CtxBuf = DevBuf<T, CONTEXT>;

// One mate file's share of a batch's read buffers (file 0: R1, file 1: R2).
struct ReadFile {
    BatchBuf<uint8_t> seq_base;                  // CM_STAGE_PAD readable bytes in front of and behind the reads
    BatchBuf<uint64_t> off;
    // cm_reads_stage_text, flag bit 2 (R1) / 4 (R2): the file's names, name i = names[name_off[i] .. name_off[i + 1]); allocated with the bit
    BatchBuf<uint8_t> names;
    BatchBuf<uint32_t> name_off;
    bool has_names = false;
    uint64_t name_bytes_max = 0;                 // no more name bytes than this (the host never learns the exact number)
    // cm_reads_stage_text, flag bit 3: the file's quality lines, quality of read i = qual[off[i] .. off[i + 1]); allocated with the bit
    BatchBuf<uint8_t> qual;
    uint8_t *seq() const { return seq_base + cmc::CM_STAGE_PAD; }
};
// The read buffers of one batch, by mate file; a context has two (resident, staged) and cm_reads_swap exchanges them.
struct ReadBufs {
    ReadFile file[2];
    bool has_quals = false;                      // flag bit 3 was given: both files' qualities are kept
    uint64_t bases = 0;                          // with has_quals: off[n] of both files
    void keep_nothing() { file[0].has_names = file[1].has_names = has_quals = false; }
};
// Buffer by buffer over the files, in the order the buffers came to be: one that has never allocated joins the other's lifetime
// list here, and a batch's memory is freed in the order of that list.
inline void swap(ReadBufs &a, ReadBufs &b) {
    [[maybe_unused]] auto &[m1, m2, m3, m4, m5, m6, m7] = a.file[0];      // an eighth member does not compile until it changes places below
    for (int f = 0; f < 2; ++f) swap(a.file[f].seq_base, b.file[f].seq_base);
    for (int f = 0; f < 2; ++f) swap(a.file[f].off, b.file[f].off);
    swap(a.file[0].names, b.file[0].names);
    swap(a.file[0].name_off, b.file[0].name_off);
    for (int f = 0; f < 2; ++f) swap(a.file[f].qual, b.file[f].qual);
    swap(a.file[1].names, b.file[1].names);
    swap(a.file[1].name_off, b.file[1].name_off);
    for (int f = 0; f < 2; ++f) std::swap(a.file[f].has_names, b.file[f].has_names);
    for (int f = 0; f < 2; ++f) std::swap(a.file[f].name_bytes_max, b.file[f].name_bytes_max);
    std::swap(a.has_quals, b.has_quals);
    std::swap(a.bases, b.bases);
}

// What the seeding of a tile leaves for its chain stage: the seed ranges of every probe, the DP-cell offsets of every chaining
// problem (+ total and largest problem, also copied to h_pin[PIN_CELLS + 2 s ..]).  Two sets: see map_rounds_issue.
// The work classes of the tile's chaining problems and their sorted list (k_chain_cls + counting sort), the zeroed cursors of the
// chain kernels (improvement-log pool: cm_ctx::pool_cursor(s); heavy work list) -- everything the chain kernels need but the chain
// records themselves.
struct SeedSet {
    BatchBuf<uint32_t> sstart, scnt, sraw;
    BatchBuf<unsigned long long> celloff, bsum;
    BatchBuf<unsigned int> bmax;
    BatchBuf<int8_t> cls4;
    BatchBuf<unsigned int> cblk, cctr;           // class counters / block histograms of the CHAIN stage's sort (own copies: the pair
                                                 // stage of the previous round uses its own at the same time)
    BatchBuf<uint32_t> perm4;
    BatchBuf<int32_t> thigh;                     // high_hits per problem while the chain records are not free yet (k_chain_apply)
    bool cls_deferred = false;                   // classes made before the chain records were free, k_chain_apply still to run
    bool skip_dead = false;                      // the cell offsets (and the classes, once made) leave the dead problems out (run_seed_tile)
};
// The chain records of a round.  Two sets: the pair stage of round r reads set r & 1 while the chaining of round r + 1 fills the other.
// nchain[r] is the number of chains in the problem's records -- except for a problem the round pipeline did not chain because nobody
// reads its chains (quad_dead: the pair's other mate has no hit): there nchain[r] = 1 is a marker, "this mate has hits", resid[r] = 0
// and the first record has chain_len = 0.  Such a pair has nchain = 0 on all of the other mate, so every reader that looks at records
// of two-sided pairs only (process_read, pair_class, k_pair_cost, the heavy pairs' kernels) never meets the marker as a count.
struct ChainRecs {
    BatchBuf<cm_chain> chains;
    BatchBuf<int32_t> nchain, high;
    BatchBuf<uint16_t> resid;
};
// What a pair stage keeps once per set of chain records (item i + 1 leaves item i's alone, item i + 2 starts after ev.pair[b]): the
// ordered lists of its pairs, the class counters + work cursors, the per-pair capacity flags (zero between launches), the pairs to
// re-run (RetryArgs) with [count, cursor], the heavy-pair pipeline's fall-back list with its count.  Views: set b is the b-th half of
// one allocation each (PairSetMem, cut in prepare_resident).
struct PairSet {
    uint32_t *perm = nullptr, *hlist = nullptr;
    unsigned int *cls_ctr = nullptr;
    uint32_t *pair_err = nullptr, *retry_list = nullptr;
    unsigned int *retry_ctr = nullptr;
    uint32_t *hp_fall = nullptr;
    unsigned int *hp_fallctr = nullptr;
};
struct PairSetMem {
    BatchBuf<uint32_t> perm, hlist;
    BatchBuf<unsigned int> cls_ctr;
    BatchBuf<uint32_t> pair_err, retry_list;
    BatchBuf<unsigned int> retry_ctr;
    BatchBuf<uint32_t> hp_fall;
    BatchBuf<unsigned int> hp_fallctr;
};
// scratch of a pair stage's three-pass sort (run_pair_tile), used on the ordering stream only
struct PairSort {
    BatchBuf<int8_t> cls, sub, sub2;
    BatchBuf<uint32_t> perm1, perm0;
    BatchBuf<unsigned int> ctr2, ctr3, blk_cnt;
};
// the heavy pairs as a pipeline of kernels (cm_heavy_pipe.h): arrays of one tile
struct HeavyPipe {
    BatchBuf<HPair> pairs;
    BatchBuf<uint32_t> list2, q, q2;
    BatchBuf<HTask> T;
    BatchBuf<int8_t> tcls;                       // work class of every task, the order k_hp_tasks walks them in, the counting sort's scratch
    BatchBuf<uint32_t> tperm;
    BatchBuf<unsigned int> tblk, tctr;
    BatchBuf<HUnp> U;
    BatchBuf<cmc::PreDP> pre, pre2;
    BatchBuf<HRes> res;
    BatchBuf<uint16_t> lists;
    BatchBuf<unsigned int> ctr;
    uint32_t tasks_cap = 0, unp_cap = 0;
};
// DP cells of the chain kernels and the improvement-log pool
struct ChainWork {
    BatchBuf<double> score;
    BatchBuf<int32_t> prev;
    unsigned long long cells_cap = 0;
    BatchBuf<uint8_t> pool;
    unsigned long long pool_bytes = 0;
};
// cm_collect_*: compaction scratch sized for the batch, output staging that outlives it
struct Collect {
    BatchBuf<int8_t> cls;
    BatchBuf<uint32_t> perm;
    BatchBuf<unsigned int> blk, ctr;
    CtxBuf<unsigned long long> idx;
    CtxBuf<cm_mapped_read> st;
    CtxBuf<cm_record> rec;
};

// cm_reads_stage_text: per file the block's text, the newline counts per chunk (scanned in place), the line-start table, the
// sequence lengths (scanned in place) and the record starts; the scans' block totals and the result block (cmft::Res).
struct TextStage {
    BatchBuf<uint8_t> text[2];
    BatchBuf<uint32_t> cnt[2], ls[2], slen[2];
    BatchBuf<uint64_t> rec[2];
    BatchBuf<uint32_t> tmp;
    BatchBuf<unsigned long long> res;
    BatchBuf<uint32_t> nstart;                   // flag bits 2 and 4 only: where each name starts in its text (R1's, then R2's: one stream)
};
// A column of the chromosome table on the device with its host mirror: a call compares its table with the mirror and uploads only
// a column that differs (RowsRun::prepare).
template <class T>
struct ChrColumn {
    std::vector<T> host;
    bool valid = false;
    CtxBuf<T> dev;
    bool holds(const std::vector<T> &now) const { return valid && now == host; }
};
// One output file of a row formatter's call: the items' lengths scanned in place into offsets, the rows or records, every span's path.
struct RowsFileBufs {
    BatchBuf<uint32_t> off;
    BatchBuf<uint8_t> out, path;
};
// The row formatters' buffers, shared by cm_format_pam, cm_format_sam (one file) and cm_format_remain, cm_format_remain_sorted (two:
// both are sized before either is written).  The chromosome table in columns -- the names' text and offsets, and for the remain
// records the shifts (cm_chr_info.start_pos) --, the 64-bit totals of the files, the scan's block totals, the files' own buffers.
struct RowsBufs {
    ChrColumn<uint8_t> chr_text;
    ChrColumn<uint32_t> chr_off, chr_shift;
    CtxBuf<unsigned long long> total;
    BatchBuf<uint32_t> tmp;
    RowsFileBufs file[2];
    std::vector<uint8_t> h_path;
    BatchBuf<int64_t> keys;                      // the remain records' sort keys
    // cm_format_remain_sorted only: the radix keys and pairs before and behind the sort, its workspace, the heads scanned into group
    // numbers, the groups' starts and counters, the selection list of either mate file
    BatchBuf<uint64_t> rkey0, rkey1;
    BatchBuf<uint32_t> pair0, by_key, heads, gstart, list1, list2;
    BatchBuf<uint8_t> sort_ws;
    CtxBuf<unsigned int> ties;
};

// The streams of a context, under the letters of DESIGN §4.  STREAMS lists them in creation order, which decides the hardware
// queue a stream lands on; everything that walks the streams walks that table.
struct Streams {
    hipStream_t B = nullptr;       // main: seeding of the first item, chaining, everything outside cm_map_rounds
    hipStream_t B2 = nullptr;      // heavy work of a chain stage, concurrent with the light kernel on B
    hipStream_t C = nullptr;       // H2D copies of the staged batch (cm_reads_stage)
    // The pair stage of round r runs on its own streams while B / B2 already seed and chain round r + 1 (cm_map_rounds): seeds
    // and chains are functions of (read, contig) only, the carried state enters in the pair stage.
    hipStream_t P = nullptr, P2 = nullptr;
    hipStream_t R = nullptr;       // the late launches of a pair stage: fall-back, re-run (RetryArgs)
    hipStream_t O = nullptr;       // work classes + ordered lists of a pair stage, computed under the pair stage of the item before
    hipStream_t S = nullptr;       // seeding of the NEXT item, issued while the chain stage of this one runs (map_rounds_issue)
};
enum StreamKind { BLOCKING, NON_BLOCKING, NON_BLOCKING_LOWEST };
struct StreamDef {
    hipStream_t Streams::*st;
    const char *name;              // in teardown diagnostics
    StreamKind kind;
};
// P at the lowest priority: the light kernel's persistent waves are the filler of a pair stage, and the short kernels of the heavy
// pairs' pipeline and of the next item's seeding / chaining get their workgroups placed first (hg38-like step 74.3 -> 70.9 ms; 72.3
// with the pipeline's stream raised instead, 76.9 with both, 72.9 with the heavy chaining stream lowered).
constexpr StreamDef STREAMS[] = {
    {&Streams::B, "main", BLOCKING},           {&Streams::B2, "heavy chains", BLOCKING},     {&Streams::C, "copy", NON_BLOCKING},
    {&Streams::P, "pairs", NON_BLOCKING_LOWEST}, {&Streams::P2, "heavy pairs", NON_BLOCKING}, {&Streams::R, "re-run", NON_BLOCKING},
    {&Streams::O, "pair ordering", NON_BLOCKING}, {&Streams::S, "seeding", NON_BLOCKING},
};
// The events of a context, all without timing.  Nothing but hipEvent_t in here: creation and destruction walk the struct as an array.
struct Events {
    hipEvent_t fork = nullptr, join = nullptr;          // B -> B2 -> B around the heavy chains
    hipEvent_t join_p = nullptr, tail = nullptr;
    hipEvent_t flags = nullptr;                         // main stream: the pair stage two items back is complete (its flags may be read: early seeding)
    hipEvent_t staged = nullptr, retired = nullptr;     // the staged batch's copies are complete / the buffers a swap retired are free
    hipEvent_t order[2] = {nullptr, nullptr};           // work classes + ordered lists of a pair stage of set b are complete
    hipEvent_t seed[2] = {nullptr, nullptr};            // seeds + cell offsets of a seed set are complete
    hipEvent_t first[2] = {nullptr, nullptr};           // an item's two pair kernels are done (set b): its re-run may start
    hipEvent_t prep[2] = {nullptr, nullptr}, pair[2] = {nullptr, nullptr};
    hipEvent_t *begin() { return &fork; }
    hipEvent_t *end() { return begin() + sizeof(Events) / sizeof(hipEvent_t); }
};
static_assert(sizeof(Events) == 17 * sizeof(hipEvent_t), "Events holds events only");

}  // namespace

struct cm_ctx {
    cm_params P{};
    unsigned id = 0;                          // serial number of the context in this process: names it in teardown diagnostics
    int teardown_errors = 0;
    Streams st;
    Events ev;
    std::vector<DevMem *> bufs[2];            // [Life]: the buffers of that lifetime which hold memory
    // The late launches of a pair stage: the re-run (RetryArgs) and the fall-back of the heavy-pair pipeline (k_pair_heavy over the
    // pairs that did not fit its arrays), decided late: see settle_pair.
    struct Rerun {
        bool deferred = false;
        cmc::KCore core;
        ReadsDev rd;
        uint64_t p0 = 0;
        uint32_t nt = 0;
        cm_chain *chains = nullptr;
        int32_t *nchain = nullptr, *high = nullptr;
        uint8_t *act_out = nullptr;
        int is_last = 0, cap2 = 0;
        size_t lds2 = 0;
        bool fall = false;
        size_t lds_heavy = 0;
        int str_cap = 0;
        unsigned fall_grid = 0;
    } rerun[2];
    bool pair_pending[2] = {false, false};
    // cross-batch prefetch (cm_map_rounds): the staged batch's first round seeded and chained under this batch's last pair stage
    int item_base = 0;                        // items (tile x round) mapped so far: item i uses chain-record set (item_base + i) & 1
    bool pre_launched = false;                // done for the staged batch ...
    bool pre_ready = false;                   // ... which cm_reads_swap has made the current one
    int pre_slot = -1, pre_b = 0;
    uint64_t pre_gen = 0, pre_n = 0;
    uint32_t pre_nt = 0;                      // pairs of the prefetched item (the staged batch's first tile)
    BatchBuf<uint8_t> d_ones;                 // all-active flags of a fresh batch
    uint64_t ones_cap = 0;
    unsigned long long *h_pin = nullptr;          // page-locked landing zone of the scalar read-backs (cell total, error flags, counts)
    uint32_t h_pin_nt = 0;                        // pairs of the tile whose heavy load was last sent to h_pin[PIN_HEAVY_LOAD] (0: none yet)
    std::string err = "";
    Slot slots[MAX_SLOTS];
    cm_circ_chain_ws circ_ws{};               // cm_circ_chain_batch's device workspace: grow-only, filled by cm_circ_chain_run, released by cm_destroy
    // reads
    uint64_t n_pairs = 0;
    ReadBufs rd;
    BatchBuf<cm_mapped_read> d_state;
    BatchBuf<uint8_t> d_active;               // current flags (valid after the last completed round)
    BatchBuf<uint8_t> d_active_b;             // the other parity: a round reads one array and writes the other
    BatchBuf<int32_t> d_cat;
    int n_seeds = 0, max_len = 0;
    // The staged batch (cm_reads_stage, cm_reads_stage_text): a second set of read buffers filled on the copy stream while the
    // resident batch is mapped.  stage_open and commit() write the record, cm_reads_swap and the prefetch of cm_map_rounds read it.
    struct Staged {
        bool ready = false, has_prior = false;    // a batch is staged and not yet swapped in; its carried states are in `prior`
        uint64_t n_pairs = 0;
        int max_len = 0;
        ReadBufs rd;
        BatchBuf<cm_mapped_read> prior;
        void reset() { commit(0, 0, false, false), rd.keep_nothing(); }
        void commit(uint64_t n, int len, bool carried, bool is_ready = true) { n_pairs = n, max_len = len, has_prior = carried, ready = is_ready; }
    } staged;
    TextStage ft;                             // cm_reads_stage_text
    RowsBufs rows;                            // cm_format_pam, cm_format_sam
    // workspace of one tile
    uint32_t tile = 0;
    SeedSet seed[2];                          // item i + 1 is seeded into one while the chain stage of item i reads the other
    ChainRecs rec[2];
    PairSetMem pair_mem;
    PairSet pset[2];
    PairSort sort;
    ChainWork dp;
    HeavyPipe hp;
    Collect col;
    BatchBuf<unsigned long long> d_lane_clk;      // diagnostic build of the timing study only
    BatchBuf<HRes> d_hres;                        // task outcomes of k_pair_heavy: 64 per resident block
    BatchBuf<unsigned long long> d_type_hist;
    BatchBuf<unsigned long long> d_heavy_load;    // cost beyond HEAVY_COST summed over the tile in the pair stage (k_pair_cost)
    BatchBuf<cmc::MemoSpill> d_spill;             // RETRY_GRID x 64 lanes x RETRY_SPILL overflow entries of the extension memo
    CtxBuf<unsigned long long> d_pool_cursor;     // [seed set]
    unsigned long long *pool_cursor(int s) const { return d_pool_cursor + s; }
    CtxBuf<int> d_err;
    CtxBuf<unsigned long long> d_counters;
    std::vector<unsigned long long> h_celloff;
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_free;           // timing events are recycled: creating them is slow and comes in bursts
    double ms[PC_COUNT] = {};                  // [ProfClass]
    uint64_t launches[PC_COUNT] = {};
};

namespace {

int fail(cm_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}
#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail(ctx, (e_ == hipErrorOutOfMemory) ? CM_ENOMEM : CM_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// A HIP status nobody can return to the caller (teardown, frees inside grow-only buffers).  An asynchronous error -- a fault of a
// kernel this context launched -- is sticky and would otherwise first show as an abort inside whatever context runs next;
// reported here it carries the id of the context that raised it.  The first few per context go to stderr.
void report_hip(cm_ctx *ctx, const char *what, hipError_t e) {
    if (e == hipSuccess) return;
    const int k = ctx ? ctx->teardown_errors++ : 0;
    if (k < 8) fprintf(stderr, "[cmhot] context #%u: %s failed: %s (%d)\n", ctx ? ctx->id : 0u, what, hipGetErrorString(e), (int)e);
}

template <class T>
int up(cm_ctx *ctx, std::vector<void *> &allocs, const T *host, size_t n, const T **dev) {
    void *d = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    HIPCHK(ctx, hipMalloc(&d, bytes));
    allocs.push_back(d);
    if (n) HIPCHK(ctx, hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->st.B));
    *dev = (const T *)d;
    return CM_OK;
}
void free_all(cm_ctx *ctx, std::vector<void *> &v) {
    for (void *p : v) report_hip(ctx, "hipFree", hipFree(p));
    v.clear();
}
void drop_entry_near(cm_ctx *ctx, Slot &s) {
    if (s.entry_near) report_hip(ctx, "hipFree", hipFree(s.entry_near));
    s.entry_near = nullptr;
}
// Grow-only buffers: a batch re-uses the previous batch's allocation when it is large enough.  hipFree + hipMalloc
// of the multi-GB workspaces cost ~0.85 s per 1 M-pair batch on MI355X, 85x the mapping itself (tests/diag/upload_rate.py).
// On growth the old memory is freed first and the contents are lost; 0 bytes allocate 1.
void dfree(cm_ctx *c, DevMem &m) {
    if (m.p) report_hip(c, "hipFree", hipFree(m.p));
    m.p = nullptr;
    m.cap = 0;
}
template <class T, Life L>
hipError_t ensure(cm_ctx *c, DevBuf<T, L> &m, size_t bytes) {
    if (m.p && m.cap >= bytes) return hipSuccess;
    dfree(c, m);
    const hipError_t e = hipMalloc(&m.p, bytes ? bytes : 1);
    if (e != hipSuccess) return e;
    m.cap = bytes;
    if (!m.listed) (m.listed = &c->bufs[L])->push_back(&m);
    return e;
}
// every buffer of one lifetime class
void release(cm_ctx *c, Life l) {
    for (DevMem *m : c->bufs[l]) {
        dfree(c, *m);
        m->listed = nullptr;
    }
    c->bufs[l].clear();
}

void free_reads(cm_ctx *c) {
    // the staged buffers may still be the target of copies in flight
    if (c->st.C) report_hip(c, "hipStreamSynchronize(copy stream)", hipStreamSynchronize(c->st.C));
    release(c, BATCH);
    c->pset[0] = c->pset[1] = PairSet{};
    c->ones_cap = 0;
    c->pre_launched = c->pre_ready = false;
    c->staged.reset();
    c->n_pairs = 0;
    c->tile = 0;
}

static hipEvent_t take_event(cm_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->ev_free.empty()) {
        e = c->ev_free.back();
        c->ev_free.pop_back();
    } else (void)hipEventCreate(&e);
    return e;
}
struct Timer {
    cm_ctx *c;
    ProfClass cls;
    ProfRec r{};
    bool on;
    hipStream_t st;
    Timer(cm_ctx *ctx, ProfClass k, hipStream_t stream = nullptr) : c(ctx), cls(k), on(ctx->prof), st(stream ? stream : ctx->st.B) {
        if (on) {
            r.a = take_event(c);
            r.b = take_event(c);
            r.cls = cls;
            (void)hipEventRecord(r.a, st);
        }
    }
    ~Timer() {
        if (on) {
            (void)hipEventRecord(r.b, st);
            c->recs.push_back(r);
        }
    }
};

// A kernel launch that its profile class counts: launch and count in one place, so that cm_prof_get's launches[] (which bench.py
// prints and divides by) cannot drift from the kernel sequences.  The arguments convert implicitly to the kernel's parameter types.
template <class T> struct AsIs { using type = T; };          // (keeps `args` out of the deduction: KArgs comes from the kernel alone)
template <class... KArgs>
void launch(cm_ctx *ctx, ProfClass cls, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t st, typename AsIs<KArgs>::type... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    if (cls != PC_NONE) ++ctx->launches[cls];
}
// The counting sort of n elements by class, 16 classes at most: k_cls_hist -> k_cls_scan -> k_cls_place on one stream, counted by
// the profile class pc (PC_NONE: by nobody).
struct CountingSort {
    hipStream_t st;
    const int8_t *cls;                       // class of element i (negative: left out)
    uint32_t n;
    unsigned int *blk;                       // scratch: [class][block] counts; nb = blocks of CLS_T elements that n makes
    uint32_t nb;
    unsigned int *ctr;                       // out: CTR_WORDS words (totals, CTR_SUM, CTR_BASE + class)
    uint32_t *perm;                          // out: the elements by class, highest class first, stable
    int n_used = N_CLS;                      // classes the caller produces
    uint32_t *hlist = nullptr;               // optional: the list of HEAVY_CLS, when the bit mask `separate` of classes kept out of perm
    int separate = -1;                       //           (none: -1) names it
    const uint32_t *order = nullptr;         // optional: visit the elements in this order (a later pass of an LSD radix sort) ...
    const unsigned int *n_order = nullptr;   // ... its length, on the device
    const unsigned int *n_dev = nullptr;     // optional: the elements there are, on the device (at most n); only the blocks in use are visited
    uint32_t grid_cap = 0;                   // workgroups of hist / place at most (0: one per block)
};
void counting_sort(cm_ctx *ctx, ProfClass pc, const CountingSort &a) {
    const dim3 grid(a.grid_cap && a.grid_cap < a.nb ? a.grid_cap : a.nb);
    const unsigned int *count = a.order ? a.n_order : a.n_dev;
    launch(ctx, pc, k_cls_hist, grid, dim3(CLS_W), 0, a.st, a.cls, a.n, a.blk, a.nb, a.order, count);
    launch(ctx, pc, k_cls_scan, dim3(1), dim3(SCAN_CLS_T), 0, a.st, a.blk, a.nb, a.ctr, a.separate, a.n_used, a.n_dev);
    launch(ctx, pc, k_cls_place, grid, dim3(CLS_W), 0, a.st, a.cls, a.n, a.blk, a.nb, a.ctr, a.perm, a.hlist, a.order, count);
}

KCore make_core(const cm_ctx *c, const Slot &s) {
    KCore k;
    k.P = c->P;
    k.X = s.X;
    k.A = s.A;
    k.desc = s.d_desc;
    k.entry_near = s.entry_near;
    return k;
}

int check_slot(cm_ctx *ctx, int slot, bool need_annot) {
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (!ctx->slots[slot].loaded) return fail(ctx, CM_ESTATE, "contig slot %d not loaded", slot);
    if (need_annot && !ctx->slots[slot].has_annot) return fail(ctx, CM_ESTATE, "annotation of slot %d not loaded", slot);
    return CM_OK;
}

ReadsDev reads_dev(const ReadBufs &r) { return ReadsDev{r.file[0].seq(), r.file[1].seq(), r.file[0].off, r.file[1].off}; }
ReadsDev current_reads(const cm_ctx *ctx) { return reads_dev(ctx->rd); }

constexpr unsigned HP_PLAN_GRID = 2048;      // workgroups of k_hp_plan (each with its own task-list scratch)
// CM_HEAVY_PIPELINE=0: the heavy pairs of a tile through k_pair_heavy alone (the round-3 path)
static bool heavy_pipeline() {
    static const bool v = !(getenv("CM_HEAVY_PIPELINE") && getenv("CM_HEAVY_PIPELINE")[0] == '0');
    return v;
}
static unsigned long long chain_light_w() {
    static const unsigned long long v = getenv("CM_CHAIN_LIGHT_W") ? strtoull(getenv("CM_CHAIN_LIGHT_W"), nullptr, 10) : 256ull;
    return v;
}
static unsigned int chain_light_cells() {
    static const unsigned int v = getenv("CM_CHAIN_LIGHT_CELLS") ? (unsigned)atoi(getenv("CM_CHAIN_LIGHT_CELLS")) : 96u;
    return v;
}

// The round pipeline leaves unchained the problems whose chains nobody reads (quad_dead).  The rule rests on "a retained hit makes a
// chain", which needs room for one chain: max_chain_len >= 1, all cm_create admits.
static bool skip_dead_chains(const cm_ctx *ctx) { return ctx->P.max_chain_len >= 1; }

// seeds of one tile into seed set s, on stream st: k_seed, the scan of the problems' DP cells, the two totals to the host; with
// rb (the chain records the tile's chain stage will fill: their per-problem counters are initialised here) also the work
// classes + sorted lists of the chaining problems and the zeroed cursors.  ev.seed[s] is recorded behind them.
// The second half of run_seed_tile: the work classes + sorted lists of the chaining problems of seed set s, the per-problem counters of
// the chain records rb and the zeroed cursors.  (On its own when the seeds were computed before the chain records were free: the
// cross-batch prefetch.)
// skip_dead: as the seeds' scan was told (run_seed_tile).
static int seed_classes(cm_ctx *ctx, uint64_t pair0, uint32_t n_tile, const uint8_t *act, int s, hipStream_t st, const ChainRecs *rb, bool skip_dead,
                        bool defer = false) {
    const int S = ctx->n_seeds;
    const uint32_t n_prob = n_tile * 4u;
    if ((uint64_t)n_prob * (uint64_t)S == 0) return CM_OK;
    const SeedSet &sb = ctx->seed[s];
    if (sb.skip_dead != skip_dead) return fail(ctx, CM_ESTATE, "seed set %d: cell offsets and classes disagree about unchained problems", s);
    // Light problems: one lane each, index order.  Heavy problems (many hits): one wave each (k_chain_heavy), heaviest class
    // first.  (Used by run_chain_tile when it takes the split path; computed here because these five small launches, queued
    // behind the persistent pair kernels of the previous item, took 6 ms of the chain stage's critical path.)
    Timer t(ctx, PC_ORDER, st);
    // defer: the chain records rb are still read by an earlier pair stage -- nothing is written into them here, run_chain_tile does that
    // (k_chain_apply) when it is ordered behind that stage
    launch(ctx, PC_ORDER, k_chain_cls, dim3((n_prob + BLK - 1) / BLK), dim3(BLK), 0, st, sb.scnt, sb.sraw, S, n_prob, sb.cls4, defer ? sb.thigh : rb->high,
           chain_light_w(), chain_light_cells(), defer ? (int32_t *)nullptr : rb->nchain, defer ? (uint16_t *)nullptr : rb->resid,
           defer ? (cm_chain *)nullptr : rb->chains, act, pair0, skip_dead ? 1 : 0, ctx->d_counters);
    ctx->seed[s].cls_deferred = defer;
    counting_sort(ctx, PC_ORDER, {st, sb.cls4, n_prob, sb.cblk, (n_prob + CLS_T - 1) / CLS_T, sb.cctr, sb.perm4});
    HIPCHK(ctx, hipMemsetAsync(ctx->pool_cursor(s), 0, sizeof(unsigned long long), st));
    HIPCHK(ctx, hipMemsetAsync(sb.cctr + CTR_CHAIN_NEXT, 0, sizeof(unsigned int), st));
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}
// skip_dead: the round pipeline's rule -- a problem whose chains nobody reads (quad_dead) gets no DP cells, no class and no chains.
// Off for the test hooks (cm_seed_batch, cm_chain_batch), which chain everything.
int run_seed_tile(cm_ctx *ctx, const KCore &core, const ReadsDev &rd, uint64_t pair0, uint32_t n_tile, const uint8_t *act, int s, hipStream_t st,
                  const ChainRecs *rb, bool skip_dead, bool defer_rb = false) {
    const int S = ctx->n_seeds;
    const uint64_t total = (uint64_t)n_tile * 4u * (uint64_t)S;
    if (total == 0) return CM_OK;
    const SeedSet &sb = ctx->seed[s];
    {
        Timer t(ctx, PC_SEED, st);
        launch(ctx, PC_SEED, k_seed, dim3((unsigned)((total + BLK - 1) / BLK)), dim3(BLK), 0, st, core, rd, act, pair0, n_tile, S, sb.sstart, sb.scnt, sb.sraw,
               ctx->d_counters);
    }
    const uint32_t n_prob = n_tile * 4u;
    {
        Timer t(ctx, PC_SCAN, st);
        const uint32_t nb = (n_prob + SCAN_ELEMS - 1) / SCAN_ELEMS;
        launch(ctx, PC_SCAN, k_scan_a, dim3(nb), dim3(SCAN_T), 0, st, sb.scnt, S, n_prob, sb.celloff, sb.bsum, sb.bmax, skip_dead ? 1 : 0);
        ctx->seed[s].skip_dead = skip_dead;
        launch(ctx, PC_SCAN, k_scan_mid<unsigned long long, true>, dim3(1), dim3(1024), 0, st, sb.bsum, nb, sb.celloff + n_prob, sb.bmax);
        launch(ctx, PC_SCAN, k_scan_c, dim3((n_prob + SCAN_T - 1) / SCAN_T), dim3(SCAN_T), 0, st, sb.celloff, sb.bsum, n_prob);
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin + PIN_CELLS + 2 * s, sb.celloff + n_prob, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (rb) {
        const int rc = seed_classes(ctx, pair0, n_tile, act, s, st, rb, skip_dead, defer_rb);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev.seed[s], st));
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}

// chains of one tile from seed set s (run_seed_tile) into the chain records rb.  `after_launch` (may be empty) is called once, when
// the chain kernels of the tile have been launched and before the host waits for them.
int run_chain_tile(cm_ctx *ctx, const KCore &core, const ReadsDev &rd, uint64_t pair0, uint32_t n_tile, bool parallel_ok, const uint8_t *act,
                   const ChainRecs &rb, int s, const std::function<int()> &after_launch = {}) {
    const int S = ctx->n_seeds;
    const uint32_t n_prob = n_tile * 4u;
    if (n_prob == 0 || S == 0) return after_launch ? after_launch() : CM_OK;
    const SeedSet &sb = ctx->seed[s];
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.seed[s], 0));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev.seed[s]));
    if (ctx->seed[s].cls_deferred) {           // classes made while the chain records were in use (the caller has ordered this stream behind that)
        hipLaunchKernelGGL(k_chain_apply, dim3((n_prob + BLK - 1) / BLK), dim3(BLK), 0, ctx->st.B, n_prob, (const int8_t *)sb.cls4, (const int32_t *)sb.thigh,
                           rb.high, rb.nchain, rb.resid, rb.chains);
        ctx->seed[s].cls_deferred = false;
    }
    const unsigned long long total = ctx->h_pin[PIN_CELLS + 2 * s];
    const unsigned long long max_cells = ctx->h_pin[PIN_CELLS + 2 * s + 1];      // of one problem
    // problem ranges whose DP cells fit the workspace
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    if (total <= ctx->dp.cells_cap) {
        ranges.push_back({0u, n_prob});
    } else {
        ctx->h_celloff.resize((size_t)n_prob + 1);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_celloff.data(), sb.celloff, ((size_t)n_prob + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
        uint32_t a = 0;
        while (a < n_prob) {
            uint32_t b = a;
            while (b < n_prob && ctx->h_celloff[b + 1] - ctx->h_celloff[a] <= ctx->dp.cells_cap) ++b;
            if (b == a) return fail(ctx, CM_ELIMIT, "one chaining problem needs %llu DP cells (> workspace %llu)",
                                    ctx->h_celloff[a + 1] - ctx->h_celloff[a], ctx->dp.cells_cap);
            ranges.push_back({a, b});
            a = b;
        }
    }
    // k_chain_heavy keeps a problem's hit positions in LDS: sized for the largest problem of this tile (a multiple of 2 KB, so
    // that launches of similar tiles share a configuration), not for the n_seeds x seed_lim a problem could have in theory --
    // the kernel waits on memory most of the time and the LDS request decides how many waves a CU holds.
    // (+ behind the hits: one bit per cell and a queue of 320 hits, see the kernel's upper_bound pass; behind those the improved
    // bits, one per cell padded per slot.  Those go into the 2 KB of slack of the hits' part where it has them -- the request of
    // such a tile is what it was without them -- and are added where the hits' part is the theoretical bound.)
    const size_t lds_extra = ((size_t)max_cells / 64 + 2) * 8 + 640;
    const size_t lds_need = (size_t)max_cells * sizeof(uint32_t) + lds_extra + (size_t)heavy_im_words((uint32_t)max_cells, (uint32_t)S) * sizeof(uint32_t);
    const size_t heavy_lds = std::max<size_t>(std::min<size_t>((size_t)S * (size_t)ctx->P.seed_lim * sizeof(uint32_t),
                                                               ((size_t)max_cells * sizeof(uint32_t) + 2047) / 2048 * 2048 + 2048) + (lds_extra + 255) / 256 * 256,
                                              (lds_need + 255) / 256 * 256);
#if defined(CM_CHAIN_DIAG)
    fprintf(stderr, "heavy_lds %zu (largest problem %llu cells)\n", heavy_lds, max_cells);
#endif
    // (otherwise everything stays on the sequential kernel and the class lists of run_seed_tile go unused)
    const bool split = ranges.size() == 1 && parallel_ok && heavy_lds <= 152u * 1024u;
    bool fresh = true;            // the cursors are still as run_seed_tile zeroed them
    // one launch group over problems [a, b) whose DP cells start at `base`: the improvement log of every problem comes out of the
    // shared pool, whose cursor starts at 0 for every group
    auto launch_group = [&](uint32_t a, uint32_t b, unsigned long long base, bool use_split) -> int {
        const uint32_t n = b - a;
        if (!fresh) {
            HIPCHK(ctx, hipMemsetAsync(ctx->pool_cursor(s), 0, sizeof(unsigned long long), ctx->st.B));
            HIPCHK(ctx, hipMemsetAsync(sb.cctr + CTR_CHAIN_NEXT, 0, sizeof(unsigned int), ctx->st.B));
        }
        fresh = false;
        if (use_split) {          // the few long problems run on the second stream, concurrently with the bulk
            HIPCHK(ctx, hipEventRecord(ctx->ev.fork, ctx->st.B));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B2, ctx->ev.fork, 0));
            {
            Timer t(ctx, PC_CHAIN_HEAVY, ctx->st.B2);
            // (a property of the function, process-wide: only ever raised, so a launch in flight from another context of this
            // process never sees its limit lowered)
            static std::atomic<size_t> heavy_attr{64u * 1024u};
            if (heavy_lds > heavy_attr.load()) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)k_chain_heavy, hipFuncAttributeMaxDynamicSharedMemorySize, (int)heavy_lds));
                heavy_attr.store(heavy_lds);
            }
            const uint32_t hb = n < 8192u ? n : 8192u;
            launch(ctx, PC_CHAIN_HEAVY, k_chain_heavy, dim3(hb), dim3(64), heavy_lds, ctx->st.B2, core, rd, pair0, S, sb.sstart, sb.scnt, sb.celloff,
                   ctx->dp.score, ctx->dp.prev, ctx->dp.pool, ctx->dp.pool_bytes, ctx->pool_cursor(s), rb.chains, rb.nchain, ctx->d_err, rb.resid, sb.perm4,
                   sb.cctr + CTR_BASE + CHAIN_LIGHT_CLS - 1, sb.cctr + CTR_CHAIN_NEXT, ctx->d_counters);
            }
            HIPCHK(ctx, hipEventRecord(ctx->ev.join, ctx->st.B2));
        }
        Timer t(ctx, PC_CHAIN);
        launch(ctx, PC_CHAIN, k_chain, dim3((n + BLK_CHAIN - 1) / BLK_CHAIN), dim3(BLK_CHAIN), 0, ctx->st.B, core, rd, act, pair0, a, b, S, sb.sstart, sb.scnt,
               sb.sraw, sb.celloff, base, ctx->dp.score, ctx->dp.prev, ctx->dp.pool, ctx->dp.pool_bytes, ctx->pool_cursor(s), rb.chains, rb.nchain, rb.high,
               ctx->d_err, rb.resid, use_split ? sb.perm4 : (const uint32_t *)nullptr, sb.cctr + CTR_BASE + CHAIN_LIGHT_CLS - 1, sb.cctr + CTR_SUM,
               sb.skip_dead ? (const int8_t *)sb.cls4 : (const int8_t *)nullptr);
        if (use_split) HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.join, 0));       // timed with the light kernel: the stage ends here
        HIPCHK(ctx, hipGetLastError());
        return CM_OK;
    };
    // did the group run out of log space?  (one small read-back per group; the pair stage must not start on truncated logs)
    auto pool_lost = [&](bool *lost) -> int {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin + PIN_POOL_ERR, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
        const int e = *(const int *)(ctx->h_pin + PIN_POOL_ERR);
        *lost = (e & cmc::ERR_POOL) != 0;
        if (*lost) {                                          // the other flags stay for cm_sync to report (the pair stage of the
            hipLaunchKernelGGL(k_err_clear, dim3(1), dim3(64), 0, ctx->st.B, ctx->d_err, (int)cmc::ERR_POOL);   // previous round may be setting some right now)
            HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
        }
        return CM_OK;
    };
    const unsigned long long pool_max = getenv("CM_POOL_MAX") ? strtoull(getenv("CM_POOL_MAX"), nullptr, 10) : (48ull << 30);
    bool told = false;
    for (auto &rg : ranges) {
        unsigned long long base = 0;
        if (rg.first != 0) base = ctx->h_celloff[rg.first];
        int rc = launch_group(rg.first, rg.second, base, split);
        if (rc) return rc;
        if (!told && after_launch && (rc = after_launch())) return rc;
        told = true;
        bool lost = false;
        if ((rc = pool_lost(&lost))) return rc;
        // The reference's score2chain has no capacity limit.  When the log pool ran out: first a larger pool (x4 up to pool_max)
        // and the same group again; then the group in halves on the one-lane-per-problem kernel, every piece with the whole pool
        // to itself.  Every retry recomputes its problems from the seeds, so nothing of the failed attempt survives.
        while (lost && ctx->dp.pool_bytes < pool_max) {
            unsigned long long want = ctx->dp.pool_bytes * 4ull;
            if (want > pool_max) want = pool_max;
            HIPCHK(ctx, hipStreamSynchronize(ctx->st.B2));
            if (ensure(ctx, ctx->dp.pool, want) != hipSuccess) {            // not enough HBM for a larger pool: keep the old size, go to the split path
                (void)hipGetLastError();
                HIPCHK(ctx, ensure(ctx, ctx->dp.pool, ctx->dp.pool_bytes));
                break;
            }
            ctx->dp.pool_bytes = want;
            if ((rc = launch_group(rg.first, rg.second, base, split))) return rc;
            if ((rc = pool_lost(&lost))) return rc;
        }
        if (lost) {
            std::vector<std::pair<uint32_t, uint32_t>> todo{{rg.first, rg.second}};
            while (!todo.empty()) {
                const auto pc = todo.back();
                todo.pop_back();
                if ((rc = launch_group(pc.first, pc.second, base, false))) return rc;
                if ((rc = pool_lost(&lost))) return rc;
                if (!lost) continue;
                if (pc.second - pc.first <= 1)
                    return fail(ctx, CM_ELIMIT, "one chaining problem's improvement log does not fit %llu bytes", ctx->dp.pool_bytes);
                const uint32_t mid = pc.first + (pc.second - pc.first) / 2;
                todo.push_back({mid, pc.second});
                todo.push_back({pc.first, mid});
            }
        }
    }
    return CM_OK;
}

int check_dev_err(cm_ctx *ctx) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin + PIN_DEV_ERR, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    const int e = *(const int *)(ctx->h_pin + PIN_DEV_ERR);
    if (e) {
        (void)hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->st.B);       // reported once: the next batch starts clean
        return fail(ctx, CM_ELIMIT, "device capacity limit hit:%s%s%s", (e & cmc::ERR_POOL) ? " chain improvement-log pool exhausted;" : "",
                    (e & (cmc::ERR_SEEDS | cmc::ERR_BAND)) ? " DP string longer than the staging buffer;" : "",
                    (e & cmc::ERR_MEMO) ? " extension memo overflowed where the reference's memo would have served a colliding key" : "");
    }
    return CM_OK;
}

}  // namespace

// ================================================================== C-ABI
extern "C" {

int cm_create(const cm_params *p, cm_ctx **out) {
    if (!p || !out) return CM_EINVAL;
    *out = nullptr;
    const int c = p->kmer - CM_WINDOW_SIZE;
    if (p->kmer < CM_WINDOW_SIZE || c > 8) return CM_EINVAL;
    if (p->max_chain_len < 1 || p->max_chain_len > CM_BESTCHAINLIM) return CM_EINVAL;   // chain.h:14-17 fixed array
    if (p->band < 0 || p->band > cmc::MAX_BAND) return CM_EINVAL;
    if (p->seed_lim < 1 || p->seed_lim > 65535) return CM_EINVAL;
    if (p->max_ed < 0 || p->max_sc < 0 || p->max_read_len < p->kmer) return CM_EINVAL;
    // Five streams of one context work at the same time (seed / chain, heavy chains, pair stage, heavy pairs, H2D staging); the
    // runtime's default of 4 hardware queues makes two of them share one and serialises them.  Only effective when this is the
    // first HIP call of the process; callers that bring up HIP earlier (PyTorch) set the variable themselves (bench.py does).
    // When the variable was not set (or set lower) on entry and something else of this process -- PyTorch, an RCCL communicator --
    // has already brought HIP up, setting it now changes nothing and the schedule runs on the default 4 hardware queues: said
    // once on stderr (CM_QUIET=1 silences it) and left in cm_last_error() of the new context, instead of silently running slower.
    const char *hwq = getenv("GPU_MAX_HW_QUEUES");
    const bool hwq_low = !hwq || atoi(hwq) < 16;
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CM_ENODEV;
    if (p->device < 0 || p->device >= ndev) return CM_ENODEV;
    if (hipSetDevice(p->device) != hipSuccess) return CM_ENODEV;
    cm_ctx *ctx = new cm_ctx();
    ctx->P = *p;
    {
        static std::atomic<unsigned> serial{0};
        ctx->id = ++serial;
    }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    for (const StreamDef &d : STREAMS) {
        hipStream_t *st = &(ctx->st.*d.st);
        if ((d.kind == BLOCKING              ? hipStreamCreate(st)
             : d.kind == NON_BLOCKING_LOWEST ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio_lo)
                                             : hipStreamCreateWithFlags(st, hipStreamNonBlocking)) != hipSuccess) {
            cm_destroy(ctx);
            return CM_EHIP;
        }
    }
    for (hipEvent_t &e : ctx->ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            cm_destroy(ctx);
            return CM_EHIP;
        }
    if (ensure(ctx, ctx->d_pool_cursor, 2 * sizeof(unsigned long long)) != hipSuccess ||
        ensure(ctx, ctx->d_err, sizeof(int)) != hipSuccess ||
        ensure(ctx, ctx->d_counters, CN_WORDS * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc((void **)&ctx->h_pin, PIN_BYTES, hipHostMallocDefault) != hipSuccess) {
        cm_destroy(ctx);
        return CM_ENOMEM;
    }
    memset(ctx->h_pin, 0, PIN_BYTES);
    (void)hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->st.B);
    (void)hipMemsetAsync(ctx->d_counters, 0, CN_WORDS * sizeof(unsigned long long), ctx->st.B);
    if (hwq_low) {
        ctx->err = "note: GPU_MAX_HW_QUEUES was " + std::string(hwq ? hwq : "unset") +
                   " when this context was created; if HIP was initialised earlier in this process the seven streams of a context share the "
                   "default 4 hardware queues (pipelined rounds run slower). Export GPU_MAX_HW_QUEUES=16 before the first HIP call.";
        static std::atomic<bool> said{false};
        if (hwq && !said.exchange(true) && !getenv("CM_QUIET")) fprintf(stderr, "[cmhot] %s\n", ctx->err.c_str());
    }
    *out = ctx;
    return CM_OK;
}

void cm_destroy(cm_ctx *ctx) {
    if (!ctx) return;
    report_hip(ctx, "hipSetDevice", hipSetDevice(ctx->P.device));
    // Every stream of the context is drained, and its status looked at, before anything it could still touch is released: an
    // asynchronous error of this context's work is reported here, under this context's id, instead of surfacing as an abort in
    // whichever context uses the device next.
    for (const StreamDef &d : STREAMS)
        if (ctx->st.*d.st) report_hip(ctx, (std::string("hipStreamSynchronize(") + d.name + ")").c_str(), hipStreamSynchronize(ctx->st.*d.st));
    report_hip(ctx, "hipGetLastError at teardown", hipGetLastError());
    for (auto e : ctx->ev_free) report_hip(ctx, "hipEventDestroy", hipEventDestroy(e));
    ctx->ev_free.clear();
    for (auto &r : ctx->recs) {
        report_hip(ctx, "hipEventDestroy", hipEventDestroy(r.a));
        report_hip(ctx, "hipEventDestroy", hipEventDestroy(r.b));
    }
    ctx->recs.clear();
    free_reads(ctx);
    for (auto &s : ctx->slots) {
        free_all(ctx, s.idx_allocs);
        free_all(ctx, s.ann_allocs);
        drop_entry_near(ctx, s);
    }
    release(ctx, CONTEXT);                 // (the grow-only output staging of cm_collect_* outlives a batch)
    report_hip(ctx, "hipFree (stage 2 chain workspace)", cc_ws_release(ctx->circ_ws));
    if (ctx->h_pin) report_hip(ctx, "hipHostFree", hipHostFree(ctx->h_pin));
    for (hipEvent_t e : ctx->ev)
        if (e) report_hip(ctx, "hipEventDestroy", hipEventDestroy(e));
    for (const StreamDef &d : STREAMS)
        if (ctx->st.*d.st) report_hip(ctx, "hipStreamDestroy", hipStreamDestroy(ctx->st.*d.st));
    delete ctx;
}

const char *cm_last_error(const cm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// Slot::entry_near of a slot whose index and annotation are both in place (else nothing); synchronises ctx->st.B
static int make_entry_near(cm_ctx *ctx, Slot &s) {
    drop_entry_near(ctx, s);
    if (!s.loaded || !s.has_annot || s.X.n_entries == 0) return CM_OK;
    if (s.X.ref_len > 0x80000000u) return CM_OK;          // k_chain_heavy carries the bit in bit 31 of a position
    const uint64_t n = s.X.n_entries;
    uint64_t *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)((n + 63) / 64) * sizeof(uint64_t)) != hipSuccess) {      // not enough HBM: the kernel reads the position bitset
        (void)hipGetLastError();
        return CM_OK;
    }
    s.entry_near = d;
    hipLaunchKernelGGL(k_entry_near, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, s.X.pos, n, s.A.near_border_bits, (uint64_t)s.A.n_bits, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st.B);
    if (e != hipSuccess) drop_entry_near(ctx, s);          // (the caller gives the slot up)
    HIPCHK(ctx, e);
    return CM_OK;
}

// bucket descriptors + the final synchronisation of a contig load (s.X holds the device arrays)
static int finish_contig(cm_ctx *ctx, Slot &s) {
    const size_t nb = ((size_t)1 << (2 * CM_WINDOW_SIZE)) + 1;
    s.d_desc = nullptr;
    static const bool use_desc = !(getenv("CM_SEED_DESC") && getenv("CM_SEED_DESC")[0] == '0');
    if (use_desc) {          // 16 bytes per bucket (4 GiB per contig): a probe becomes one random read instead of two dependent ones
        const uint64_t n_buckets = nb - 1;
        uint32_t *d = nullptr;
        if (hipMalloc((void **)&d, n_buckets * cmc::DESC_WORDS * sizeof(uint32_t)) == hipSuccess) {
            s.idx_allocs.push_back(d);
            hipLaunchKernelGGL(k_build_desc, dim3((unsigned)((n_buckets + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, s.X.bucket_off, s.X.checksum, n_buckets,
                               ctx->P.kmer, d);
            HIPCHK(ctx, hipGetLastError());
            s.d_desc = d;
        } else (void)hipGetLastError();      // not enough HBM: probes go through the arrays
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    s.loaded = true;
    return make_entry_near(ctx, s);
}

int cm_load_contig(cm_ctx *ctx, int slot, const cm_index_view *iv) {
    if (!ctx || !iv) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (!iv->genome || !iv->bucket_off || !iv->checksum || !iv->pos) return fail(ctx, CM_EINVAL, "null index array");
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    Slot &s = ctx->slots[slot];
    free_all(ctx, s.idx_allocs);
    drop_entry_near(ctx, s);
    s.d_desc = nullptr;
    s.loaded = false;
    ++s.gen;
    const size_t nb = ((size_t)1 << (2 * CM_WINDOW_SIZE)) + 1;
    s.X = *iv;
    int rc;
    {   // genome with CM_STAGE_PAD readable bytes on both sides (vector loads of the DP staging over-read)
        uint8_t *g = nullptr;
        const size_t pad = cmc::CM_STAGE_PAD;
        HIPCHK(ctx, hipMalloc((void **)&g, (size_t)iv->ref_len + 2 * pad));
        s.idx_allocs.push_back(g);
        HIPCHK(ctx, hipMemsetAsync(g, 0, (size_t)iv->ref_len + 2 * pad, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(g + pad, iv->genome, (size_t)iv->ref_len, hipMemcpyHostToDevice, ctx->st.B));
        s.X.genome = g + pad;
    }
    if ((rc = up(ctx, s.idx_allocs, iv->bucket_off, nb, &s.X.bucket_off))) return rc;
    if ((rc = up(ctx, s.idx_allocs, iv->checksum, (size_t)iv->n_entries, &s.X.checksum))) return rc;
    if ((rc = up(ctx, s.idx_allocs, iv->pos, (size_t)iv->n_entries, &s.X.pos))) return rc;
    return finish_contig(ctx, s);
}

// exclusive (or inclusive) scan of n uint32 items on stream st; tmp: (n / S32_B + 2) words
static int scan32_on(cm_ctx *ctx, hipStream_t st, const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *tmp, uint32_t add, int inclusive) {
    const uint32_t nb = (uint32_t)((n + S32_B - 1) / S32_B);
    if (nb == 0) return CM_OK;
    hipLaunchKernelGGL(k_scan32_a, dim3(nb), dim3(S32_T), 0, st, in, n, out, tmp, add, inclusive);
    hipLaunchKernelGGL((k_scan_mid<uint32_t, false>), dim3(1), dim3(1024), 0, st, tmp, nb, (uint32_t *)nullptr, (const unsigned int *)nullptr);
    hipLaunchKernelGGL(k_scan32_c, dim3(nb), dim3(S32_T), 0, st, out, n, (const uint32_t *)tmp);
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}
// ... on the main stream (the index loaders)
static int scan32(cm_ctx *ctx, const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *tmp, uint32_t add, int inclusive) {
    return scan32_on(ctx, ctx->st.B, in, n, out, tmp, add, inclusive);
}

int cm_load_contig_raw(cm_ctx *ctx, int slot, const cm_index_raw *raw) {
    if (!ctx || !raw) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (!raw->genome || (raw->n_buckets && (!raw->hv || !raw->count14 || !raw->table))) return fail(ctx, CM_EINVAL, "null array in the raw record");
    if (raw->table_slots > 0xffffffffull) return fail(ctx, CM_ELIMIT, "table of %llu slots", (unsigned long long)raw->table_slots);
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    Slot &s = ctx->slots[slot];
    free_all(ctx, s.idx_allocs);
    drop_entry_near(ctx, s);
    s.d_desc = nullptr;
    s.loaded = false;
    ++s.gen;
    const uint64_t n_all = (uint64_t)1 << (2 * CM_WINDOW_SIZE);
    const uint32_t n_b = raw->n_buckets;
    s.X = cm_index_view{};
    s.X.contig_num = raw->contig_num;
    s.X.ref_len = raw->ref_len;
    int rc;
    {
        uint8_t *g = nullptr;
        const size_t pad = cmc::CM_STAGE_PAD;
        HIPCHK(ctx, hipMalloc((void **)&g, (size_t)raw->ref_len + 2 * pad));
        s.idx_allocs.push_back(g);
        HIPCHK(ctx, hipMemsetAsync(g, 0, (size_t)raw->ref_len + 2 * pad, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(g + pad, raw->genome, (size_t)raw->ref_len, hipMemcpyHostToDevice, ctx->st.B));
        s.X.genome = g + pad;
    }
    // temporaries: the table as in the file, the bucket list, the table offset of every bucket, scan block sums
    std::vector<void *> tmp;
    struct FreeTmp {
        cm_ctx *c;
        std::vector<void *> &v;
        ~FreeTmp() { free_all(c, v); }
    } free_tmp{ctx, tmp};
    const RawEntry *d_tab = nullptr;
    const uint32_t *d_hv = nullptr, *d_cnt = nullptr;
    if ((rc = up(ctx, tmp, (const RawEntry *)raw->table, (size_t)raw->table_slots, &d_tab))) return rc;
    if ((rc = up(ctx, tmp, raw->hv, (size_t)n_b, &d_hv))) return rc;
    if ((rc = up(ctx, tmp, raw->count14, (size_t)n_b, &d_cnt))) return rc;
    uint32_t *d_start = nullptr, *d_bs = nullptr, *d_off = nullptr;
    int *d_bad = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_start, ((size_t)n_b + 1) * sizeof(uint32_t)));
    tmp.push_back(d_start);
    HIPCHK(ctx, hipMalloc((void **)&d_bs, ((size_t)(n_all / S32_B) + 4) * sizeof(uint32_t)));
    tmp.push_back(d_bs);
    HIPCHK(ctx, hipMalloc((void **)&d_bad, sizeof(int)));
    tmp.push_back(d_bad);
    HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), ctx->st.B));
    HIPCHK(ctx, hipMalloc((void **)&d_off, (n_all + 1) * sizeof(uint32_t)));
    s.idx_allocs.push_back(d_off);
    HIPCHK(ctx, hipMemsetAsync(d_off, 0, (n_all + 1) * sizeof(uint32_t), ctx->st.B));
    if ((rc = scan32(ctx, d_cnt, n_b, d_start, d_bs, 1u, 0))) return rc;                 // slot of every bucket's header
    if (n_b) {
        hipLaunchKernelGGL(k_raw_counts, dim3((n_b + BLK - 1) / BLK), dim3(BLK), 0, ctx->st.B, d_tab, (const uint32_t *)d_start, d_hv, d_cnt, n_b, n_all, d_off, d_bad);
        HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = scan32(ctx, d_off, n_all + 1, d_off, d_bs, 0u, 1))) return rc;             // counts -> bucket offsets, in place
    unsigned long long landing[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(&landing[0], d_off + n_all, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipMemcpyAsync(&landing[1], d_bad, sizeof(int), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    if ((int)landing[1]) return fail(ctx, CM_EINVAL, "malformed index table: a bucket header is out of range");
    const uint64_t total = (uint32_t)landing[0];
    uint16_t *d_cs = nullptr;
    uint32_t *d_ps = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_cs, (total ? total : 1) * sizeof(uint16_t)));
    s.idx_allocs.push_back(d_cs);
    HIPCHK(ctx, hipMalloc((void **)&d_ps, (total ? total : 1) * sizeof(uint32_t)));
    s.idx_allocs.push_back(d_ps);
    if (n_b) {
        hipLaunchKernelGGL(k_raw_scatter, dim3((n_b + BLK - 1) / BLK), dim3(BLK), 0, ctx->st.B, d_tab, (const uint32_t *)d_start, d_hv, n_b, (const uint32_t *)d_off, d_cs, d_ps);
        HIPCHK(ctx, hipGetLastError());
    }
    s.X.bucket_off = d_off;
    s.X.checksum = d_cs;
    s.X.pos = d_ps;
    s.X.n_entries = total;
    return finish_contig(ctx, s);       // (synchronises the stream: the temporaries may go)
}

// The ordering passes of cm_build_contig on ctx->st.B; st_host receives the IB_ST_* words.  Temporaries go on `tmp`.
static int ib_order(cm_ctx *ctx, const uint32_t *d_off, uint16_t *d_cs, uint32_t *d_ps, uint64_t total, uint32_t *d_bs, std::vector<void *> &tmp,
                    unsigned long long st_host[IB_ST_WORDS], size_t *tmp_bytes) {
    const uint64_t n_all = (uint64_t)1 << (2 * CM_WINDOW_SIZE);
    // test / diagnostic knobs: smaller thresholds send small inputs down the workgroup and oversize paths
    static const uint32_t wg_lim = std::max<uint32_t>(1u, std::min<uint32_t>(getenv("CM_IB_WG_MAX") ? (uint32_t)atoi(getenv("CM_IB_WG_MAX")) : cmib::WG_MAX, IB_WG_CAP));
    static const uint32_t lane_max = std::max<uint32_t>(1u, std::min<uint32_t>(getenv("CM_IB_LANE_MAX") ? (uint32_t)atoi(getenv("CM_IB_LANE_MAX")) : cmib::LANE_MAX, wg_lim));
    unsigned long long *d_st = nullptr;
    uint32_t *d_med = nullptr, *d_over = nullptr;
    const size_t med_cap = (size_t)(total / ((uint64_t)lane_max + 1)) + 1, over_cap = (size_t)(total / ((uint64_t)wg_lim + 1)) + 1;
    HIPCHK(ctx, hipMalloc((void **)&d_st, IB_ST_WORDS * sizeof(unsigned long long)));
    tmp.push_back(d_st);
    HIPCHK(ctx, hipMalloc((void **)&d_med, med_cap * sizeof(uint32_t)));
    tmp.push_back(d_med);
    HIPCHK(ctx, hipMalloc((void **)&d_over, over_cap * sizeof(uint32_t)));
    tmp.push_back(d_over);
    *tmp_bytes += (med_cap + over_cap) * sizeof(uint32_t);
    HIPCHK(ctx, hipMemsetAsync(d_st, 0, IB_ST_WORDS * sizeof(unsigned long long), ctx->st.B));
    hipLaunchKernelGGL(k_ib_order_lane, dim3((unsigned)(n_all / BLK)), dim3(BLK), 0, ctx->st.B, d_off, n_all, d_cs, d_ps, lane_max, wg_lim, d_med, d_over, d_st);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(st_host, d_st, IB_ST_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    const uint32_t n_med = (uint32_t)st_host[IB_ST_NMED], n_over = (uint32_t)st_host[IB_ST_NOVER];
    if (n_med) {
        hipLaunchKernelGGL(k_ib_order_wg, dim3(std::min<uint32_t>(n_med, 1u << 16)), dim3(BLK), 0, ctx->st.B, d_off, (const uint32_t *)d_med, n_med, d_cs, d_ps);
        HIPCHK(ctx, hipGetLastError());
    }
    if (!n_over) return CM_OK;
    // oversize buckets: all entries of a chunk of the list (up to 2^16 buckets) in one radix sort of 64-bit keys
    uint32_t *d_start = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_start, ((size_t)n_over + 1) * sizeof(uint32_t)));
    tmp.push_back(d_start);
    HIPCHK(ctx, hipMemsetAsync(d_start + n_over, 0, sizeof(uint32_t), ctx->st.B));
    hipLaunchKernelGGL(k_ib_over_sizes, dim3((n_over + BLK - 1) / BLK), dim3(BLK), 0, ctx->st.B, d_off, (const uint32_t *)d_over, n_over, d_start);
    int rc;
    if ((rc = scan32(ctx, d_start, (uint64_t)n_over + 1, d_start, d_bs, 0u, 0))) return rc;          // exclusive, in place: start[n_over] = all oversize entries
    std::vector<uint32_t> start((size_t)n_over + 1);
    HIPCHK(ctx, hipMemcpyAsync(start.data(), d_start, start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    auto rank_bits_of = [](uint32_t n_ranks) {
        unsigned b = 1;
        while ((1u << b) < n_ranks) ++b;
        return b;
    };
    uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
    void *d_sort = nullptr;
    uint32_t largest = 0;
    size_t sort_bytes = 0;
    for (uint32_t r0 = 0; r0 < n_over; r0 += cmib::OVER_CHUNK) {           // the largest chunk and the most sort workspace any chunk asks for
        const uint32_t r1 = std::min(n_over, r0 + cmib::OVER_CHUNK), m = start[r1] - start[r0];
        size_t need = 0;
        HIPCHK(ctx, rocprim::radix_sort_keys(nullptr, need, d_k0, d_k1, (size_t)m, 0u, 48u + rank_bits_of(r1 - r0), ctx->st.B));
        largest = std::max(largest, m);
        sort_bytes = std::max(sort_bytes, need);
    }
    HIPCHK(ctx, hipMalloc((void **)&d_k0, (size_t)largest * sizeof(uint64_t)));
    tmp.push_back(d_k0);
    HIPCHK(ctx, hipMalloc((void **)&d_k1, (size_t)largest * sizeof(uint64_t)));
    tmp.push_back(d_k1);
    HIPCHK(ctx, hipMalloc(&d_sort, sort_bytes ? sort_bytes : 1));
    tmp.push_back(d_sort);
    *tmp_bytes += 2 * (size_t)largest * sizeof(uint64_t) + sort_bytes + ((size_t)n_over + 1) * sizeof(uint32_t);
    for (uint32_t r0 = 0; r0 < n_over; r0 += cmib::OVER_CHUNK) {
        const uint32_t r1 = std::min(n_over, r0 + cmib::OVER_CHUNK), m = start[r1] - start[r0];
        const unsigned rank_bits = rank_bits_of(r1 - r0);
        size_t have = sort_bytes;
        const dim3 grid(std::min<uint32_t>(r1 - r0, 1u << 16));
        hipLaunchKernelGGL(k_ib_over_pack, grid, dim3(BLK), 0, ctx->st.B, d_off, (const uint32_t *)d_over, (const uint32_t *)d_start, r0, r1, (const uint16_t *)d_cs,
                           (const uint32_t *)d_ps, d_k0);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, rocprim::radix_sort_keys(d_sort, have, d_k0, d_k1, (size_t)m, 0u, 48u + rank_bits, ctx->st.B));
        hipLaunchKernelGGL(k_ib_over_unpack, grid, dim3(BLK), 0, ctx->st.B, d_off, (const uint32_t *)d_over, (const uint32_t *)d_start, r0, r1, (const uint64_t *)d_k1,
                           d_cs, d_ps);
        HIPCHK(ctx, hipGetLastError());
    }
    return CM_OK;
}

static int build_contig_arrays(cm_ctx *ctx, Slot &s, const uint8_t *genome, uint32_t ref_len, cm_build_stats *stats, hipEvent_t ev_a, hipEvent_t ev_b) {
    const uint64_t n_all = (uint64_t)1 << (2 * CM_WINDOW_SIZE);
    const int k = ctx->P.kmer, c = k - CM_WINDOW_SIZE;
    {
        uint8_t *g = nullptr;
        const size_t pad = cmc::CM_STAGE_PAD;
        HIPCHK(ctx, hipMalloc((void **)&g, (size_t)ref_len + 2 * pad));
        s.idx_allocs.push_back(g);
        HIPCHK(ctx, hipMemsetAsync(g, 0, (size_t)ref_len + 2 * pad, ctx->st.B));
        if (ref_len) HIPCHK(ctx, hipMemcpyAsync(g + pad, genome, (size_t)ref_len, hipMemcpyHostToDevice, ctx->st.B));
        s.X.genome = g + pad;
    }
    std::vector<void *> tmp;
    struct FreeTmp {
        cm_ctx *c;
        std::vector<void *> &v;
        ~FreeTmp() { free_all(c, v); }
    } free_tmp{ctx, tmp};
    size_t tmp_bytes = ((size_t)(n_all / S32_B) + 4) * sizeof(uint32_t);
    uint32_t *d_bs = nullptr, *d_off = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_bs, tmp_bytes));
    tmp.push_back(d_bs);
    HIPCHK(ctx, hipMalloc((void **)&d_off, (n_all + 1) * sizeof(uint32_t)));
    s.idx_allocs.push_back(d_off);
    HIPCHK(ctx, hipEventRecord(ev_a, ctx->st.B));
    HIPCHK(ctx, hipMemsetAsync(d_off, 0, (n_all + 1) * sizeof(uint32_t), ctx->st.B));
    // the number of entries is at most ref_len - k + 1 < 2^32: the 32-bit counters and scans cannot overflow
    const uint32_t n_pos = ref_len >= (uint32_t)k ? ref_len - (uint32_t)k + 1u : 0u;
    const dim3 pgrid((unsigned)(((uint64_t)n_pos + IB_TILE - 1) / IB_TILE));
    if (n_pos) {
        hipLaunchKernelGGL(k_ib_positions<false>, pgrid, dim3(BLK), 0, ctx->st.B, s.X.genome, ref_len, n_pos, k, c, d_off, (uint16_t *)nullptr, (uint32_t *)nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    int rc;
    if ((rc = scan32(ctx, d_off, n_all + 1, d_off, d_bs, 0u, 1))) return rc;             // counts -> bucket ends, in place
    uint32_t total32 = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total32, d_off + n_all, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    const uint64_t total = total32;
    if (total > (uint64_t)n_pos) return fail(ctx, CM_ELIMIT, "%llu entries from %u k-mer starts", (unsigned long long)total, n_pos);
    uint16_t *d_cs = nullptr;
    uint32_t *d_ps = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_cs, (total ? total : 1) * sizeof(uint16_t)));
    s.idx_allocs.push_back(d_cs);
    HIPCHK(ctx, hipMalloc((void **)&d_ps, (total ? total : 1) * sizeof(uint32_t)));
    s.idx_allocs.push_back(d_ps);
    unsigned long long st[IB_ST_WORDS] = {0, 0, 0, 0, 0, 0};
    if (total) {
        hipLaunchKernelGGL(k_ib_positions<true>, pgrid, dim3(BLK), 0, ctx->st.B, s.X.genome, ref_len, n_pos, k, c, d_off, d_cs, d_ps);   // ends -> starts
        HIPCHK(ctx, hipGetLastError());
        if ((rc = ib_order(ctx, d_off, d_cs, d_ps, total, d_bs, tmp, st, &tmp_bytes))) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ev_b, ctx->st.B));
    s.X.bucket_off = d_off;
    s.X.checksum = d_cs;
    s.X.pos = d_ps;
    s.X.n_entries = total;
    if ((rc = finish_contig(ctx, s))) return rc;       // (synchronises the stream: the temporaries may go)
    if (stats) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev_a, ev_b));
        memset(stats, 0, sizeof *stats);
        stats->n_entries = total;
        stats->max_bucket = (uint32_t)st[IB_ST_MAX];
        stats->reserved = (uint32_t)std::min<size_t>(tmp_bytes >> 20, 0xffffffffu);      // peak temporary HBM of the build, MiB
        for (int i = 0; i < 3; ++i) stats->buckets_by_path[i] = st[IB_ST_PATH + i];
        stats->ms_device = ms;
    }
    return CM_OK;
}

int cm_build_contig(cm_ctx *ctx, int slot, int32_t contig_num, const uint8_t *genome, uint32_t ref_len, cm_build_stats *stats) {
    if (!ctx) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (!genome && ref_len) return fail(ctx, CM_EINVAL, "null genome");
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    Slot &s = ctx->slots[slot];
    free_all(ctx, s.idx_allocs);
    drop_entry_near(ctx, s);
    s.d_desc = nullptr;
    s.loaded = false;
    ++s.gen;
    s.X = cm_index_view{};
    s.X.contig_num = contig_num;
    s.X.ref_len = ref_len;
    hipEvent_t ev_a = take_event(ctx), ev_b = take_event(ctx);
    if (!ev_a || !ev_b) return fail(ctx, CM_EHIP, "hipEventCreate failed");
    const int rc = build_contig_arrays(ctx, s, genome, ref_len, stats, ev_a, ev_b);
    if (rc != CM_OK) {                                   // the slot stays unloaded and owns nothing
        (void)hipStreamSynchronize(ctx->st.B);
        (void)hipGetLastError();
        free_all(ctx, s.idx_allocs);
        s.d_desc = nullptr;
        s.loaded = false;
        s.X = cm_index_view{};
    }
    ctx->ev_free.push_back(ev_a);
    ctx->ev_free.push_back(ev_b);
    return rc;
}

int cm_index_download(cm_ctx *ctx, int slot, uint32_t *bucket_off, uint16_t *checksum, uint32_t *pos, uint64_t cap_entries, uint64_t *n_entries) {
    if (!ctx) return CM_EINVAL;
    int rc;
    if ((rc = check_slot(ctx, slot, false))) return rc;
    const Slot &s = ctx->slots[slot];
    const uint64_t n = s.X.n_entries;
    if (n_entries) *n_entries = n;
    if (!bucket_off && !checksum && !pos) return CM_OK;
    if ((checksum || pos) && cap_entries < n) return fail(ctx, CM_ELIMIT, "slot %d holds %llu entries, the buffers %llu", slot, (unsigned long long)n, (unsigned long long)cap_entries);
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    const size_t nb = ((size_t)1 << (2 * CM_WINDOW_SIZE)) + 1;
    if (bucket_off) HIPCHK(ctx, hipMemcpyAsync(bucket_off, s.X.bucket_off, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->st.B));
    if (checksum && n) HIPCHK(ctx, hipMemcpyAsync(checksum, s.X.checksum, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->st.B));
    if (pos && n) HIPCHK(ctx, hipMemcpyAsync(pos, s.X.pos, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return CM_OK;
}

int cm_load_annotation(cm_ctx *ctx, int slot, const cm_annot_view *av) {
    if (!ctx || !av) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (av->n_iv == 0 || av->n_chr == 0) return fail(ctx, CM_EINVAL, "annotation needs >= 1 interval and >= 1 chromosome");
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    Slot &s = ctx->slots[slot];
    free_all(ctx, s.ann_allocs);
    drop_entry_near(ctx, s);
    s.has_annot = false;
    ++s.gen;
    cmc::AnnotAosHost aos;
    cmc::build_annot_aos(*av, aos);
    cmc::AnnotDev &A = s.A;
    A = cmc::AnnotDev{};
    A.n_iv = av->n_iv; A.n_seg = av->n_seg; A.n_trans = av->n_trans; A.n_gene = av->n_gene; A.n_chr = av->n_chr; A.n_bits = av->n_bits;
    A.pair_reach = aos.pair_reach;
    int rc;
    auto &al = s.ann_allocs;
    if ((rc = up(ctx, al, aos.iv.data(), aos.iv.size(), &A.iv))) return rc;
    if ((rc = up(ctx, al, av->iv_seg, (size_t)av->iv_seg_off[av->n_iv], &A.iv_seg))) return rc;
    if ((rc = up(ctx, al, aos.seg.data(), aos.seg.size(), &A.seg))) return rc;
    if ((rc = up(ctx, al, av->seg_tid, (size_t)av->seg_tid_off[av->n_seg], &A.seg_tid))) return rc;
    if ((rc = up(ctx, al, aos.tr.data(), aos.tr.size(), &A.tr))) return rc;
    if ((rc = up(ctx, al, av->t2s, (size_t)av->t2s_off[av->n_trans], &A.t2s))) return rc;
    if ((rc = up(ctx, al, aos.gene.data(), aos.gene.size(), &A.gene))) return rc;
    const size_t bit_words = (size_t)((av->n_bits + 63) / 64);      // bit_at() takes any p < n_bits: the last word may be a partial one
    if ((rc = up(ctx, al, av->near_border_bits, bit_words, &A.near_border_bits))) return rc;
    if ((rc = up(ctx, al, av->intronic_bits, bit_words, &A.intronic_bits))) return rc;
    if ((rc = up(ctx, al, av->chr_shift, (size_t)av->n_chr, &A.chr_shift))) return rc;
    if ((rc = up(ctx, al, av->chr_id, (size_t)av->n_chr, &A.chr_id))) return rc;
    if (av->iv_bucket && av->n_iv_bucket >= 2) {
        if ((rc = up(ctx, al, av->iv_bucket, (size_t)av->n_iv_bucket, &A.iv_bucket))) return rc;
        A.iv_bucket_shift = av->iv_bucket_shift;
        A.n_iv_bucket = av->n_iv_bucket;
    }
    // the staging copies are asynchronous: the host vectors must outlive them
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    {   // every window bound upper_bound() can return lies within maxIntronLen of the queried hit (k_chain_heavy)
        const long long mi = ctx->P.max_intron;
        bool ok = mi >= (long long)ctx->P.max_read_len + ctx->P.max_ed && mi < (1ll << 30);
        for (uint32_t i = 0; i < av->n_iv && ok; ++i) {
            if (av->iv_seg_off[i + 1] == av->iv_seg_off[i]) continue;
            const long long far = std::max<long long>((long long)av->iv_max_next_exon[i] + ctx->P.kmer, (long long)av->iv_max_end[i]);
            if (far - (long long)av->iv_spos[i] > mi) ok = false;
        }
        s.chain_parallel_ok = ok;
    }
    s.has_annot = true;
    return make_entry_near(ctx, s);
}

int cm_unload_contig(cm_ctx *ctx, int slot) {
    if (!ctx || slot < 0 || slot >= MAX_SLOTS) return CM_EINVAL;
    (void)hipSetDevice(ctx->P.device);
    (void)hipStreamSynchronize(ctx->st.B);
    free_all(ctx, ctx->slots[slot].idx_allocs);
    free_all(ctx, ctx->slots[slot].ann_allocs);
    drop_entry_near(ctx, ctx->slots[slot]);
    ctx->slots[slot].loaded = ctx->slots[slot].has_annot = false;
    ctx->slots[slot].d_desc = nullptr;
    ++ctx->slots[slot].gen;
    return CM_OK;
}

static int check_seeds(cm_ctx *ctx, int max_len) {
    if (!cmft::too_many_seeds(max_len, ctx->P.kmer, cmc::MAX_SEEDS)) return CM_OK;
    return fail(ctx, CM_ELIMIT, "%d seeds per read > %d supported", max_len / ctx->P.kmer, cmc::MAX_SEEDS);
}

// Validation shared by cm_reads_upload / cm_reads_stage; returns the longest read through *max_len_out.
static int check_reads(cm_ctx *ctx, const cm_reads *rd, int *max_len_out) {
    const uint64_t n = rd->n_pairs;
    if (n > 0x3fffffffull) return fail(ctx, CM_ELIMIT, "more than 2^30 pairs in one batch");
    if (!rd->seq1 || !rd->seq2 || !rd->off1 || !rd->off2) return fail(ctx, CM_EINVAL, "null read arrays");
    const uint64_t lim = (uint64_t)ctx->P.max_read_len;
    uint64_t bad = 0, longest = 0;
    // (2^21 pairs: 1.4 ms on one core, with the GPU idle when the call sits between two batches -- cm_reads_stage; ranges on a few threads)
    auto scan = [&](uint64_t lo, uint64_t hi, uint64_t *bad_o, uint64_t *long_o) {
        uint64_t bd = 0, lg = 0;
        for (uint64_t i = lo; i < hi; ++i) {
            const uint64_t l1 = rd->off1[i + 1] - rd->off1[i], l2 = rd->off2[i + 1] - rd->off2[i];     // wraps to huge when not monotone
            const uint64_t m = l1 > l2 ? l1 : l2;
            if (m > lim && !bd) bd = i + 1;
            if (m > lg) lg = m;
        }
        *bad_o = bd;
        *long_o = lg;
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned n_thr = n < (1u << 18) ? 1u : std::min(8u, hw ? hw : 1u);
    uint64_t bd[8] = {0}, lg[8] = {0};
    std::thread th[8];
    unsigned started = 1;
    try {
        for (; started < n_thr; ++started) th[started] = std::thread(scan, n * started / n_thr, n * (started + 1) / n_thr, &bd[started], &lg[started]);
    } catch (...) {                                       // no more threads to be had: the rest of the ranges on this one
    }
    scan(0, n / n_thr, &bd[0], &lg[0]);
    for (unsigned k = started; k < n_thr; ++k) scan(n * k / n_thr, n * (k + 1) / n_thr, &bd[k], &lg[k]);
    for (unsigned k = 1; k < started; ++k) th[k].join();
    for (unsigned k = 0; k < n_thr; ++k) {
        if (bd[k] && !bad) bad = bd[k];                       // the first offending pair
        if (lg[k] > longest) longest = lg[k];
    }
    if (bad) {
        const uint64_t i = bad - 1;
        if (rd->off1[i + 1] < rd->off1[i] || rd->off2[i + 1] < rd->off2[i]) return fail(ctx, CM_EINVAL, "read offsets not monotone at pair %llu", (unsigned long long)i);
        return fail(ctx, CM_EINVAL, "pair %llu longer than max_read_len %d", (unsigned long long)i, ctx->P.max_read_len);
    }
    *max_len_out = (int)longest;
    return check_seeds(ctx, (int)longest);
}

// Pairs per tile (launch group) of a batch of n pairs.
static uint32_t tile_for(uint64_t n) {
    // A batch is walked in at least two tiles when it has more than 2^20 pairs (round-major order: a tile's seeding then sees the flags
    // its previous pair stage wrote), and the tiles are as large as the batch allows up to 2^21: an item costs 1 - 4 ms beyond what
    // grows with its pairs (tails of the persistent grids, ~40 launches, three host round trips) -- 2^22-pair batches 146.6 ms per step
    // in four tiles, 139.0 in two; 2^21-pair batches 73 ms in two tiles, 96 in four, 77 in one.
    uint32_t tile_cap = TILE_PAIRS;
    if (n > 2ull * TILE_PAIRS) {
        const uint64_t half = ((n + 1) / 2 + 65535) / 65536 * 65536;
        tile_cap = (uint32_t)std::min<uint64_t>(half, TILE_PAIRS_MAX);
    }
    if (const char *e = getenv("CM_TILE_PAIRS")) {       // tuning knob: pairs per launch group
        const long v = atol(e);
        if (v >= 64 && v <= (1l << 24)) tile_cap = (uint32_t)v;
    }
    return (uint32_t)(n < tile_cap ? n : tile_cap);
}

// Per-tile workspace and per-batch state of the batch that is becoming resident (n pairs, longest read max_len).
static int prepare_resident(cm_ctx *ctx, uint64_t n, int max_len) {
    ctx->n_seeds = max_len / ctx->P.kmer;
    ctx->max_len = max_len;
    HIPCHK(ctx, ensure(ctx, ctx->d_state, n * sizeof(cm_mapped_read)));
    HIPCHK(ctx, ensure(ctx, ctx->d_active, n));
    HIPCHK(ctx, ensure(ctx, ctx->d_active_b, n));
    HIPCHK(ctx, ensure(ctx, ctx->d_cat, n * sizeof(int32_t)));
    // workspace for one tile
    const uint32_t tile = tile_for(n);
    ctx->tile = tile;
    const size_t nprob = (size_t)tile * 4, nprobe = nprob * (size_t)(ctx->n_seeds ? ctx->n_seeds : 1);
    for (SeedSet &sd : ctx->seed) {
        HIPCHK(ctx, ensure(ctx, sd.sstart, nprobe * 4));
        HIPCHK(ctx, ensure(ctx, sd.scnt, nprobe * 4));
        HIPCHK(ctx, ensure(ctx, sd.sraw, nprobe * 4));
        HIPCHK(ctx, ensure(ctx, sd.celloff, (nprob + 2) * 8));
        HIPCHK(ctx, ensure(ctx, sd.bmax, (nprob / SCAN_ELEMS + 2) * 4));
        HIPCHK(ctx, ensure(ctx, sd.bsum, (nprob / SCAN_ELEMS + 2) * 8));
        HIPCHK(ctx, ensure(ctx, sd.cctr, CTR_WORDS * sizeof(unsigned int)));
        HIPCHK(ctx, ensure(ctx, sd.cblk, (size_t)N_CLS * (4 * (size_t)tile / CLS_T + 2) * sizeof(unsigned int)));
        HIPCHK(ctx, ensure(ctx, sd.cls4, (size_t)tile * 4));
        HIPCHK(ctx, ensure(ctx, sd.perm4, (size_t)tile * 4 * 4));
        HIPCHK(ctx, ensure(ctx, sd.thigh, (size_t)tile * 4 * sizeof(int32_t)));
    }
    for (ChainRecs &cr : ctx->rec) {
        HIPCHK(ctx, ensure(ctx, cr.chains, nprob * CM_BESTCHAINLIM * sizeof(cm_chain)));
        HIPCHK(ctx, ensure(ctx, cr.nchain, nprob * 4));
        HIPCHK(ctx, ensure(ctx, cr.high, nprob * 4));
        HIPCHK(ctx, ensure(ctx, cr.resid, (size_t)tile * 4 * sizeof(uint16_t)));
    }
    // DP cells: room for 64 cells per problem on average, at least 8M (one worst-case problem is
    // n_seeds * seed_lim cells); larger tiles are split into ranges by run_chain_tile.
    unsigned long long cap = (unsigned long long)nprob * 64ull;
    const unsigned long long worst = (unsigned long long)ctx->P.seed_lim * (unsigned long long)(ctx->n_seeds ? ctx->n_seeds : 1);
    if (cap < (8ull << 20)) cap = 8ull << 20;
    if (cap < worst) cap = worst;
    if (cap > ctx->dp.cells_cap || !ctx->dp.score) ctx->dp.cells_cap = cap;        // grow-only, like the buffers behind it
    HIPCHK(ctx, ensure(ctx, ctx->dp.score, ctx->dp.cells_cap * sizeof(double)));
    HIPCHK(ctx, ensure(ctx, ctx->dp.prev, ctx->dp.cells_cap * sizeof(int32_t)));
    HIPCHK(ctx, ensure(ctx, ctx->sort.cls, (size_t)tile));
    PairSetMem &pm = ctx->pair_mem;           // x 2: one half per set of chain records (run_pair_tile)
    HIPCHK(ctx, ensure(ctx, pm.perm, (size_t)tile * 4 * 2));
    HIPCHK(ctx, ensure(ctx, pm.hlist, (size_t)tile * 4 * 2));
    HIPCHK(ctx, ensure(ctx, ctx->d_hres, (size_t)HEAVY_GRID_MAX * (64 * sizeof(HRes) + HEAVY_SCRATCH)));
    if (heavy_pipeline()) {
        // the pipeline's arrays: per heavy pair, per mate-pair task (~ 10 per heavy pair on the dense workload, room for 6 per pair of
        // the tile), per unpaired chain (room for 4 per pair of the tile); what does not fit goes to k_pair_heavy
        // (CM_HP_TASKS_CAP / CM_HP_UNP_CAP: test knobs, small capacities so that the fall-back path is taken)
        const size_t tc = getenv("CM_HP_TASKS_CAP") ? (size_t)std::max(1, atoi(getenv("CM_HP_TASKS_CAP"))) : std::max<size_t>((size_t)tile * 6, 4096);
        const size_t uc = getenv("CM_HP_UNP_CAP") ? (size_t)std::max(1, atoi(getenv("CM_HP_UNP_CAP"))) : std::max<size_t>((size_t)tile * 4, 4096);
        ctx->hp.tasks_cap = (uint32_t)tc;
        ctx->hp.unp_cap = (uint32_t)uc;
        HIPCHK(ctx, ensure(ctx, ctx->hp.pairs, (size_t)tile * sizeof(HPair)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.list2, (size_t)tile * 4));
        HIPCHK(ctx, ensure(ctx, pm.hp_fall, (size_t)tile * 4 * 2));
        HIPCHK(ctx, ensure(ctx, pm.hp_fallctr, 2 * sizeof(unsigned int)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.T, tc * sizeof(HTask)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.tcls, tc));
        HIPCHK(ctx, ensure(ctx, ctx->hp.tperm, tc * 4));
        HIPCHK(ctx, ensure(ctx, ctx->hp.tblk, (size_t)N_CLS * (tc / CLS_T + 2) * sizeof(unsigned int)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.tctr, CTR_WORDS * sizeof(unsigned int)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.pre, tc * 4 * sizeof(cmc::PreDP)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.q, tc * 4 * 4));
        HIPCHK(ctx, ensure(ctx, ctx->hp.res, tc * sizeof(HRes)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.U, uc * sizeof(HUnp)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.pre2, uc * 2 * sizeof(cmc::PreDP)));
        HIPCHK(ctx, ensure(ctx, ctx->hp.q2, uc * 2 * 4));
        HIPCHK(ctx, ensure(ctx, ctx->hp.lists, (size_t)HP_PLAN_GRID * HEAVY_LIST * 2));
        HIPCHK(ctx, ensure(ctx, ctx->hp.ctr, HC_WORDS * sizeof(unsigned int)));
    }
    {
        const uint32_t *before = pm.pair_err;
        HIPCHK(ctx, ensure(ctx, pm.pair_err, (size_t)tile * 4 * 2));      // one set per set of chain records (run_pair_tile)
        if (pm.pair_err != before) HIPCHK(ctx, hipMemsetAsync(pm.pair_err, 0, (size_t)tile * 4 * 2, ctx->st.P));   // the kernels keep it zero
    }
    HIPCHK(ctx, ensure(ctx, pm.retry_list, (size_t)tile * 4 * 2));
    HIPCHK(ctx, ensure(ctx, pm.retry_ctr, 4 * sizeof(unsigned int)));
    HIPCHK(ctx, ensure(ctx, ctx->d_heavy_load, sizeof(unsigned long long)));
    HIPCHK(ctx, ensure(ctx, ctx->d_spill, (size_t)RETRY_GRID * BLK_PAIR * RETRY_SPILL * sizeof(cmc::MemoSpill)));
    HIPCHK(ctx, ensure(ctx, pm.cls_ctr, 2 * CTR_WORDS * sizeof(unsigned int)));
    HIPCHK(ctx, ensure(ctx, ctx->sort.ctr2, CTR_WORDS * sizeof(unsigned int)));
    HIPCHK(ctx, ensure(ctx, ctx->sort.sub, (size_t)tile));
    HIPCHK(ctx, ensure(ctx, ctx->sort.perm1, (size_t)tile * 4));
    HIPCHK(ctx, ensure(ctx, ctx->sort.ctr3, CTR_WORDS * sizeof(unsigned int)));
    HIPCHK(ctx, ensure(ctx, ctx->sort.sub2, (size_t)tile));
    HIPCHK(ctx, ensure(ctx, ctx->sort.perm0, (size_t)tile * 4));
    HIPCHK(ctx, ensure(ctx, ctx->sort.blk_cnt, (size_t)N_CLS * (4 * (size_t)tile / CLS_T + 2) * sizeof(unsigned int)));
    if (getenv("CM_LANE_CLK")) {
#if defined(CM_DIAG)
        const size_t clk_words = 16 * 2 + 1;  // per-pair rows + wave-level rows of k_pair and k_pair_heavy (diag)
#else
        const size_t clk_words = 1;
#endif
        HIPCHK(ctx, ensure(ctx, ctx->d_lane_clk, n * 8 * clk_words));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_lane_clk, 0, n * 8 * clk_words, ctx->st.B));
    }
    unsigned long long pool = (unsigned long long)nprob * 2048ull;       // improvement log
    if (pool < (256ull << 20)) pool = 256ull << 20;
    if (pool > (8ull << 30)) pool = 8ull << 30;
    if (const char *e = getenv("CM_POOL_BYTES")) {       // test knob: start with a small log pool to exercise the recovery path
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 4096 && !ctx->dp.pool) pool = v;
    }
    if (pool > ctx->dp.pool_bytes || !ctx->dp.pool) ctx->dp.pool_bytes = pool;
    HIPCHK(ctx, ensure(ctx, ctx->dp.pool, ctx->dp.pool_bytes));
    for (int b = 0; b < 2; ++b) {             // set b: the b-th half (the only place that cuts them)
        const size_t at = (size_t)b * tile;
        ctx->pset[b] = PairSet{pm.perm + at,       pm.hlist + at,      pm.cls_ctr + (size_t)b * CTR_WORDS,
                               pm.pair_err + at,   pm.retry_list + at, pm.retry_ctr + 2 * b,       // [count, cursor]
                               pm.hp_fall ? pm.hp_fall + at : nullptr, pm.hp_fallctr ? pm.hp_fallctr + b : nullptr};
    }
    return CM_OK;
}

// Copies of one batch into (grow-only) read buffers on stream `st`: only the CM_STAGE_PAD slack around the reads is
// cleared (cmc::stage over-reads into it), the reads themselves are overwritten by the copy.
static int copy_reads(cm_ctx *ctx, const cm_reads *rd, hipStream_t st, ReadBufs &to) {
    const uint64_t n = rd->n_pairs;
    const uint8_t *const seq[2] = {rd->seq1, rd->seq2};
    const uint64_t *const off[2] = {rd->off1, rd->off2};
    const size_t bytes[2] = {(size_t)off[0][n] - (size_t)off[0][0], (size_t)off[1][n] - (size_t)off[1][0]};
    if (off[0][0] != 0 || off[1][0] != 0) return fail(ctx, CM_EINVAL, "read offsets must start at 0");
    const size_t pad = cmc::CM_STAGE_PAD;                  // readable slack around the reads (see cmc::stage)
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, ensure(ctx, to.file[f].seq_base, bytes[f] + 2 * pad));
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, ensure(ctx, to.file[f].off, (n + 1) * sizeof(uint64_t)));
    for (int f = 0; f < 2; ++f) {
        HIPCHK(ctx, hipMemsetAsync(to.file[f].seq_base, 0, pad, st));
        HIPCHK(ctx, hipMemsetAsync(to.file[f].seq_base + pad + bytes[f], 0, pad, st));
    }
    for (int f = 0; f < 2; ++f)
        if (bytes[f]) HIPCHK(ctx, hipMemcpyAsync(to.file[f].seq(), seq[f], bytes[f], hipMemcpyHostToDevice, st));
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, hipMemcpyAsync(to.file[f].off, off[f], (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    return CM_OK;
}

// A batch of n pairs becomes resident (cm_reads_upload, cm_reads_swap; n_pairs is 0 here and stays 0 on failure).  `after`: what the
// main stream waits for first; `prior`: the carried states, the caller's on the host or the staged record's on the device (`kind`).
static int make_resident(cm_ctx *ctx, uint64_t n, int max_len, hipEvent_t after, const cm_mapped_read *prior, hipMemcpyKind kind) {
    if (int rc = prepare_resident(ctx, n, max_len)) return rc;
    ctx->n_pairs = n;
    if (after) HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, after, 0));
    KCore k{};
    k.P = ctx->P;
    hipLaunchKernelGGL(k_init_state, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, k, ctx->d_state, ctx->d_active, ctx->d_cat, n);
    // carried states: a pair is active unless the caller marks it retired by type < 0 (never produced by this library)
    if (prior) HIPCHK(ctx, hipMemcpyAsync(ctx->d_state, prior, n * sizeof(cm_mapped_read), kind, ctx->st.B));
    return CM_OK;
}

int cm_reads_upload(cm_ctx *ctx, const cm_reads *rd, const cm_mapped_read *prior) {
    if (!ctx || !rd) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    const uint64_t n = rd->n_pairs;
    ctx->pre_ready = false;                        // a prefetched first round belonged to a batch that came in through cm_reads_swap
    ctx->n_pairs = 0;
    ctx->tile = 0;
    if (n == 0) {                                  // an empty batch releases the per-batch buffers
        free_reads(ctx);
        return CM_OK;
    }
    int max_len = 0, rc = check_reads(ctx, rd, &max_len);
    if (rc) return rc;
    ctx->rd.keep_nothing();
    if ((rc = copy_reads(ctx, rd, ctx->st.B, ctx->rd)) || (rc = make_resident(ctx, n, max_len, nullptr, prior, hipMemcpyHostToDevice))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return CM_OK;
}

// A stage opens behind the copy stream: an earlier staged batch that was never swapped in is dropped (refusals for the arguments come first)
static int stage_open(cm_ctx *ctx) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.C));
    ctx->staged.reset();
    ctx->pre_launched = false;
    return CM_OK;
}

int cm_reads_stage(cm_ctx *ctx, const cm_reads *rd, const cm_mapped_read *prior) {
    if (!ctx || !rd) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (rd->n_pairs == 0) return fail(ctx, CM_EINVAL, "cm_reads_stage: empty batch");
    int max_len = 0, rc = check_reads(ctx, rd, &max_len);
    if (rc || (rc = stage_open(ctx)) || (rc = copy_reads(ctx, rd, ctx->st.C, ctx->staged.rd))) return rc;
    if (prior) {
        HIPCHK(ctx, ensure(ctx, ctx->staged.prior, rd->n_pairs * sizeof(cm_mapped_read)));
        HIPCHK(ctx, hipMemcpyAsync(ctx->staged.prior, prior, rd->n_pairs * sizeof(cm_mapped_read), hipMemcpyHostToDevice, ctx->st.C));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev.staged, ctx->st.C));
    ctx->staged.commit(rd->n_pairs, max_len, prior != nullptr);
    return CM_OK;
}

// The steps of cm_reads_stage_text (below), in its order.  First the staged read buffers and the tokeniser's own, sized by the plan; the
// result block cleared, the two blocks on their way.
static int ft_begin(cm_ctx *ctx, const cmft::Sizes &S, const uint8_t *const text[2], const uint64_t len[2]) {
    TextStage &T = ctx->ft;
    const size_t words = (size_t)S.nb + 1;
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, ensure(ctx, ctx->staged.rd.file[f].seq_base, len[f] + 2 * cmc::CM_STAGE_PAD));
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, ensure(ctx, ctx->staged.rd.file[f].off, words * sizeof(uint64_t)));
    HIPCHK(ctx, ensure(ctx, T.res, cmft::RES_WORDS * sizeof(unsigned long long)));
    for (int f = 0; f < 2; ++f) {
        HIPCHK(ctx, ensure(ctx, T.text[f], (len[f] + 15) / 16 * 16 + cmft::TEXT_SLACK));
        HIPCHK(ctx, ensure(ctx, T.cnt[f], ((size_t)S.n_chunks[f] + 1) * sizeof(uint32_t)));
        HIPCHK(ctx, ensure(ctx, T.ls[f], (size_t)S.ls_cap[f] * sizeof(uint32_t)));
        HIPCHK(ctx, ensure(ctx, T.slen[f], words * sizeof(uint32_t)));
        HIPCHK(ctx, ensure(ctx, T.rec[f], words * sizeof(uint64_t)));
    }
    HIPCHK(ctx, ensure(ctx, T.tmp, (size_t)(S.scan_items / S32_B + 2) * sizeof(uint32_t)));
    HIPCHK(ctx, hipMemsetAsync(T.res, 0xff, 2 * sizeof(unsigned long long), ctx->st.C));                   // RES_BAD1, RES_BAD2: none
    HIPCHK(ctx, hipMemsetAsync(T.res + cmft::RES_MAX_LEN, 0, sizeof(unsigned long long), ctx->st.C));
    for (int f = 0; f < 2; ++f)
        if (len[f]) HIPCHK(ctx, hipMemcpyAsync(T.text[f], text[f], len[f], hipMemcpyHostToDevice, ctx->st.C));
    return CM_OK;
}
// lines of both files (counts, scan, line starts), then their records (verdicts + lengths, scan, offsets, the bases), the result block
static int ft_tokenise(cm_ctx *ctx, const cmft::Sizes &S, const FtShape &sh, const uint64_t len[2]) {
    TextStage &T = ctx->ft;
    const ReadFile *to = ctx->staged.rd.file;
    hipStream_t st = ctx->st.C;
    for (int f = 0; f < 2; ++f) {
        const uint32_t nc = S.n_chunks[f];
        hipLaunchKernelGGL(k_ft_count, dim3(nc / FT_WAVES + 1), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], len[f], nc, (uint32_t *)T.cnt[f]);
        if (int rc = scan32_on(ctx, st, T.cnt[f], (uint64_t)nc + 1, T.cnt[f], T.tmp, 0u, 0)) return rc;
        hipLaunchKernelGGL(k_ft_lines, dim3((nc + FT_WAVES - 1) / FT_WAVES + 1), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], len[f], nc, (const uint32_t *)T.cnt[f],
                           S.trail[f], (uint32_t *)T.ls[f], S.ls_cap[f]);
    }
    for (int f = 0; f < 2; ++f) {
        const unsigned gb = S.nb / FT_T + 1;                  // covers i = 0 .. S.nb
        hipLaunchKernelGGL(k_ft_records, dim3(gb), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], (const uint32_t *)T.ls[f], sh, f, S.nb, (uint32_t *)T.slen[f],
                           (unsigned long long *)T.res);
        if (int rc = scan32_on(ctx, st, T.slen[f], (uint64_t)S.nb + 1, T.slen[f], T.tmp, 0u, 0)) return rc;
        hipLaunchKernelGGL(k_ft_offsets, dim3(gb), dim3(FT_T), 0, st, (const uint32_t *)T.ls[f], (const uint32_t *)T.slen[f], sh, len[f], (uint64_t *)to[f].off,
                           (uint64_t *)T.rec[f]);
        const unsigned gc = (unsigned)std::min<uint64_t>(((uint64_t)S.nb * cmft::COPY_LANES + FT_T - 1) / FT_T + 1, 1u << 16);
        hipLaunchKernelGGL(k_ft_copy, dim3(gc), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], (const uint32_t *)T.ls[f], (const uint64_t *)to[f].off, sh,
                           (uint8_t *)to[f].seq_base);
    }
    hipLaunchKernelGGL(k_ft_finish, dim3(1), dim3(1), 0, st, sh, (const uint64_t *)to[0].off, (const uint64_t *)to[1].off, (const uint64_t *)T.rec[0],
                       (const uint64_t *)T.rec[1], (unsigned long long *)T.res);
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}
// the refusal a verdict stands for, in the words of next_plain / build_side / check_reads
static int ft_refusal(cm_ctx *ctx, const cmft::Verdict &v) {
    static const char *const bad[] = {"", "the header line is empty or does not start with '@'", "the third line is empty or does not start with '+'",
                                      "the quality line is not as long as the sequence line", "a 23-token header (carried state: take cm_fastq_next)"};
    switch (v.what) {
    case cmft::LINES_LEFT: return fail(ctx, v.code, "FASTQ file %d: %llu lines behind its last whole record", v.file + 1, v.count);
    case cmft::FILE2_SHORT: return fail(ctx, v.code, "FASTQ file 2 ends before file 1");
    case cmft::MALFORMED: return fail(ctx, v.code, "FASTQ file %d, record %llu of the block: %s", v.file + 1, v.record, bad[v.count]);
    case cmft::READ_TOO_LONG: return fail(ctx, v.code, "a read of %llu bases is longer than max_read_len %d", v.count, ctx->P.max_read_len);
    case cmft::TOO_MANY_SEEDS: return check_seeds(ctx, (int)v.count);
    default: return CM_OK;                                  // ACCEPTED
    }
}
// Flag bit 2 (f = 0) / 4 (f = 1): file f's names stay with the staged batch.  Sized by the read-back: no longer than the
// header lines, which are what the consumed text holds besides bases and qualities.  ev.staged moves behind them; nobody waits here.
static int ft_keep_names(cm_ctx *ctx, int f, uint64_t n, uint64_t used, uint64_t bases) {
    TextStage &T = ctx->ft;
    ReadFile &to = ctx->staged.rd.file[f];
    hipStream_t st = ctx->st.C;
    const uint64_t name_max = used - std::min<uint64_t>(used, 2 * bases);
    HIPCHK(ctx, ensure(ctx, to.names, (size_t)name_max + 4));
    HIPCHK(ctx, ensure(ctx, to.name_off, ((size_t)n + 1) * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, T.nstart, ((size_t)n + 1) * sizeof(uint32_t)));
    const unsigned gn = (unsigned)(n / FT_T + 1);            // covers i = 0 .. n
    hipLaunchKernelGGL(k_ft_name_len, dim3(gn), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], (const uint32_t *)T.ls[f], (uint32_t)n, (uint32_t *)T.nstart,
                       (uint32_t *)to.name_off);
    if (int rc = scan32_on(ctx, st, to.name_off, n + 1, to.name_off, T.tmp, 0u, 0)) return rc;
    const unsigned gc = (unsigned)std::min<uint64_t>((n * cmft::COPY_LANES + FT_T - 1) / FT_T, 1u << 16);
    hipLaunchKernelGGL(k_ft_name_copy, dim3(gc), dim3(FT_T), 0, st, (const uint8_t *)T.text[f], (const uint32_t *)T.nstart, (const uint32_t *)to.name_off, (uint32_t)n,
                       (uint8_t *)to.names);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev.staged, st));
    to.has_names = true;
    to.name_bytes_max = name_max;
    return CM_OK;
}
// Flag bit 3: both files' quality lines into arrays that share the offsets with the bases; a word of slack: the formatter reads whole words
static int ft_keep_quals(cm_ctx *ctx, uint64_t n, const uint64_t bases[2]) {
    TextStage &T = ctx->ft;
    ReadBufs &to = ctx->staged.rd;
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, ensure(ctx, to.file[f].qual, (size_t)bases[f] + 8));
    const unsigned gc = (unsigned)std::min<uint64_t>((n * cmft::COPY_LANES + FT_T - 1) / FT_T, 1u << 16);
    for (int f = 0; f < 2; ++f)
        hipLaunchKernelGGL(k_ft_qual_copy, dim3(gc), dim3(FT_T), 0, ctx->st.C, (const uint8_t *)T.text[f], (const uint32_t *)T.ls[f], (const uint64_t *)to.file[f].off,
                           (uint32_t)n, (uint8_t *)to.file[f].qual);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev.staged, ctx->st.C));
    to.has_quals = true;
    to.bases = bases[0] + bases[1];
    return CM_OK;
}

// cm_reads_stage for FASTQ text: the two blocks go over PCIe as they are and the kernels k_ft_* (bodies: cm_fastq_text.h) find the
// lines, check every record and fill the staged read buffers, all on the staging stream.  The batch's shape is known on the device
// only; the host sizes everything from the text lengths (cmft::plan_sizes) and learns the shape and the verdicts from one small
// read-back (cmft::verdict).
int cm_reads_stage_text(cm_ctx *ctx, const uint8_t *text1, uint64_t len1, const uint8_t *text2, uint64_t len2, uint64_t max_pairs, uint32_t flags,
                        uint64_t *rec1, uint64_t *rec2, cm_text_batch *out) {
    if (!ctx || !out) return CM_EINVAL;
    memset(out, 0, sizeof *out);
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    const uint8_t *const text[2] = {text1, text2};
    const uint64_t len[2] = {len1, len2};
    cmft::Sizes S;
    int rc, file = 0;
    if ((rc = cmft::plan_sizes(text, len, max_pairs, flags, &S, &file)))      // refused for its arguments: an earlier staged batch stays
        return rc == CM_EINVAL ? fail(ctx, rc, "cm_reads_stage_text: null text") : fail(ctx, rc, "cm_reads_stage_text: a block of %llu bytes", (unsigned long long)len[file]);
    if ((rc = stage_open(ctx)) || (rc = ft_begin(ctx, S, text, len))) return rc;
    TextStage &T = ctx->ft;
    hipStream_t st = ctx->st.C;
    hipEvent_t t_a = nullptr, t_b = nullptr;                // cm_prof_enable: the kernels' time, copies excluded (cm_text_batch.reserved)
    if (ctx->prof) {
        t_a = take_event(ctx);
        t_b = take_event(ctx);
        if (t_a) HIPCHK(ctx, hipEventRecord(t_a, st));
    }
    const FtShape sh{T.cnt[0] + S.n_chunks[0], T.cnt[1] + S.n_chunks[1], S.trail[0], S.trail[1], S.max_pairs};
    if ((rc = ft_tokenise(ctx, S, sh, len))) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev.staged, st));       // behind the last tokeniser kernel: the cross-batch prefetch reads the buffers behind it
    if (t_a && t_b) HIPCHK(ctx, hipEventRecord(t_b, st));
    unsigned long long *R = ctx->h_pin + PIN_TEXT;          // the read-back
    HIPCHK(ctx, hipMemcpyAsync(R, T.res, cmft::RES_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (t_a && t_b) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t_a, t_b) == hipSuccess) out->reserved = (int32_t)std::min(ms * 1000.f, 2.0e9f);
    }
    for (hipEvent_t e : {t_a, t_b})
        if (e) ctx->ev_free.push_back(e);
    if ((rc = ft_refusal(ctx, cmft::verdict(R, flags, max_pairs, ctx->P.max_read_len, ctx->P.kmer, cmc::MAX_SEEDS)))) return rc;
    *out = cm_text_batch{R[cmft::RES_PAIRS], R[cmft::RES_USED1], R[cmft::RES_USED2], (int32_t)R[cmft::RES_MAX_LEN], out->reserved};
    const uint64_t n = out->n_pairs, used[2] = {R[cmft::RES_USED1], R[cmft::RES_USED2]}, bases[2] = {R[cmft::RES_BASES1], R[cmft::RES_BASES2]};
    if (n == 0) return CM_OK;                               // nothing staged: the caller supplies more bytes
    if (rec1) HIPCHK(ctx, hipMemcpyAsync(rec1, T.rec[0], (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (rec2) HIPCHK(ctx, hipMemcpyAsync(rec2, T.rec[1], (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (rec1 || rec2) HIPCHK(ctx, hipStreamSynchronize(st));
    // kept data, on the staging stream in this order: R1 names, qualities, R2 names
    if ((flags & 4u) && (rc = ft_keep_names(ctx, 0, n, used[0], bases[0]))) return rc;
    if ((flags & 8u) && (rc = ft_keep_quals(ctx, n, bases))) return rc;
    if ((flags & 16u) && (rc = ft_keep_names(ctx, 1, n, used[1], bases[1]))) return rc;
    ctx->staged.commit(n, out->max_len, false);
    return CM_OK;
}

// The peeks: per file of the resident batch src[0 .. off[n]) into dst (nullable; cap bytes of room) and, where asked for, the n + 1 offsets
struct Peek { uint8_t *dst; uint64_t cap; const uint8_t *src; uint64_t *off_out; };
static int peek_files(cm_ctx *ctx, const char *fn, const char *noun, const Peek (&p)[2]) {
    const uint64_t n = ctx->n_pairs;
    hipStream_t st = ctx->st.B;
    uint64_t total[2] = {0, 0};
    for (int f = 0; f < 2; ++f) HIPCHK(ctx, hipMemcpyAsync(&total[f], ctx->rd.file[f].off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    for (int f = 0; f < 2; ++f)
        if (p[f].off_out) HIPCHK(ctx, hipMemcpyAsync(p[f].off_out, ctx->rd.file[f].off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if ((p[0].dst && p[0].cap < total[0]) || (p[1].dst && p[1].cap < total[1])) return fail(ctx, CM_ELIMIT, "%s: %llu / %llu %s bytes", fn, (unsigned long long)total[0], (unsigned long long)total[1], noun);
    for (int f = 0; f < 2; ++f)
        if (p[f].dst && total[f]) HIPCHK(ctx, hipMemcpyAsync(p[f].dst, p[f].src, total[f], hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return CM_OK;
}

// test hook: the resident batch's read bytes and offsets copied back
int cm_reads_peek(cm_ctx *ctx, uint8_t *seq1, uint64_t cap1, uint64_t *off1, uint8_t *seq2, uint64_t cap2, uint64_t *off2, uint64_t *n_pairs) {
    if (!ctx || !n_pairs) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    *n_pairs = ctx->n_pairs;
    if (ctx->n_pairs == 0 || (!seq1 && !seq2 && !off1 && !off2)) return CM_OK;
    const ReadFile *F = ctx->rd.file;
    return peek_files(ctx, "cm_reads_peek", "read", {{seq1, cap1, F[0].seq(), off1}, {seq2, cap2, F[1].seq(), off2}});
}

int cm_reads_swap(cm_ctx *ctx) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    cm_ctx::Staged &sb = ctx->staged;
    if (!sb.ready) return fail(ctx, CM_ESTATE, "cm_reads_swap: no staged batch");
    // work already queued on the mapping stream still reads the old buffers: order the swap behind it on the device
    // (no host wait), and the new batch's first kernel behind the staged copies
    swap(ctx->rd, sb.rd);
    sb.ready = false;
    ctx->pre_ready = ctx->pre_launched;                            // cm_map_rounds prepared this batch's first round already
    ctx->pre_launched = false;
    ctx->pre_n = sb.n_pairs;
    ctx->n_pairs = 0;
    if (int rc = make_resident(ctx, sb.n_pairs, sb.max_len, ctx->ev.staged, sb.has_prior ? (const cm_mapped_read *)sb.prior : nullptr, hipMemcpyDeviceToDevice)) return rc;
    // the next cm_reads_stage overwrites the buffers this swap retired: it must wait for the mapping stream's work on them
    HIPCHK(ctx, hipEventRecord(ctx->ev.retired, ctx->st.B));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.C, ctx->ev.retired, 0));
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}

// The re-run launch of a pair stage and ev.pair[b] behind it.  Eight blocks that each ask for 47 - 64 KB of LDS behind kernels that
// fill the chip wait milliseconds for their turn -- on the hg38-like bench until the heavy chaining kernel of the NEXT item had
// drained, and the item after that (its seeding reads the flags, its chaining rewrites the chain records) behind them -- to find,
// nearly always, an empty list.  So with several tiles the decision is made late (`defer`): the pair stage copies the length of
// its re-run list to the host, and whoever first needs the stage to be complete calls settle_pair, which waits for the two pair
// kernels (ev.first[b]), launches the re-run only if something is queued, and records ev.pair[b].
static int launch_rerun(cm_ctx *ctx, int b) {
    const cm_ctx::Rerun &q = ctx->rerun[b];
    const PairSet &ps = ctx->pset[b];
    const RetryArgs ra2{ps.pair_err, ps.retry_list, ps.retry_ctr, ctx->d_spill, RETRY_SPILL, 0};
    hipLaunchKernelGGL(k_pair_rerun, dim3(RETRY_GRID), dim3(BLK_PAIR), q.lds2, ctx->st.R, q.core, q.rd, q.p0, q.nt, q.chains, q.nchain, q.high,
                       ctx->d_state, q.act_out, ctx->d_cat, q.is_last, ctx->d_err, ctx->d_counters, q.cap2, (unsigned long long *)nullptr,
                       (const uint32_t *)ps.retry_list, (const unsigned int *)ps.retry_ctr, ps.retry_ctr + 1, ra2);
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}
// The pipeline's fall-back launch: k_pair_heavy over the pairs whose tasks or unpaired chains did not fit the pipeline's arrays (none on
// the bench workloads).  A launch that asks for 14 KB of LDS per wave to find an empty list waited 0.03 - 2.3 ms behind the chain kernels
// of the next item at the end of every pair stage: decided late like the re-run, from the list length the stage copied to the host.
static int launch_fall_back(cm_ctx *ctx, int b, hipStream_t st) {
    const cm_ctx::Rerun &q = ctx->rerun[b];
    const PairSet &ps = ctx->pset[b];
    const RetryArgs ra1{ps.pair_err, ps.retry_list, ps.retry_ctr, nullptr, 0, 1};
    launch(ctx, PC_HEAVY, k_pair_heavy, dim3(q.fall_grid), dim3(BLK_PAIR), q.lds_heavy, st, q.core, q.rd, q.p0, ps.hp_fall, ps.hp_fallctr, q.chains, q.nchain, q.high,
           ctx->d_state, q.act_out, ctx->d_cat, q.is_last, ctx->d_err, ctx->d_counters, q.str_cap, nullptr, ctx->d_hres, ps.cls_ctr + CTR_NEXT + 1, ra1);
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}
// wait = false: without blocking the host (the end of cm_map_rounds, which stays asynchronous): the re-run is launched whatever the count
static int settle_pair(cm_ctx *ctx, int b, bool wait = true) {
    if (!ctx->rerun[b].deferred) return CM_OK;
    ctx->rerun[b].deferred = false;
    if (wait) HIPCHK(ctx, hipEventSynchronize(ctx->ev.first[b]));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.R, ctx->ev.first[b], 0));
    bool fell = false;
    if (ctx->rerun[b].fall && (!wait || *(const volatile unsigned int *)(ctx->h_pin + PIN_FALL_N + b) != 0u)) {
        const int rc = launch_fall_back(ctx, b, ctx->st.R);        // (may queue pairs for the re-run: that one unconditionally then)
        if (rc) return rc;
        fell = true;
    }
    if (!wait || fell || *(const volatile unsigned int *)(ctx->h_pin + PIN_RERUN_N + b) != 0u) {
        const int rc = launch_rerun(ctx, b);
        if (rc) return rc;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev.pair[b], ctx->st.R));
    return CM_OK;
}

// The pair stage of one tile and round on the pair streams: waits for that item's chains (ev.prep[b]), reads the flags
// act_in, writes act_out for every pair of the tile, signals ev.pair[b] when the chain buffers of set b are free again.
// same_tile_as_prev: the previous item was this tile's previous round -- its re-run launch (stream R) wrote states and flags this
// item's pair kernels read; every other consumer is ordered behind the re-run through ev.pair[].
static int run_pair_tile(cm_ctx *ctx, const KCore &core, uint64_t p0, uint32_t nt, int is_last_round, const uint8_t *act_in, uint8_t *act_out,
                         const ChainRecs &rb, int b, bool same_tile_as_prev, bool defer) {
    const ReadsDev rd = current_reads(ctx);
    hipStream_t sp = ctx->st.P, sp2 = ctx->st.P2, sp3 = ctx->st.R;
    {
        int rc;
        if ((rc = settle_pair(ctx, b))) return rc;                       // this set's previous stage (its re-run list is about to be reused)
        if (same_tile_as_prev && (rc = settle_pair(ctx, b ^ 1))) return rc;
    }
    // The work classes and ordered lists of this stage (ten small launches) go to a stream of their own, so -- every array the pair
    // kernels read from them existing once per set of chain records -- they are computed while the pair stage of the item before
    // still runs, as soon as this item's chains are complete; behind that stage on the pair stream they were 1.7 ms per item with
    // nothing else on the chip but the next item's seeding (12 % of the hg38-like step).
    hipStream_t so = ctx->st.O;
    HIPCHK(ctx, hipStreamWaitEvent(so, ctx->ev.prep[b], 0));
    if (same_tile_as_prev && ctx->pair_pending[b ^ 1]) HIPCHK(ctx, hipStreamWaitEvent(so, ctx->ev.pair[b ^ 1], 0));
    const PairSet &ps = ctx->pset[b];
    uint32_t *const perm = ps.perm, *const hlist = ps.hlist, *const pair_err = ps.pair_err;
    unsigned int *const cls_ctr = ps.cls_ctr, *const retry_ctr = ps.retry_ctr;
    // str_cap: chars per staged string (multiple of 8); LDS = 2 strings x lbuf_bytes(str_cap) x 64 lanes
    // a DP string is at most a read minus one seed, plus the band (extend_side: len + band; dp_fits() reports anything longer)
    // (+ 4 characters of slack: 144 characters = 76-byte rows for 2 x 150 bp at k = 20.  No slack gives 72-byte rows and takes
    // k_pair_heavy's LDS per wave from 12 to 11 allocation steps of 1 280 bytes: its kernel time -4 %, the step +1 %: NOTES 44)
    constexpr int str_slack = 4;
    const int str_cap = ((ctx->max_len - ctx->P.kmer + ctx->P.band + str_slack + 7) / 8) * 8;
    // The pair kernels' time hardly depends on their occupancy (16.0 / 16.2 / 16.4 ms per step at 4 / 3 / 2 waves per SIMD on the
    // hg38-like bench; 22 ms at 1).  Padding their LDS request to hold them at 1..3 waves per SIMD would leave registers and wave
    // slots to the seeding / chaining of the next round; measured best overall: no padding (4 waves per SIMD).
    constexpr unsigned slots_per_simd = 4;
    const size_t lds_bytes = (size_t)2 * lbuf_bytes(str_cap) * BLK_PAIR;
    const size_t lds_heavy = lds_bytes + HG * sizeof(HSlot);
    // the re-run launch of k_pair (RetryArgs): staging buffers for strings of any length a read of this batch can produce
    const int cap2 = std::min(((2 * ctx->max_len + 64 + 7) / 8) * 8, 1016);      // 1016: 64 KB of LDS per wave
    const size_t lds2 = (size_t)2 * lbuf_bytes(cap2) * BLK_PAIR;
    {   // dynamic-LDS limits of the three kernels: process-wide properties, only ever raised (see run_chain_tile)
        static std::atomic<size_t> lim[3] = {{48u * 1024u}, {48u * 1024u}, {48u * 1024u}};
        const void *fn[3] = {(const void *)k_pair, (const void *)k_pair_rerun, (const void *)k_pair_heavy};
        const size_t want[3] = {lds_bytes, lds2, lds_heavy};
        for (int k = 0; k < 3; ++k)
            if (want[k] > lim[k].load()) {
                HIPCHK(ctx, hipFuncSetAttribute(fn[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)want[k]));
                lim[k].store(want[k]);
            }
    }
    {
        Timer t(ctx, PC_ORDER, so);
        const uint32_t nbk = (nt + CLS_T - 1) / CLS_T;
        static const bool fixed_cost = getenv("CM_HEAVY_COST") != nullptr;             // tuning knob: no adaptive threshold
        static const int heavy_cost = fixed_cost ? atoi(getenv("CM_HEAVY_COST")) : HEAVY_COST;
        unsigned long long *load = nullptr;
        if (!fixed_cost) {
            load = ctx->d_heavy_load;
            HIPCHK(ctx, hipMemsetAsync(load, 0, sizeof(unsigned long long), so));
            // (PC_NONE: the class has counted ten launches per stage, k_pair_cls + the sort, since before this kernel came)
            launch(ctx, PC_NONE, k_pair_cost, dim3((nt + BLK - 1) / BLK), dim3(BLK), 0, so, rb.nchain, act_in, p0, nt, HEAVY_COST, load);
            // the host learns the load of a tile one or two items late (no wait): good enough to size the next heavy grid
            HIPCHK(ctx, hipMemcpyAsync((void *)(ctx->h_pin + PIN_HEAVY_LOAD), load, sizeof(unsigned long long), hipMemcpyDeviceToHost, so));
            ctx->h_pin_nt = nt;
        }
        launch(ctx, PC_ORDER, k_pair_cls, dim3((nt + BLK - 1) / BLK), dim3(BLK), 0, so, core, rb.chains, rb.resid, rb.nchain, act_in, p0, nt, ctx->sort.cls, ctx->d_cat,
               heavy_cost, ctx->sort.sub, ctx->sort.sub2, act_out, load);
        // three-pass LSD radix sort, 16 x 16 x 16 classes: by the longest residual, by the set of extensions a pair needs, then (stable) by its class
        const PairSort &w = ctx->sort;
        counting_sort(ctx, PC_ORDER, {so, w.sub2, nt, w.blk_cnt, nbk, w.ctr3, w.perm0});
        counting_sort(ctx, PC_ORDER, {so, w.sub, nt, w.blk_cnt, nbk, w.ctr2, w.perm1, N_CLS, nullptr, -1, w.perm0, w.ctr3 + CTR_SUM});
        counting_sort(ctx, PC_ORDER, {so, w.cls, nt, w.blk_cnt, nbk, cls_ctr, perm, N_CLS, hlist, 1 << HEAVY_CLS, w.perm1, w.ctr2 + CTR_SUM});
    }
    HIPCHK(ctx, hipMemsetAsync(cls_ctr + CTR_NEXT, 0, 2 * sizeof(unsigned int), so));     // both work cursors
    HIPCHK(ctx, hipMemsetAsync(retry_ctr, 0, 2 * sizeof(unsigned int), so));                     // re-run count + cursor of this set
    HIPCHK(ctx, hipEventRecord(ctx->ev.order[b], so));
    HIPCHK(ctx, hipStreamWaitEvent(sp, ctx->ev.prep[b], 0));
    HIPCHK(ctx, hipStreamWaitEvent(sp, ctx->ev.order[b], 0));
    const RetryArgs ra1{pair_err, ps.retry_list, retry_ctr, nullptr, 0, 1};
    {   // what the late launches of this stage need (settle_pair: the re-run, the pipeline's fall-back)
        cm_ctx::Rerun &q = ctx->rerun[b];
        q.core = core; q.rd = rd; q.p0 = p0; q.nt = nt;
        q.chains = rb.chains; q.nchain = rb.nchain; q.high = rb.high;
        q.act_out = act_out; q.is_last = is_last_round; q.cap2 = cap2; q.lds2 = lds2;
        q.fall = false;
    }
    // The heavy pairs go to a second stream: their kernels fit into the slots the light kernel leaves instead of queueing behind it.
    // That stream waits for this item's chains and lists itself, not for the light stream (which sits at the lowest priority, behind the
    // light kernel of the item before): what the heavy kernels share with the previous stage's light kernel exists once per set (re-run
    // list, cursors) or per tile (states, flags: another tile's, or ordered behind ev.pair through the ordering stream).
    HIPCHK(ctx, hipStreamWaitEvent(sp2, ctx->ev.prep[b], 0));
    HIPCHK(ctx, hipStreamWaitEvent(sp2, ctx->ev.order[b], 0));
    {
        Timer t(ctx, PC_HEAVY, sp2);
        // both pair kernels are persistent: together they fill the wave slots of every SIMD (256 CUs x 4 SIMDs), half each
        const unsigned cap = 256u * 4u * slots_per_simd;
        // Heavy grid: half the wave capacity, or all of it when the tiles of this run carry a large heavy load (the value
        // k_pair_cost left for an earlier item, read without waiting): on the dense genome the heavy kernel has work for every
        // slot (19.9 vs 18.9 M pairs/s); with little heavy work the extra waves only sit on registers the next item's chain
        // stage is waiting for (round-2 genome: 43.3 vs 44.4 M pairs/s).
        const volatile unsigned long long *seen = (const volatile unsigned long long *)(ctx->h_pin + PIN_HEAVY_LOAD);
        const bool loaded_run = ctx->h_pin_nt && *seen > HEAVY_LOAD * (unsigned long long)ctx->h_pin_nt;
        const unsigned heavy_cap = cap / (loaded_run ? 1u : 2u);
        const unsigned heavy_lim = std::min(heavy_cap, HEAVY_GRID_MAX);     // d_hres is sized for HEAVY_GRID_MAX blocks
        const unsigned heavy_grid = nt < heavy_lim ? (nt ? nt : 1u) : heavy_lim;
        if (heavy_pipeline() && ctx->P.band == 3) {
            // the heavy pairs as a pipeline of full-width kernels (cm_heavy_pipe.h); what does not fit its arrays comes back in a
            // fall-back list and goes through k_pair_heavy behind it
            const HPipe hp{ctx->hp.pairs, ctx->hp.list2, ps.hp_fall, ctx->hp.T, ctx->hp.pre, ctx->hp.q, ctx->hp.res, ctx->hp.U, ctx->hp.pre2,
                           ctx->hp.q2, ctx->hp.ctr, ctx->hp.tasks_cap, ctx->hp.unp_cap, ps.hp_fallctr, ctx->hp.tcls};
            const unsigned int *n_heavy = cls_ctr + HEAVY_CLS, *n_list2 = ctx->hp.ctr + HC_LIST2;
            constexpr unsigned pipe_grid = 2048u;        // workgroups of the item kernels
            const size_t lds_slots = HG * sizeof(HSlot);
            HIPCHK(ctx, hipMemsetAsync(ctx->hp.ctr, 0, HC_WORDS * sizeof(unsigned int), sp2));
            HIPCHK(ctx, hipMemsetAsync(ps.hp_fallctr, 0, sizeof(unsigned int), sp2));
            const dim3 g(pipe_grid), wg(BLK_PAIR);
            // Two passes (process_read's two attempts), the second over the few pairs whose other orientation has chains at all (k_hp_finish
            // settles the others in place).  CM_HP_ATTEMPTS=1 (diagnostic) sends those pairs whole to the fall-back kernel instead: its
            // long tail over a few hundred heavy pairs costs more than nine short launches (77.9 vs 75.9 ms per step).
            static const bool task_order = !(getenv("CM_HP_TASK_ORDER") && getenv("CM_HP_TASK_ORDER")[0] == '0');      // diagnostic: tasks in array order
            static const int n_attempts = (getenv("CM_HP_ATTEMPTS") && atoi(getenv("CM_HP_ATTEMPTS")) == 1) ? 1 : 2;
            for (int attempt = 0; attempt < n_attempts; ++attempt) {
                // An attempt starts from zeroed counters: the memset above, k_hp_reset between the two.  The class counts that step in both
                // (nine steps per attempt since the pipeline came: the reset and the eight item kernels; the task sort is not among them).
                if (attempt) launch(ctx, PC_HEAVY, k_hp_reset, dim3(1), dim3(64), 0, sp2, ctx->hp.ctr);
                else ++ctx->launches[PC_HEAVY];
                launch(ctx, PC_HEAVY, k_hp_plan, dim3(HP_PLAN_GRID), wg, lds_slots, sp2, core, rd, p0, hlist, n_heavy, ctx->hp.list2, n_list2, attempt,
                       rb.chains, rb.nchain, rb.high, ctx->d_state, hp, ctx->hp.lists, str_cap, ctx->d_counters);
                launch(ctx, PC_HEAVY, k_hp_dp, g, wg, lds_bytes, sp2, core, rd, p0, attempt, hp, 0, str_cap);
                const bool ordered = task_order && attempt == 0;       // (the second attempt's handful: array order)
                if (ordered) {       // the tasks by work class, heaviest first: 16 classes over the tile's task array, whose length is on the device
                    const unsigned int *n_t = ctx->hp.ctr + HC_TASKS;
                    CountingSort ts{sp2, ctx->hp.tcls, ctx->hp.tasks_cap, ctx->hp.tblk, (ctx->hp.tasks_cap + CLS_T - 1) / CLS_T, ctx->hp.tctr, ctx->hp.tperm};
                    ts.n_dev = n_t, ts.grid_cap = 2048u;               // a grid that walks the stretches in use
                    counting_sort(ctx, PC_NONE, ts);
                }
                launch(ctx, PC_HEAVY, k_hp_tasks, g, wg, lds_bytes, sp2, core, rd, p0, attempt, rb.chains, rb.nchain, hp, pair_err, str_cap, ordered ? (uint32_t *)ctx->hp.tperm : nullptr,
                     ctx->hp.tctr + CTR_SUM);
                launch(ctx, PC_HEAVY, k_hp_fold, g, wg, 0, sp2, core, p0, ctx->hp.list2, n_list2, n_heavy, attempt, hp, ctx->d_counters);
                launch(ctx, PC_HEAVY, k_hp_unp_req, g, wg, 0, sp2, core, rd, p0, attempt, rb.chains, hp, str_cap);
                launch(ctx, PC_HEAVY, k_hp_dp, g, wg, lds_bytes, sp2, core, rd, p0, attempt, hp, 1, str_cap);
                launch(ctx, PC_HEAVY, k_hp_unp, g, wg, lds_bytes, sp2, core, rd, p0, attempt, rb.chains, hp, pair_err, str_cap);
                launch(ctx, PC_HEAVY, k_hp_finish, g, wg, 0, sp2, core, p0, ctx->hp.list2, n_list2, n_heavy, attempt, hp, ctx->d_state, act_out, ctx->d_cat, is_last_round, ctx->d_counters, ra1,
                     rb.nchain, n_attempts == 1 ? 1 : 0);
            }
            // what did not fit goes through k_pair_heavy: now (one tile), or when the stage is settled and the list is known to hold something
            // (its own work cursor, cls_ctr + CTR_NEXT + 1, was zeroed with the light kernel's)
            HIPCHK(ctx, hipMemcpyAsync((void *)(ctx->h_pin + PIN_FALL_N + b), ps.hp_fallctr, sizeof(unsigned int), hipMemcpyDeviceToHost, sp2));
            {
                cm_ctx::Rerun &q = ctx->rerun[b];
                q.fall = true;
                q.lds_heavy = lds_heavy;
                q.str_cap = str_cap;
                q.fall_grid = std::min(heavy_grid, 256u);
            }
            if (!defer) {
                int rc;
                if ((rc = launch_fall_back(ctx, b, sp2))) return rc;
                ctx->rerun[b].fall = false;
            }
        } else {
            launch(ctx, PC_HEAVY, k_pair_heavy, dim3(heavy_grid), dim3(BLK_PAIR), lds_heavy, sp2, core, rd, p0, hlist, cls_ctr + HEAVY_CLS, rb.chains, rb.nchain, rb.high,
                   ctx->d_state, act_out, ctx->d_cat, is_last_round, ctx->d_err, ctx->d_counters, str_cap,
                   ctx->d_lane_clk ? ctx->d_lane_clk + (size_t)nt * 16 + (size_t)(nt / 64 + 1) * 64 : nullptr, ctx->d_hres, cls_ctr + CTR_NEXT + 1, ra1);
        }
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev.join_p, sp2));
    {
        Timer t(ctx, PC_PAIR, sp);      // = the pair stage: the light kernel and the wait for the second stream
        const unsigned want = (nt + BLK_PAIR - 1) / BLK_PAIR, cap = (heavy_pipeline() && ctx->P.band == 3) ? 2048u      // the pipeline's kernels come and go: half the slots (78.7 -> 76.3 ms per step)
                                                                                                           : 256u * 4u * slots_per_simd;   // light takes the slots heavy leaves: full cap
        launch(ctx, PC_PAIR, k_pair, dim3(want < cap ? want : cap), dim3(BLK_PAIR), lds_bytes, sp, core, rd, p0, nt, rb.chains, rb.nchain, rb.high, ctx->d_state,
               act_out, ctx->d_cat, is_last_round, ctx->d_err, ctx->d_counters, str_cap, ctx->d_lane_clk, perm, cls_ctr + CTR_SUM, cls_ctr + CTR_NEXT, ra1);
        HIPCHK(ctx, hipStreamWaitEvent(sp, ctx->ev.join_p, 0));
    }
    // The re-run of whatever the two kernels queued (usually nothing: the launch reads the count on the device and ends): the same
    // code over the re-run list, one pair per lane, memo spill area, staging buffers for strings of any length a read of this
    // batch can produce.  On a stream of its own: a launch of 8 blocks behind kernels that fill the chip can wait milliseconds
    // for its turn (2.5 ms on average on the hg38-like bench), and only the consumers of this item's results have to wait for
    // it -- ev.pair[b] (chain records of set b free, flags and states of the tile final) is recorded behind it.
    HIPCHK(ctx, hipMemcpyAsync((void *)(ctx->h_pin + PIN_RERUN_N + b), retry_ctr, sizeof(unsigned int), hipMemcpyDeviceToHost, sp));
    HIPCHK(ctx, hipEventRecord(ctx->ev.first[b], sp));
    ctx->rerun[b].deferred = defer;
    if (!defer) {
        HIPCHK(ctx, hipStreamWaitEvent(sp3, ctx->ev.first[b], 0));
        int rc;
        if ((rc = launch_rerun(ctx, b))) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev.pair[b], sp3));
    }
    ctx->pair_pending[b] = true;
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}

// The rounds of cm_map_rounds; any failure (a HIP call, a stage) returns from here and is cleaned up by the caller below.
// *rounds_done counts the rounds whose pair stage was issued for every tile (the flags arrays have swapped roles that often).
static int map_rounds_issue(cm_ctx *ctx, const int *slots, int n_rounds, int last_is_final, int *items_done, int *rounds_done) {
    int rc;
    // Cross-batch prefetch (see the end of this function): possible when this call ends the batch and the next one is staged and fits
    // the workspace as it is sized now (nothing may be reallocated under the kernels in flight).
    const bool prefetch = last_is_final && ctx->staged.ready && ctx->staged.n_pairs <= ctx->n_pairs && ctx->staged.max_len <= ctx->max_len;
    if (prefetch && ctx->ones_cap < ctx->staged.n_pairs) {          // flags of a fresh batch: every pair active
        HIPCHK(ctx, ensure(ctx, ctx->d_ones, ctx->n_pairs));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_ones, 1, ctx->n_pairs, ctx->st.B));
        ctx->ones_cap = ctx->n_pairs;
    }
    // everything queued on the main stream so far (uploads, resets, collects of the previous batch) comes first
    HIPCHK(ctx, hipEventRecord(ctx->ev.tail, ctx->st.B));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.P, ctx->ev.tail, 0));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.S, ctx->ev.tail, 0));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.O, ctx->ev.tail, 0));
    HIPCHK(ctx, hipEventRecord(ctx->ev.flags, ctx->st.B));
    uint8_t *A[2] = {ctx->d_active, ctx->d_active_b};      // A[0] = flags before the first of these rounds
    // The work items: (tile, round).  One tile per batch: its rounds in order.  Several tiles: ROUND-major -- every tile through
    // round r, then every tile through round r + 1 -- so that between the pair stage of (tile, r) and the seeding of (tile, r + 1)
    // lies the work of the other tiles: the flags that pair stage wrote are final when the seeding starts, and seeds / chains are
    // computed for exactly the pairs still active (with one tile the seeding of round r + 1 runs UNDER the pair stage of round r
    // and has to take the flags from before it, a superset: 20 % more seeding and chaining on the hg38-like bench).
    struct Item { uint64_t p0; uint32_t nt; int r; };
    std::vector<Item> items;
    const uint64_t n_tiles = (ctx->n_pairs + ctx->tile - 1) / ctx->tile;
    const bool round_major = n_tiles >= 2;
    auto tile_nt = [&](uint64_t t) { return (uint32_t)((ctx->n_pairs - t * ctx->tile < ctx->tile) ? ctx->n_pairs - t * ctx->tile : ctx->tile); };
    if (round_major) {
        for (int r = 0; r < n_rounds; ++r)
            for (uint64_t t = 0; t < n_tiles; ++t) items.push_back(Item{t * ctx->tile, tile_nt(t), r});
    } else {
        for (uint64_t t = 0; t < n_tiles; ++t)
            for (int r = 0; r < n_rounds; ++r) items.push_back(Item{t * ctx->tile, tile_nt(t), r});
    }
    const int n_items = (int)items.size();
    std::vector<int> tiles_of_round((size_t)n_rounds, 0);
    // Was this batch's first item prepared while the previous batch was in its last pair stage (see the end of this function)?
    const bool use_pre = ctx->pre_ready && slots[0] == ctx->pre_slot && ctx->slots[slots[0]].gen == ctx->pre_gen && ctx->n_pairs == ctx->pre_n &&
                         items[0].nt == ctx->pre_nt && (ctx->item_base & 1) == ctx->pre_b;
    ctx->pre_ready = ctx->pre_launched = false;            // the items below reuse both sets of chain records
    if (use_pre) ++ctx->launches[PC_PREFETCH];       // (no launch: a take-over)
    const ReadsDev rd_cur = current_reads(ctx);
    // Seeds and chains of round r depend on the reads and the contig only; the flags merely skip pairs that are retired.
    // Round-major: A[r & 1], what the pair stage of (tile, r - 1) wrote -- item i - n_tiles, complete before item i - 2, for
    // which this item waits anyway (it reuses its chain records).  One tile: the pair stage of round r - 1 is still writing
    // A[r & 1], so the flags from before it (pairs it retires get chains nobody looks at).
    auto prep_flags = [&](int i) -> const uint8_t * {
        const int r = items[i].r;
        return round_major ? A[r & 1] : ((r == 0) ? A[0] : A[(r - 1) & 1]);
    };
    // Seeding runs one item ahead of chaining.  The chain stage of an item ends with a long tail of a few heavy problems, one
    // wave each, and the host waits for it (the pair stage must not start on truncated improvement logs); seeding of the next
    // item used to start after that wait, with the chip nearly idle through the tail and the next chain stage waiting for the
    // seeds.  Now seeding of item i + 1 is issued (stream S, seed set (i + 1) & 1) as soon as the chain kernels of item i are
    // launched: it needs the flags of the pair stage of item i - 1 (two tiles; earlier with more), which ends during that chain
    // stage, so the seeds are computed under the tail and the next chain stage starts right behind this one.
    std::vector<char> seeded((size_t)n_items, 0);
    bool pre_seeded = false;
    // With three or more tiles the flags item i + 1 reads were written by the pair stage of item i - 2 or earlier, complete before the
    // chain stage of item i starts: the seeds (not their classes, which go into chain records item i - 1's pair stage still reads) are
    // then computed under that chain stage instead of behind the pair stage of item i - 1.  Two tiles: seeding + chaining (8 + 14 ms at
    // 2^21 pairs) sat between the end of one pair stage and the start of the next but one, longer than the pair stage between them.
    // Two tiles: the flags are the ones the pair kernels of item i - 1 write, and the host cannot issue anything when those end -- it
    // sits in the wait for the chain stage of item i, which ends later: the seeding of item i + 1 started when THAT was over, and the
    // chip idled for 5 - 6 ms of every 22-ms item with nothing but the tail of k_chain_heavy on it.  The seeds are queued on the device
    // behind ev.first of that pair stage instead (its kernels and the heavy pairs' pipeline; a pair left to a late launch -- re-run,
    // fall-back -- counts as active until that launch writes its flag, a superset, and the classes below use the final flags).
    const bool early_ok = round_major;
    auto issue_seed_early = [&](int i) -> int {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->st.S, ctx->ev.flags, 0));
        if (n_tiles == 2 && i >= 2) HIPCHK(ctx, hipStreamWaitEvent(ctx->st.S, ctx->ev.first[(ctx->item_base + i) & 1], 0));
        // the whole seed stage: the classes too, into scratch of the seed set (the chain records they belong in are still being read;
        // run_chain_tile carries them over).  Under superset flags a pair the late launches retire gets chains nobody looks at.
        const ChainRecs &rbe = ctx->rec[(ctx->item_base + i) & 1];
        const int e = run_seed_tile(ctx, make_core(ctx, ctx->slots[slots[items[i].r]]), rd_cur, items[i].p0, items[i].nt, prep_flags(i), i & 1, ctx->st.S, &rbe, skip_dead_chains(ctx), true);
        seeded[(size_t)i] = 1;
        return e;
    };
    auto issue_seed = [&](int i, hipStream_t st) -> int {
        const int b = (ctx->item_base + i) & 1;
        // flags (and, for the chain stage behind it, the chain records of set b) are final once that pair stage is done; the main
        // stream queues the same wait before the chain stage and clears the mark
        int e;
        if ((e = settle_pair(ctx, b))) return e;
        if (ctx->pair_pending[b]) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev.pair[b], 0));
        const ChainRecs &rbi = ctx->rec[b];
        e = run_seed_tile(ctx, make_core(ctx, ctx->slots[slots[items[i].r]]), rd_cur, items[i].p0, items[i].nt, prep_flags(i), i & 1, st, &rbi, skip_dead_chains(ctx));
        seeded[(size_t)i] = 1;
        return e;
    };
    for (int i = 0; i < n_items; ++i) {
        const uint64_t p0 = items[i].p0;
        const uint32_t nt = items[i].nt;
        const int r = items[i].r, b = (ctx->item_base + i) & 1;
        const Slot &sl = ctx->slots[slots[r]];
        const KCore core = make_core(ctx, sl);
        const ChainRecs &rb = ctx->rec[b];
        const uint8_t *act_prep = prep_flags(i);
        // ... if the pair stage whose flags it reads (item i - 1 with two tiles) is over by then.  Otherwise the host would sit in
        // settle_pair until it is, and this item's pair stage -- whose work classes and lists can be computed under that same stage
        // (stream O) -- would be issued late: then the seeding is issued behind this item's pair stage instead (`late`).
        auto ahead = [&]() -> int {
            if (i + 1 >= n_items || seeded[(size_t)i + 1]) return CM_OK;
            if (early_ok) return issue_seed_early(i + 1);      // queued on the device behind what it depends on: nothing left for later
            const int bn = (ctx->item_base + i + 1) & 1;
            if (ctx->rerun[bn].deferred && hipEventQuery(ctx->ev.first[bn]) != hipSuccess) {
                (void)hipGetLastError();                                  // not ready
                return CM_OK;
            }
            return issue_seed(i + 1, ctx->st.S);
        };
        auto late = [&]() -> int { return (i + 1 < n_items && !seeded[(size_t)i + 1]) ? issue_seed(i + 1, ctx->st.S) : CM_OK; };
        // The last item has nothing of this batch to seed ahead: the seeds of the NEXT batch's first item instead (the prefetch below
        // then starts with its chain stage; without this the prefetched chains ended 3.7 ms after the batch's last pair stage and
        // held up the hand-over).  Seeds only: the chain records they will be chained into are still being read.
        if (i == n_items - 1 && prefetch && !pre_seeded) {
            const Slot &sl0 = ctx->slots[slots[0]];
            const uint32_t nt0 = tile_for(ctx->staged.n_pairs);                     // = that batch's first tile (<= this batch's: it has no more pairs)
            const ReadsDev rd_next = reads_dev(ctx->staged.rd);
            HIPCHK(ctx, hipStreamWaitEvent(ctx->st.S, ctx->ev.staged, 0));
            if ((rc = run_seed_tile(ctx, make_core(ctx, sl0), rd_next, 0, nt0, ctx->d_ones, n_items & 1, ctx->st.S, nullptr, skip_dead_chains(ctx)))) return rc;
            pre_seeded = true;
        }
        if (use_pre && i == 0) {                                          // set b holds this item's chains, ev.prep[b] is recorded
            if ((rc = ahead())) return rc;
        } else {
            if (!seeded[(size_t)i] && (rc = issue_seed(i, ctx->st.B))) return rc;
            if ((rc = settle_pair(ctx, b))) return rc;
            if (ctx->pair_pending[b]) {                                   // chain buffers of set b: free once their pair stage is done
                HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.pair[b], 0));
                ctx->pair_pending[b] = false;
            }
            HIPCHK(ctx, hipEventRecord(ctx->ev.flags, ctx->st.B));      // (pair stage of item i - 2 and everything before it)
            // (one tile: the chain kernels do not wait for the pair stage of round r - 1 to use its output flags -- chain kernels
            // 8.4 -> 6.7 ms per step, step 24.0 -> 25.1 ms: the wait costs more than the work it saves)
            if ((rc = run_chain_tile(ctx, core, rd_cur, p0, nt, sl.chain_parallel_ok, act_prep, rb, i & 1, ahead))) return rc;
            HIPCHK(ctx, hipEventRecord(ctx->ev.prep[b], ctx->st.B));
        }
        const int is_last = (r == n_rounds - 1) ? (last_is_final != 0) : 0;
        const bool same_tile = i > 0 && items[i - 1].p0 == p0;
        if ((rc = run_pair_tile(ctx, core, p0, nt, is_last, A[r & 1], A[(r + 1) & 1], rb, b, same_tile, round_major))) return rc;
        if ((rc = late())) return rc;
        ++*items_done;
        if (++tiles_of_round[(size_t)r] == (int)n_tiles) ++*rounds_done;
    }
    ctx->item_base = (ctx->item_base + n_items) & 1;
    *items_done = 0;                                   // accounted for
    // Cross-batch prefetch.  A batch's first item cannot hide behind one of its own pair stages, and its last pair stage has no
    // later item of its own to cover.  So when this call ends the batch and the next one is already staged (cm_reads_stage),
    // that batch's first item (first tile, slots[0]) is seeded and chained now, from the staging buffers (every pair of a fresh
    // batch is active), into the set of chain records the running pair stage does not read.  cm_reads_swap keeps the result;
    // the next cm_map_rounds uses it if it starts with the same slot, still holding the same contig.  Condition: the staged
    // batch fits the workspace as it is sized now (nothing may be reallocated under the kernels in flight).
    if (prefetch) {
        const int b = ctx->item_base;
        const Slot &sl = ctx->slots[slots[0]];
        const KCore core = make_core(ctx, sl);
        const uint32_t nt = tile_for(ctx->staged.n_pairs);     // = that batch's first tile (prepare_resident)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.staged, 0));
        if ((rc = settle_pair(ctx, b))) return rc;
        if (ctx->pair_pending[b]) {
            HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.pair[b], 0));
            ctx->pair_pending[b] = false;
        }
        const ChainRecs &rbn = ctx->rec[b];
        const ReadsDev rd_next = reads_dev(ctx->staged.rd);
        if (pre_seeded) {                                      // seeds are there (or on their way): the classes, into the records now free
            HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.seed[n_items & 1], 0));
            if ((rc = seed_classes(ctx, 0, nt, ctx->d_ones, n_items & 1, ctx->st.B, &rbn, skip_dead_chains(ctx)))) return rc;
        } else if ((rc = run_seed_tile(ctx, core, rd_next, 0, nt, ctx->d_ones, n_items & 1, ctx->st.B, &rbn, skip_dead_chains(ctx)))) return rc;
        if ((rc = run_chain_tile(ctx, core, rd_next, 0, nt, sl.chain_parallel_ok, ctx->d_ones, rbn, n_items & 1))) return rc;
        HIPCHK(ctx, hipEventRecord(ctx->ev.prep[b], ctx->st.B));
        ctx->pre_launched = true;
        ctx->pre_slot = slots[0];
        ctx->pre_gen = sl.gen;
        ctx->pre_b = b;
        ctx->pre_nt = nt;
    }
    // later work on the main stream (downloads, collects, the next batch) is ordered behind the last pair stage on the device
    // (set item_base ^ 1 = the last item's goes second: stream R's last entry then waits for stream P's last)
    if ((rc = settle_pair(ctx, ctx->item_base, false)) || (rc = settle_pair(ctx, ctx->item_base ^ 1, false))) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev.tail, ctx->st.R));               // (R's last launch waits for P's last)
    HIPCHK(ctx, hipStreamWaitEvent(ctx->st.B, ctx->ev.tail, 0));
    ctx->pair_pending[0] = ctx->pair_pending[1] = false;                     // covered by the wait above
    if (n_rounds & 1) swap(ctx->d_active, ctx->d_active_b);             // the current flags are in the other array now
    *rounds_done = 0;                                  // accounted for
    return CM_OK;
}

int cm_map_rounds(cm_ctx *ctx, const int *slots, int n_rounds, int last_is_final) {
    if (!ctx || (n_rounds > 0 && !slots) || n_rounds < 0) return CM_EINVAL;
    int rc;
    for (int r = 0; r < n_rounds; ++r)
        if ((rc = check_slot(ctx, slots[r], true))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (ctx->n_pairs == 0 || n_rounds == 0) return CM_OK;
    int items_done = 0, rounds_done = 0;
    rc = map_rounds_issue(ctx, slots, n_rounds, last_is_final, &items_done, &rounds_done);
    if (rc == CM_OK) return rc;
    // One exit for every failure inside: nothing of this call may still be running when the caller frees or reuses the batch
    // buffers, and the bookkeeping must describe what was actually issued -- the chain-record set parity (item_base), the
    // flags array that holds the latest flags (one swap per completed round), no prepared first item, no pending pair stage.
    // The states of the batch are unspecified after a failed call (upload or reset before mapping again).
    // (every stream but the copy stream: the staging copy of the next batch is none of this call's work and may go on)
    for (const StreamDef &d : STREAMS)
        if (d.st != &Streams::C) (void)hipStreamSynchronize(ctx->st.*d.st);
    ctx->rerun[0].deferred = ctx->rerun[1].deferred = false;
    ctx->seed[0].cls_deferred = ctx->seed[1].cls_deferred = false;
    ctx->item_base = (ctx->item_base + items_done) & 1;
    if (rounds_done & 1) swap(ctx->d_active, ctx->d_active_b);
    ctx->pair_pending[0] = ctx->pair_pending[1] = false;
    ctx->pre_ready = ctx->pre_launched = false;
    return rc;
}

int cm_map_round(cm_ctx *ctx, int slot, int is_last_round) { return cm_map_rounds(ctx, &slot, 1, is_last_round); }

int cm_sync(cm_ctx *ctx) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    // the main stream is ordered behind every other stream's work at the end of each call (ev.tail); the staging copy of
    // cm_reads_stage is the one thing a caller can have in flight beside it
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.C));
    return check_dev_err(ctx);
}

int cm_reads_reset(cm_ctx *ctx) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (ctx->n_pairs == 0) return CM_OK;
    KCore k{};
    k.P = ctx->P;
    hipLaunchKernelGGL(k_init_state, dim3((unsigned)((ctx->n_pairs + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, k, ctx->d_state, ctx->d_active,
                       ctx->d_cat, ctx->n_pairs);
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}

#ifdef CM_TRACE_HOST
#define TRACE_T0 auto tr_t = std::chrono::steady_clock::now()
#define TRACE_PT(name) do { auto n_ = std::chrono::steady_clock::now(); fprintf(stderr, "[trace] %s %.1f us\n", name, std::chrono::duration<double, std::micro>(n_ - tr_t).count()); tr_t = n_; } while (0)
#else
#define TRACE_T0
#define TRACE_PT(name)
#endif
// stable compaction of the active pairs (block histogram -> scan -> place): ascending pair index, no atomics, no
// host sort; leaves the permutation in d_col_perm and the count in d_col_ctr[0]
static int compact_active(cm_ctx *ctx) {
    const uint64_t n = ctx->n_pairs;
    if (n > 0xfffffff0ull) return fail(ctx, CM_ELIMIT, "cm_collect_*: too many pairs");
    const uint32_t nbk = (uint32_t)((n + CLS_T - 1) / CLS_T);
    // scratch sized for the whole batch, made on first use
    HIPCHK(ctx, ensure(ctx, ctx->col.cls, n));
    HIPCHK(ctx, ensure(ctx, ctx->col.perm, n * 4));
    HIPCHK(ctx, ensure(ctx, ctx->col.blk, (size_t)N_CLS * (nbk + 2) * sizeof(unsigned int)));
    HIPCHK(ctx, ensure(ctx, ctx->col.ctr, CTR_WORDS * sizeof(unsigned int)));
    hipLaunchKernelGGL(k_active_cls, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, ctx->d_active, n, ctx->col.cls);
    counting_sort(ctx, PC_NONE, {ctx->st.B, ctx->col.cls, (uint32_t)n, ctx->col.blk, nbk, ctx->col.ctr, ctx->col.perm, 1});      // one class: active
    return CM_OK;
}
// count + error flags through the pinned landing zone (one synchronisation).  check_dev_err lands its copy in word 0 again
// (PIN_DEV_ERR = PIN_COLLECT_N): it is called here only after the count has been taken out of that word.
static int read_count(cm_ctx *ctx, uint64_t cap, unsigned int *cnt, const char *what) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin + PIN_COLLECT_N, ctx->col.ctr, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin + PIN_COLLECT_ERR, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    *cnt = *(const unsigned int *)(ctx->h_pin + PIN_COLLECT_N);
    if (*(const int *)(ctx->h_pin + PIN_COLLECT_ERR)) return check_dev_err(ctx);
    if (*cnt > cap) return fail(ctx, CM_ELIMIT, "%s: %u active pairs > cap %llu", what, *cnt, (unsigned long long)cap);
    return CM_OK;
}

int cm_collect_active(cm_ctx *ctx, uint64_t cap, uint64_t *out_idx, cm_mapped_read *out_state, uint64_t *out_n) {
    if (!ctx || !out_n || (cap && (!out_idx || !out_state))) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    *out_n = 0;
    if (ctx->n_pairs == 0) return CM_OK;
    int rc = compact_active(ctx);
    if (rc) return rc;
    if (cap) {                                    // grow-only output staging
        HIPCHK(ctx, ensure(ctx, ctx->col.idx, cap * sizeof(unsigned long long)));
        HIPCHK(ctx, ensure(ctx, ctx->col.st, cap * sizeof(cm_mapped_read)));
    }
    if (cap)
        hipLaunchKernelGGL(k_gather_active, dim3((unsigned)((cap + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, ctx->col.perm, ctx->col.ctr,
                           (unsigned long long)cap, ctx->d_state, ctx->col.idx, ctx->col.st);
    unsigned int cnt = 0;
    rc = read_count(ctx, cap, &cnt, "cm_collect_active");
    *out_n = cnt;
    if (rc) return rc;
    if (cnt) {
        HIPCHK(ctx, hipMemcpyAsync(out_idx, ctx->col.idx, (size_t)cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(out_state, ctx->col.st, (size_t)cnt * sizeof(cm_mapped_read), hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    }
    return CM_OK;
}

// compaction + record assembly into `d_dst` (device memory, cap records); complete on return
static int collect_records_into(cm_ctx *ctx, uint64_t index_base, uint64_t cap, cm_record *d_dst, uint64_t *out_n, const char *what) {
    *out_n = 0;
    if (ctx->n_pairs == 0) return CM_OK;
    int rc = compact_active(ctx);
    if (rc) return rc;
    if (cap)
        hipLaunchKernelGGL(k_gather_records, dim3((unsigned)((cap + BLK - 1) / BLK)), dim3(BLK), 0, ctx->st.B, ctx->col.perm, ctx->col.ctr,
                           (unsigned long long)cap, ctx->d_state, (unsigned long long)index_base, d_dst);
    unsigned int cnt = 0;
    rc = read_count(ctx, cap, &cnt, what);
    *out_n = cnt;
    return rc;
}

int cm_collect_records(cm_ctx *ctx, uint64_t index_base, uint64_t cap, cm_record *out, uint64_t *out_n) {
    if (!ctx || !out_n || (cap && !out)) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (cap) HIPCHK(ctx, ensure(ctx, ctx->col.rec, cap * sizeof(cm_record)));
    int rc = collect_records_into(ctx, index_base, cap, ctx->col.rec, out_n, "cm_collect_records");
    if (rc) return rc;
    if (*out_n) {
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->col.rec, (size_t)*out_n * sizeof(cm_record), hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    }
    return CM_OK;
}

int cm_collect_records_device(cm_ctx *ctx, uint64_t index_base, uint64_t cap, void *d_out, uint64_t *out_n) {
    if (!ctx || !out_n || (cap && !d_out)) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (cap) {                                     // a host pointer here would fault inside the kernel: refuse it up front
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, d_out) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->P.device) {
            (void)hipGetLastError();
            return fail(ctx, CM_EINVAL, "cm_collect_records_device: d_out is not memory of device %d", ctx->P.device);
        }
    }
    return collect_records_into(ctx, index_base, cap, (cm_record *)d_out, out_n, "cm_collect_records_device");
}

// "... was not staged with cm_reads_stage_text, flag bit(s) ...": the refusal of a call that needs what the resident batch does not
// keep, composed from what the call needs; CM_OK where it is all there.
struct StagedBit { bool has; const char *bit, *noun; };
static int not_staged(cm_ctx *ctx, const char *fn, std::initializer_list<StagedBit> need) {
    std::string bits, what;
    int missing = 0;
    for (const StagedBit &b : need)
        if (!b.has) {
            bits += (missing ? ", " : "") + std::string(b.bit);
            what += (missing++ ? ", no " : "no ") + std::string(b.noun);
        }
    if (!missing) return CM_OK;
    return fail(ctx, CM_ESTATE, "%s: the resident batch was not staged with cm_reads_stage_text, flag bit%s %s (%s)", fn, missing > 1 ? "s" : "", bits.c_str(), what.c_str());
}

extern "C++" {
// One column of a call's chromosome table, queued for upload when it differs from the column on the device (`now` is used up then;
// `pad` elements more are allocated than it holds).  The waits around the uploads of a call, and `valid` behind them, are prepare()'s.
template <class T>
static int upload_chr_column(cm_ctx *ctx, hipStream_t st, ChrColumn<T> &col, std::vector<T> &now, size_t pad) {
    if (col.holds(now)) return CM_OK;
    col.valid = false;
    col.host.swap(now);
    HIPCHK(ctx, ensure(ctx, col.dev, (col.host.size() + pad) * sizeof(T)));
    if (!col.host.empty()) HIPCHK(ctx, hipMemcpyAsync(col.dev, col.host.data(), col.host.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return CM_OK;
}

// What a row formatter's call says of itself: its name and nouns for the messages, the constants of its format (cm_rows_text.h),
// and the bytes of names and strings all items of a file print at most.
struct RowsCall {
    const char *fn, *range_unit, *limit_unit, *noun;
    uint32_t pair_items, span_items, item_fixed_max, item_chrs;
    uint64_t pair_limit, strings_max;
};
template <class F>
static RowsCall rows_call(const char *fn, const char *range_unit, const char *limit_unit, const char *noun, uint64_t strings_max) {
    return {fn, range_unit, limit_unit, noun, F::PAIR_ITEMS, F::SPAN_ITEMS, F::ITEM_FIXED_MAX, F::ITEM_CHRS, F::PAIR_LIMIT, strings_max};
}
// One output file of a call: its kernels, what they read, the caller's buffer.  File m of a call uses ctx->rows.file[m].
template <class Src>
struct RowsFile {
    void (*k_len)(Src, cmrt::ChrTab, uint64_t, uint32_t, uint32_t *);
    void (*k_rows)(Src, cmrt::ChrTab, uint64_t, uint32_t, const uint32_t *, uint8_t *, uint8_t *);
    Src src;
    void *out;
    uint64_t cap;
};
// What all four entry points check first: the arguments nothing can be said without, the outputs zeroed, a resident batch.
static int rows_enter(cm_ctx *ctx, const char *fn, const cm_chr_info *chrs, uint32_t n_chr, uint64_t *out_bytes, int n_files, uint64_t *n_records, uint64_t stats[4]) {
    if (!ctx || !out_bytes || (n_chr && !chrs)) return CM_EINVAL;
    for (int m = 0; m < n_files; ++m) out_bytes[m] = 0;
    if (n_records) *n_records = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (ctx->n_pairs == 0) return fail(ctx, CM_ESTATE, "%s: no resident batch", fn);
    return CM_OK;
}
// The items (PAM rows, SAM records, the remain records of either mate file) of a call, formatted on the device (the plan:
// cm_rows_text.h) for the files of the call -- one or two -- on the mapping stream, behind everything queued for the batch.  The
// steps, in the order a caller takes them: check, prepare, lengths, spans_out, finish.  Every file's length pass runs before any
// file's span pass: lengths() leaves every file's total in out_bytes before it refuses a file for its size, and a call that refuses
// either file writes neither.  Two waits: in lengths() for the totals (they size the device buffers, and a caller's may be too small), in finish() for the bytes
// (format_remain has one in front, for the active set's size, sort_remain one for the tie groups); between spans_out() and finish() a caller may queue copies of its own.
template <class Src>
struct RowsRun {
    cm_ctx *ctx;
    const RowsCall &c;
    RowsFile<Src> *file;
    int n_files;
    uint64_t first = 0, total[2] = {0, 0};
    uint32_t items = 0, spans = 0, chr_max = 1;
    cmrt::ChrTab ct{};
    RowsBufs &R = ctx->rows;
    hipStream_t st = ctx->st.B;

    // what the batch keeps, pairs or records [first, first + count) of `of`, the callers' buffers, the format's limit
    int check(std::initializer_list<StagedBit> need, uint64_t first_, uint64_t count, uint64_t of) {
        if (int rc = not_staged(ctx, c.fn, need)) return rc;
        if (first_ > of || count > of - first_)
            return fail(ctx, CM_EINVAL, "%s: %s [%llu, +%llu) of %llu", c.fn, c.range_unit, (unsigned long long)first_, (unsigned long long)count, (unsigned long long)of);
        for (int m = 0; m < n_files; ++m)
            if (!file[m].out && file[m].cap) return fail(ctx, CM_EINVAL, "%s: null out", c.fn);
        if (count >= c.pair_limit) return fail(ctx, CM_ELIMIT, "%s: %llu %s in one call", c.fn, (unsigned long long)count, c.limit_unit);
        first = first_;
        items = c.pair_items * (uint32_t)count;
        spans = (items + c.span_items - 1) / c.span_items;
        return CM_OK;
    }
    // the chromosome table in columns -- the names' text and offsets and, where the format prints positions of its own (`shifts`),
    // the chromosomes' starts --, and the buffers
    int prepare(const cm_chr_info *chrs, uint32_t n_chr, bool shifts) {
        std::vector<uint32_t> o((size_t)n_chr + 1, 0u), sh;
        std::vector<uint8_t> text;
        for (uint32_t k = 0; k < n_chr; ++k) {
            if (chrs[k].name) text.insert(text.end(), chrs[k].name, chrs[k].name + strlen(chrs[k].name));
            o[k + 1] = (uint32_t)text.size();
            chr_max = std::max(chr_max, o[k + 1] - o[k]);
            if (shifts) sh.push_back(chrs[k].start_pos);
        }
        if (!(R.chr_text.holds(text) && R.chr_off.holds(o) && (!shifts || R.chr_shift.holds(sh)))) {
            int rc;
            HIPCHK(ctx, hipStreamSynchronize(st));              // (rows of an earlier call are out, but be sure nothing reads the old table)
            if ((rc = upload_chr_column(ctx, st, R.chr_text, text, 4)) || (rc = upload_chr_column(ctx, st, R.chr_off, o, 0)) || (shifts && (rc = upload_chr_column(ctx, st, R.chr_shift, sh, 1))))
                return rc;
            HIPCHK(ctx, hipStreamSynchronize(st));
            R.chr_text.valid = R.chr_off.valid = true;
            if (shifts) R.chr_shift.valid = true;
        }
        ct = cmrt::ChrTab{R.chr_text.dev, R.chr_off.dev, n_chr};
        for (int m = 0; m < n_files; ++m) {
            HIPCHK(ctx, ensure(ctx, R.file[m].off, ((size_t)items + 1) * sizeof(uint32_t)));
            HIPCHK(ctx, ensure(ctx, R.file[m].path, spans));
        }
        HIPCHK(ctx, ensure(ctx, R.tmp, (size_t)(((uint64_t)items + 1) / S32_B + 2) * sizeof(uint32_t)));
        HIPCHK(ctx, ensure(ctx, R.total, (size_t)n_files * sizeof(unsigned long long)));
        return CM_OK;
    }
    int lengths(uint64_t *out_bytes) {
        int rc;
        // offsets are uint32: where the items of a file could come to 2^32 bytes (the names and strings at their most, every number
        // at its widest, the longest chromosome name wherever one is printed) the lengths are summed in 64 bits first
        const bool wide = c.strings_max + (uint64_t)items * (c.item_fixed_max + c.item_chrs * chr_max) >= (1ull << 32);
        unsigned long long *land = ctx->h_pin + PIN_ROWS;
        {
            Timer t(ctx, PC_ROWS, st);
            for (int m = 0; m < n_files; ++m) {
                uint32_t *off = R.file[m].off;
                hipLaunchKernelGGL(file[m].k_len, dim3(items / BLK + 1), dim3(BLK), 0, st, file[m].src, ct, first, items, off);
                if (wide) hipLaunchKernelGGL(k_rows_total, dim3(1), dim3(BLK), 0, st, (const uint32_t *)off, items, (unsigned long long *)R.total + m);
                if ((rc = scan32_on(ctx, st, off, (uint64_t)items + 1, off, R.tmp, 0u, 0))) return rc;
            }
        }
        for (int m = 0; m < n_files; ++m) {
            land[m] = 0;
            if (wide) HIPCHK(ctx, hipMemcpyAsync(land + m, R.total + m, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            else HIPCHK(ctx, hipMemcpyAsync(land + m, R.file[m].off + items, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int m = 0; m < n_files; ++m) out_bytes[m] = total[m] = land[m];
        const auto noun = [&](int m) { return n_files > 1 ? std::string(c.noun) + " of file " + std::to_string(m + 1) : std::string(c.noun); };
        for (int m = 0; m < n_files; ++m)
            if (total[m] >= (1ull << 32))
                return fail(ctx, CM_ELIMIT, "%s: %llu bytes of %s in one call (offsets are 32 bits: format in ranges)", c.fn, (unsigned long long)total[m], noun(m).c_str());
        for (int m = 0; m < n_files; ++m)
            if (total[m] > file[m].cap)
                return fail(ctx, CM_ELIMIT, "%s: %llu bytes of %s > cap %llu", c.fn, (unsigned long long)total[m], noun(m).c_str(), (unsigned long long)file[m].cap);
        return CM_OK;
    }
    int spans_out() {
        for (int m = 0; m < n_files; ++m) HIPCHK(ctx, ensure(ctx, R.file[m].out, (size_t)total[m] + 4));
        {
            Timer t(ctx, PC_ROWS, st);
            for (int m = 0; m < n_files; ++m)
                hipLaunchKernelGGL(file[m].k_rows, dim3(spans), dim3(cmrt::WAVE), 0, st, file[m].src, ct, first, items, (const uint32_t *)R.file[m].off, (uint8_t *)R.file[m].out,
                                   (uint8_t *)R.file[m].path);
        }
        HIPCHK(ctx, hipGetLastError());
        for (int m = 0; m < n_files; ++m) HIPCHK(ctx, hipMemcpyAsync(file[m].out, R.file[m].out, (size_t)total[m], hipMemcpyDeviceToHost, st));
        return CM_OK;
    }
    int finish(uint64_t stats[4]) {
        if (stats) {
            R.h_path.resize((size_t)n_files * spans);
            for (int m = 0; m < n_files; ++m) HIPCHK(ctx, hipMemcpyAsync(R.h_path.data() + (size_t)m * spans, R.file[m].path, spans, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (stats) {
            stats[0] = (uint64_t)n_files * items;
            stats[1] = total[0] + total[1];
            for (uint8_t p : R.h_path) ++stats[p ? 2 : 3];
        }
        return CM_OK;
    }
};
// cm_format_pam, cm_format_sam: pairs [first, first + count) of the resident batch into one file
template <class Src>
static int format_rows(cm_ctx *ctx, const RowsCall &c, RowsFile<Src> file, std::initializer_list<StagedBit> need, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first,
                       uint64_t count, uint64_t *out_bytes, uint64_t stats[4]) {
    RowsRun<Src> run{ctx, c, &file, 1};
    int rc;
    if ((rc = run.check(need, first, count, ctx->n_pairs)) || count == 0) return rc;
    if ((rc = run.prepare(chrs, n_chr, false)) || (rc = run.lengths(out_bytes)) || (rc = run.spans_out())) return rc;
    return run.finish(stats);
}
}  // extern "C++"

// PAM rows: one per pair; needs the kept names.  At most: every name once.
int cm_format_pam(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, void *out, uint64_t cap, uint64_t *out_bytes,
                  uint64_t stats[4]) {
    const char *fn = "cm_format_pam";
    if (int rc = rows_enter(ctx, fn, chrs, n_chr, out_bytes, 1, nullptr, stats)) return rc;
    const ReadFile &r1 = ctx->rd.file[0];
    return format_rows<cmpt::Format::Src>(ctx, rows_call<cmpt::Format>(fn, "pairs", "rows", "rows", r1.name_bytes_max),
                                          {k_pam_len, k_pam_rows, {ctx->d_state, r1.names, r1.name_off}, out, cap}, {{r1.has_names, "2", "names"}}, chrs, n_chr, first, count,
                                          out_bytes, stats);
}

// SAM records: two per pair; needs the kept names and qualities.  At most: every name twice, every read as SEQ and as QUAL.
int cm_format_sam(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, void *out, uint64_t cap, uint64_t *out_bytes,
                  uint64_t stats[4]) {
    const char *fn = "cm_format_sam";
    if (int rc = rows_enter(ctx, fn, chrs, n_chr, out_bytes, 1, nullptr, stats)) return rc;
    const ReadFile *F = ctx->rd.file;
    return format_rows<cmst::Format::Src>(
        ctx, rows_call<cmst::Format>(fn, "pairs", "pairs", "records", 2 * (F[0].name_bytes_max + ctx->rd.bases)),
        {k_sam_len, k_sam_rows, {ctx->d_state, F[0].names, F[0].name_off, {F[0].seq(), F[1].seq()}, {F[0].qual, F[1].qual}, {F[0].off, F[1].off}}, out, cap},
        {{F[0].has_names, "2", "names"}, {ctx->rd.has_quals, "3", "qualities"}}, chrs, n_chr, first, count, out_bytes, stats);
}

// Either mate file's order of the n entries of the active set (S.sel = compact_active's list) into rows.list1 / list2: the plan of
// cm_remain_order.h on the mapping stream.  One wait, for the tie groups' counters: a group above the cap is refused before any
// lane ranks (CM_ELIMIT), and without a group of two the key order is both files' order.
static int sort_remain(cm_ctx *ctx, const char *fn, const cmrm::Src &S, const cmrt::ChrTab &ct, uint32_t n) {
    RowsBufs &R = ctx->rows;
    hipStream_t st = ctx->st.B;
    uint32_t cap = cmro::TIE_CAP;
    if (const char *e = getenv("CM_REMAIN_TIE_CAP")) cap = (uint32_t)std::min<long>(cmro::TIE_CAP, std::max<long>(1, atol(e)));     // (a test knob: the boundary at small sizes)
    HIPCHK(ctx, ensure(ctx, R.rkey0, (size_t)n * sizeof(uint64_t)));
    HIPCHK(ctx, ensure(ctx, R.rkey1, (size_t)n * sizeof(uint64_t)));
    HIPCHK(ctx, ensure(ctx, R.pair0, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.by_key, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.heads, ((size_t)n + 1) * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.gstart, ((size_t)n + 1) * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.list1, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.list2, (size_t)n * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.tmp, (size_t)(((uint64_t)n + 1) / S32_B + 2) * sizeof(uint32_t)));
    HIPCHK(ctx, ensure(ctx, R.ties, 4 * sizeof(unsigned int)));
    size_t ws = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, ws, (uint64_t *)R.rkey0, (uint64_t *)R.rkey1, (uint32_t *)R.pair0, (uint32_t *)R.by_key, (size_t)n, 0u, 64u, st));
    HIPCHK(ctx, ensure(ctx, R.sort_ws, ws));
    const dim3 grid(n / BLK + 1), block(BLK);
    int rc;
    unsigned int *land = (unsigned int *)(ctx->h_pin + PIN_TIES);
    {
        Timer t(ctx, PC_ROWS, st);
        hipLaunchKernelGGL(k_remain_keys, grid, block, 0, st, S, ct.n, n, (uint64_t *)R.rkey0, (uint32_t *)R.pair0);
        HIPCHK(ctx, rocprim::radix_sort_pairs((void *)R.sort_ws, ws, (uint64_t *)R.rkey0, (uint64_t *)R.rkey1, (uint32_t *)R.pair0, (uint32_t *)R.by_key, (size_t)n, 0u, 64u, st));
        hipLaunchKernelGGL(k_remain_heads, grid, block, 0, st, (const uint64_t *)R.rkey1, n, (uint32_t *)R.heads);
        if ((rc = scan32_on(ctx, st, R.heads, (uint64_t)n + 1, R.heads, R.tmp, 0u, 0))) return rc;
        HIPCHK(ctx, hipMemsetAsync(R.ties, 0, 4 * sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_remain_gstart, grid, block, 0, st, (const uint32_t *)R.heads, n, (uint32_t *)R.gstart);
        hipLaunchKernelGGL(k_remain_gsizes, grid, block, 0, st, (const uint32_t *)R.gstart, (const uint32_t *)R.heads + n, (unsigned int *)R.ties);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(land, R.ties, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (land[0] > cap) return fail(ctx, CM_ELIMIT, "%s: a tie group of %u records > cap %u (order the batch on the host)", fn, land[0], cap);
    if (land[1] == 0) {                                   // every key once
        HIPCHK(ctx, hipMemcpyAsync(R.list1, R.by_key, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(R.list2, R.by_key, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        return CM_OK;
    }
    {
        Timer t(ctx, PC_ROWS, st);
        hipLaunchKernelGGL(k_remain_rank<0>, grid, block, 0, st, S, ct, (const uint32_t *)R.by_key, (const uint32_t *)R.heads, (const uint32_t *)R.gstart, n, (uint32_t *)R.list1);
        hipLaunchKernelGGL(k_remain_rank<1>, grid, block, 0, st, S, ct, (const uint32_t *)R.by_key, (const uint32_t *)R.heads, (const uint32_t *)R.gstart, n, (uint32_t *)R.list2);
    }
    HIPCHK(ctx, hipGetLastError());
    return CM_OK;
}

// Remain records: one per mate file of every record [first, first + count) of the active set, the set and order of cm_collect_records
// (compact_active's list is the formats' selection), through the driver with two files.  Three waits: the set's size, the driver's two.
// sorted: the order of cm_remain_order.h in place of the active set's (cm_format_remain_sorted, below), one more wait -- a batch
// refused for a tie group has n_records set, out_bytes and stats zero; out_off (nullable): the records' offsets in either file,
// count + 1 words each.
static int format_remain(cm_ctx *ctx, const char *fn, bool sorted, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, void *out1, uint64_t cap1,
                         void *out2, uint64_t cap2, uint64_t out_bytes[2], int64_t *out_keys, uint32_t *const out_off[2], uint64_t *n_records, uint64_t stats[4]) {
    int rc;
    unsigned int active = 0;
    if ((rc = rows_enter(ctx, fn, chrs, n_chr, out_bytes, 2, n_records, stats)) || (rc = compact_active(ctx)) || (rc = read_count(ctx, ~0ull, &active, fn))) return rc;
    if (n_records) *n_records = active;
    const ReadFile *F = ctx->rd.file;
    const RowsCall c = rows_call<cmrm::Format<0>>(fn, "records", "records", "records", std::max(F[0].name_bytes_max, F[1].name_bytes_max) + 2 * ctx->rd.bases);
    RowsFile<cmrm::Src> file[2] = {{k_remain_len<0>, k_remain_rows<0>, {}, out1, cap1}, {k_remain_len<1>, k_remain_rows<1>, {}, out2, cap2}};
    RowsRun<cmrm::Src> run{ctx, c, file, 2};
    if (count == ~0ull && first <= active) count = active - first;
    if ((rc = run.check({{F[0].has_names, "2", "R1 names"}, {ctx->rd.has_quals, "3", "qualities"}, {F[1].has_names, "4", "R2 names"}}, first, count, active)) || count == 0) return rc;
    if ((rc = run.prepare(chrs, n_chr, true))) return rc;
    RowsBufs &R = ctx->rows;
    hipStream_t st = ctx->st.B;
    if (out_keys) HIPCHK(ctx, ensure(ctx, R.keys, (size_t)run.items * sizeof(int64_t)));
    // either file's selection list: the active set, or the file's own order of it
    file[0].src = file[1].src = cmrm::Src{ctx->col.perm, ctx->d_state, {F[0].names, F[1].names}, {F[0].name_off, F[1].name_off}, {F[0].seq(), F[1].seq()},
                                          {F[0].qual, F[1].qual}, {F[0].off, F[1].off}, R.chr_shift.dev, out_keys ? (int64_t *)R.keys : nullptr};
    if (sorted) {
        if ((rc = sort_remain(ctx, fn, file[0].src, run.ct, active))) return rc;
        file[0].src.sel = R.list1;
        file[1].src.sel = R.list2;
    }
    if ((rc = run.lengths(out_bytes)) || (rc = run.spans_out())) return rc;
    if (out_keys) HIPCHK(ctx, hipMemcpyAsync(out_keys, R.keys, (size_t)run.items * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    for (int m = 0; m < 2; ++m)
        if (out_off && out_off[m]) HIPCHK(ctx, hipMemcpyAsync(out_off[m], R.file[m].off, ((size_t)run.items + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return run.finish(stats);
}

int cm_format_remain(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, void *out1, uint64_t cap1, void *out2, uint64_t cap2,
                     uint64_t out_bytes[2], int64_t *out_keys, uint64_t *n_records, uint64_t stats[4]) {
    return format_remain(ctx, "cm_format_remain", false, chrs, n_chr, first, count, out1, cap1, out2, cap2, out_bytes, out_keys, nullptr, n_records, stats);
}
// ... in the order of cm_sort_remain: records [first, first + count) of either file's own order of the active set (sort_remain
// above: one more wait, for the tie groups' counters).  The sort is redone by every call.
int cm_format_remain_sorted(cm_ctx *ctx, const cm_chr_info *chrs, uint32_t n_chr, uint64_t first, uint64_t count, void *out1, uint64_t cap1, void *out2, uint64_t cap2,
                            uint64_t out_bytes[2], int64_t *out_keys, uint32_t *out_off1, uint32_t *out_off2, uint64_t *n_records, uint64_t stats[4]) {
    uint32_t *const out_off[2] = {out_off1, out_off2};
    return format_remain(ctx, "cm_format_remain_sorted", true, chrs, n_chr, first, count, out1, cap1, out2, cap2, out_bytes, out_keys, out_off, n_records, stats);
}

// test hook: the qualities cm_reads_stage_text kept with the resident batch (flag bit 3), copied back: off1[n] / off2[n] bytes
int cm_quals_peek(cm_ctx *ctx, uint8_t *qual1, uint64_t cap1, uint8_t *qual2, uint64_t cap2) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (ctx->n_pairs == 0) return fail(ctx, CM_ESTATE, "cm_quals_peek: no resident batch");
    if (int rc = not_staged(ctx, "cm_quals_peek", {{ctx->rd.has_quals, "3", "qualities"}})) return rc;
    const ReadFile *F = ctx->rd.file;
    return peek_files(ctx, "cm_quals_peek", "quality", {{qual1, cap1, F[0].qual, nullptr}, {qual2, cap2, F[1].qual, nullptr}});
}

// test hook: the carried states of the resident batch overwritten, behind everything queued for it
int cm_state_poke(cm_ctx *ctx, const cm_mapped_read *states) {
    if (!ctx || !states) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    if (ctx->n_pairs == 0) return fail(ctx, CM_ESTATE, "cm_state_poke: no resident batch");
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_state, states, ctx->n_pairs * sizeof(cm_mapped_read), hipMemcpyHostToDevice, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return CM_OK;
}

int cm_host_alloc(cm_ctx *ctx, uint64_t bytes, void **out) {
    if (!ctx || !out) return CM_EINVAL;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return CM_OK;
}

int cm_host_free(cm_ctx *ctx, void *p) {
    if (!ctx) return CM_EINVAL;
    if (p) HIPCHK(ctx, hipHostFree(p));
    return CM_OK;
}

int cm_host_register(cm_ctx *ctx, void *p, uint64_t bytes) {
    if (!ctx || !p || !bytes) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipHostRegister(p, bytes, hipHostRegisterDefault));
    return CM_OK;
}

int cm_host_unregister(cm_ctx *ctx, void *p) {
    if (!ctx) return CM_EINVAL;
    if (p) HIPCHK(ctx, hipHostUnregister(p));
    return CM_OK;
}

int cm_type_histogram(cm_ctx *ctx, uint64_t out[14]) {
    if (!ctx || !out) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    for (int i = 0; i < 14; ++i) out[i] = 0;
    if (ctx->n_pairs == 0) return CM_OK;
    HIPCHK(ctx, ensure(ctx, ctx->d_type_hist, 16 * sizeof(unsigned long long)));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_type_hist, 0, 16 * sizeof(unsigned long long), ctx->st.B));
    const unsigned grid = (unsigned)std::min<uint64_t>((ctx->n_pairs + BLK - 1) / BLK, 1024);
    hipLaunchKernelGGL(k_type_hist, dim3(grid), dim3(BLK), 0, ctx->st.B, ctx->d_state, ctx->n_pairs, ctx->d_type_hist);
    unsigned long long h[16];
    HIPCHK(ctx, hipMemcpyAsync(h, ctx->d_type_hist, sizeof h, hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    for (int i = 0; i < 14; ++i) out[i] = h[i];
    return check_dev_err(ctx);
}

int cm_reads_download(cm_ctx *ctx, cm_mapped_read *out_state, int32_t *out_category, uint8_t *out_active) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    const uint64_t n = ctx->n_pairs;
    if (n) {
        if (out_state) HIPCHK(ctx, hipMemcpyAsync(out_state, ctx->d_state, n * sizeof(cm_mapped_read), hipMemcpyDeviceToHost, ctx->st.B));
        if (out_category) HIPCHK(ctx, hipMemcpyAsync(out_category, ctx->d_cat, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->st.B));
        if (out_active) HIPCHK(ctx, hipMemcpyAsync(out_active, ctx->d_active, n, hipMemcpyDeviceToHost, ctx->st.B));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return check_dev_err(ctx);
}

int cm_map_batch(cm_ctx *ctx, int slot, int is_last_round, const cm_reads *reads, const cm_mapped_read *prior, cm_mapped_read *out_state,
                 int32_t *out_category) {
    int rc = cm_reads_upload(ctx, reads, prior);
    if (rc) return rc;
    if ((rc = cm_map_round(ctx, slot, is_last_round))) return rc;
    return cm_reads_download(ctx, out_state, out_category, nullptr);
}

int cm_seed_batch(cm_ctx *ctx, int slot, uint32_t *out_start, uint32_t *out_cnt, uint32_t *out_raw, uint32_t cap_probes, uint32_t *out_n_slots) {
    if (!ctx || !out_start || !out_cnt || !out_raw || !out_n_slots) return CM_EINVAL;
    int rc = check_slot(ctx, slot, false);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    *out_n_slots = (uint32_t)ctx->n_seeds;
    const uint64_t need = ctx->n_pairs * 4ull * (uint64_t)ctx->n_seeds;
    if (need > cap_probes) return fail(ctx, CM_EINVAL, "cm_seed_batch: need room for %llu probes", (unsigned long long)need);
    const KCore core = make_core(ctx, ctx->slots[slot]);
    for (uint64_t p0 = 0; p0 < ctx->n_pairs; p0 += ctx->tile) {
        const uint32_t nt = (uint32_t)((ctx->n_pairs - p0 < ctx->tile) ? ctx->n_pairs - p0 : ctx->tile);
        if ((rc = run_seed_tile(ctx, core, current_reads(ctx), p0, nt, ctx->d_active, 0, ctx->st.B, nullptr, false))) return rc;
        const size_t cnt = (size_t)nt * 4 * ctx->n_seeds, o = (size_t)p0 * 4 * ctx->n_seeds;
        HIPCHK(ctx, hipMemcpyAsync(out_start + o, ctx->seed[0].sstart, cnt * 4, hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(out_cnt + o, ctx->seed[0].scnt, cnt * 4, hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(out_raw + o, ctx->seed[0].sraw, cnt * 4, hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    }
    return CM_OK;
}

int cm_chain_batch(cm_ctx *ctx, int slot, cm_chain *out_chains, int32_t *out_nchain, int32_t *out_high) {
    if (!ctx || !out_chains || !out_nchain || !out_high) return CM_EINVAL;
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    const KCore core = make_core(ctx, ctx->slots[slot]);
    for (uint64_t p0 = 0; p0 < ctx->n_pairs; p0 += ctx->tile) {
        const uint32_t nt = (uint32_t)((ctx->n_pairs - p0 < ctx->tile) ? ctx->n_pairs - p0 : ctx->tile);
        HIPCHK(ctx, hipMemsetAsync(ctx->rec[0].chains, 0, (size_t)nt * 4 * CM_BESTCHAINLIM * sizeof(cm_chain), ctx->st.B));
        const ChainRecs &rb0 = ctx->rec[0];
        if ((rc = run_seed_tile(ctx, core, current_reads(ctx), p0, nt, ctx->d_active, 0, ctx->st.B, &rb0, false))) return rc;
        if ((rc = run_chain_tile(ctx, core, current_reads(ctx), p0, nt, ctx->slots[slot].chain_parallel_ok, ctx->d_active, rb0, 0))) return rc;
        const size_t np = (size_t)nt * 4, o = (size_t)p0 * 4;
        HIPCHK(ctx, hipMemcpyAsync(out_chains + o * CM_BESTCHAINLIM, ctx->rec[0].chains, np * CM_BESTCHAINLIM * sizeof(cm_chain), hipMemcpyDeviceToHost,
                                   ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(out_nchain + o, ctx->rec[0].nchain, np * 4, hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipMemcpyAsync(out_high + o, ctx->rec[0].high, np * 4, hipMemcpyDeviceToHost, ctx->st.B));
        HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    }
    return check_dev_err(ctx);
}

// test hook: kernel, validation and launch live in cm_dp_probe.hip (a translation unit of its own: the kernels of this file are
// compiled exactly as they are without the hook); here only what needs the context
extern "C" int cm_dp_probe_run(hipStream_t so, const cm_params *P, const uint8_t *arena, uint64_t arena_len, const cm_dp_req *req, uint32_t n_req,
                               int str_cap, uint32_t lds_fill, int arrangement, uint32_t grid, cm_dp_res *out, char *err, size_t err_cap);
int cm_dp_batch(cm_ctx *ctx, const cm_params *P, const uint8_t *arena, uint64_t arena_len, const cm_dp_req *req, uint32_t n_req, int str_cap,
                uint32_t lds_fill, int arrangement, uint32_t grid, cm_dp_res *out) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    char msg[256] = "";
    const int rc = cm_dp_probe_run(ctx->st.B, P, arena, arena_len, req, n_req, str_cap, lds_fill, arrangement, grid, out, msg, sizeof msg);
    return rc == CM_OK ? CM_OK : fail(ctx, rc, "cm_dp_batch: %s", msg);
}

// test hook: the annotation look-ups against the slot's own AnnotDev (kernel, validation and launch in cm_annot_probe.hip)
extern "C" int cm_annot_probe_run(hipStream_t so, const cm_params *P, const void *annot, size_t annot_bytes, const cm_annot_req *req, uint32_t n_req,
                                  cm_annot_res *out, uint32_t *out_tids, char *err, size_t err_cap);
int cm_annot_batch(cm_ctx *ctx, int slot, const cm_params *P, const cm_annot_req *req, uint32_t n_req, cm_annot_res *out, uint32_t *out_tids) {
    if (!ctx) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    if (!ctx->slots[slot].has_annot) return fail(ctx, CM_ESTATE, "annotation of slot %d not loaded", slot);      // (no index, no reads needed)
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    char msg[256] = "";
    const int rc = cm_annot_probe_run(ctx->st.B, P, &ctx->slots[slot].A, sizeof(cmc::AnnotDev), req, n_req, out, out_tids, msg, sizeof msg);
    return rc == CM_OK ? CM_OK : fail(ctx, rc, "cm_annot_batch: %s", msg);
}

// stage 2's seeds and chains (kernels, validation and launch in cm_circ_chain.hip); here only what needs the context: the slot's
// annotation, for genome == NULL its resident sequence, and the workspace the calls of a context share
extern "C" int cm_circ_chain_run(hipStream_t so, cm_circ_chain_ws *wsp, const cm_params *P, const void *annot, size_t annot_bytes, const uint8_t *d_contig, uint32_t contig_len,
                                 int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs, uint64_t seqs_len,
                                 const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                                 uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                                 uint64_t *n_frags_out, uint64_t stats[8], char *err, size_t err_cap);
int cm_circ_chain_batch(cm_ctx *ctx, int slot, int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs, uint64_t seqs_len,
                        const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                        uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                        uint64_t *n_frags_out, uint64_t stats[8]) {
    if (!ctx) return CM_EINVAL;
    if (slot < 0 || slot >= MAX_SLOTS) return fail(ctx, CM_EINVAL, "slot %d out of range", slot);
    const Slot &s = ctx->slots[slot];
    if (!s.has_annot) return fail(ctx, CM_ESTATE, "annotation of slot %d not loaded", slot);
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    char msg[256] = "";
    const int rc = cm_circ_chain_run(ctx->st.B, &ctx->circ_ws, &ctx->P, &s.A, sizeof(cmc::AnnotDev), s.loaded ? s.X.genome : nullptr, s.loaded ? s.X.ref_len : 0, window_size,
                                     genome, ref_len, seqs, seqs_len, req, n_req, res, chain_score, chain_len, chain_frag_off, cap_chains, rpos, qpos,
                                     cap_frags, n_chains_out, n_frags_out, stats, msg, sizeof msg);
    return rc == CM_OK ? CM_OK : fail(ctx, rc, "cm_circ_chain_batch: %s", msg);
}

/* diagnostic: per-pair k_pair lane time in 100 MHz ticks (only when CM_LANE_CLK was set at upload) */
// diagnostic builds (-DCM_CHAIN_DIAG ...): the CN_WORDS raw counter words, [8 ..] = whatever the build accumulates there (enum Counter)
int cm_debug_counters(cm_ctx *ctx, unsigned long long *out) {
    if (!ctx || !out) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->d_counters, CN_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return CM_OK;
}

int cm_debug_lane_clk(cm_ctx *ctx, unsigned long long *out) {
    if (!ctx || !out || !ctx->d_lane_clk) return CM_EINVAL;
#if defined(CM_DIAG)
    HIPCHK(ctx, hipMemcpy(out, ctx->d_lane_clk, ctx->n_pairs * 8 * 33, hipMemcpyDeviceToHost));
#else
    HIPCHK(ctx, hipMemcpy(out, ctx->d_lane_clk, ctx->n_pairs * 8, hipMemcpyDeviceToHost));
#endif
    return CM_OK;
}

int cm_prof_enable(cm_ctx *ctx, int on) {
    if (!ctx) return CM_EINVAL;
    ctx->prof = on != 0;
    return CM_OK;
}

int cm_prof_reset(cm_ctx *ctx) {
    if (!ctx) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    for (auto &r : ctx->recs) {
        ctx->ev_free.push_back(r.a);
        ctx->ev_free.push_back(r.b);
    }
    ctx->recs.clear();
    for (int i = 0; i < PC_COUNT; ++i) {
        ctx->ms[i] = 0;
        ctx->launches[i] = 0;
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_counters, 0, CN_WORDS * sizeof(unsigned long long), ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    return CM_OK;
}

int cm_prof_get(cm_ctx *ctx, double ms[8], uint64_t launches[8]) {
    if (!ctx || !ms || !launches) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    for (auto &r : ctx->recs) {
        float t = 0;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ctx->ms[r.cls] += (double)t;
        ctx->ev_free.push_back(r.a);
        ctx->ev_free.push_back(r.b);
    }
    ctx->recs.clear();
    for (int i = 0; i < PC_COUNT; ++i) {
        ms[i] = ctx->ms[i];
        launches[i] = ctx->launches[i];
    }
    return CM_OK;
}

int cm_prof_counters(cm_ctx *ctx, uint64_t c[8]) {
    if (!ctx || !c) return CM_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->P.device));
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, ctx->d_counters, sizeof h, hipMemcpyDeviceToHost, ctx->st.B));
    HIPCHK(ctx, hipStreamSynchronize(ctx->st.B));
    for (int i = 0; i < 8; ++i) c[i] = h[i];
    c[CN_DEAD_CHAINS] = 0;          // the public words are 0 - 6, [7] is reserved (0): the device's word 7 is read through cm_debug_counters
    return CM_OK;
}

}  // extern "C"
