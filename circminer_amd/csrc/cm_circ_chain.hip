// cm_circ_chain.hip — cm_circ_chain_batch (include/circminer_hot.h): the regional seed tables, the 8-mer seeds and the k-best chains
// of stage 2 (reference src/hash_table.cpp:58-112, src/process_circ.cpp:677-737, src/chain.cpp:310-539) for all problems of a batch.
// The bodies are cm_circ_chain.h's; this file is the orchestration around them and the launch.
//
// A translation unit of its own, compiled once, for the reason cm_dp_probe.hip gives: nothing here depends on CM_MAX_CHAIN_FRAGS,
// AnnotDev is the same struct in every build, and the kernels of cm_hot.hip compile exactly as they do without it.
//
// Tables (per distinct gene of a call, in groups that fit a byte budget): count -> scan -> place -> order.  Placement takes a
// bucket's places with an atomic counter, so a bucket comes out in any order; the order pass ranks it in LDS (a surviving bucket
// has at most 1000 entries), one wave per 64 buckets.
// Chaining: resident waves take problems from a work cursor (no grid barrier, no co-residency assumed); every wave owns a fixed
// slice of the workspace (cells, improvement log, `repeats` list).  Nothing grows inside a kernel: a problem whose cells or log
// do not fit the slice is refused (flag bit 0, nothing else written, counter bumped) and the host answers it.  Every global store
// is bounded by a capacity that is a kernel argument, and so is every gather: a request, its gene, its mate and its table are
// held against n_req / n_genes / seqs_len / off_words / loc_words before anything is read through them, a list against the
// gene's windows before its hits are (a problem that fails one of these is refused; the host-side construction never makes one).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "circminer_hot.h"
#define cmc cmc_cc                     // the bodies' namespace: every build of them has its own (cm_dispatch.cpp)
#include "cm_core.h"
#include "cm_circ_chain.h"
#include "cm_circ_chain_ws.h"

namespace {

constexpr int BLK_TAB = 256;
constexpr uint32_t EMPTIED = 0xFFFFFFFFu;      // count word of a bucket the scan emptied
constexpr uint32_t MAX_WORKERS = 1024;         // resident waves of the chaining kernel
constexpr uint32_t CELL_CAP = 65536;           // DP cells of one resident problem: 128 lists x 500 hits (default seed_lim) and room to spare
constexpr uint32_t LOG_CAP_DEFAULT = 65536;    // improvement-log entries of one resident problem (NOTES: the data behind it)
constexpr uint64_t TABLE_BYTES_DEFAULT = 1ull << 30;

struct CcGene {                 // one gene of the group being worked on
    uint64_t seq_off;           // its first base in the sequence buffer
    uint32_t len, gene_start;   // len 0: a gene genome_at would refuse (all NUL: no hit)
    uint64_t off_base, cnt_base, loc_base;      // its parts of the three table pools (in words)
};

struct CcTab {
    const CcGene *genes;
    uint32_t n_genes;
    const uint8_t *seq;
    uint64_t seq_len;           // bytes behind seq
    uint32_t *off, *cnt, *loc;
    uint64_t off_words, cnt_words, loc_words;
    int ws;
    uint32_t n_buckets;         // 4^ws
};

// count pass: position i of gene blockIdx.y
__global__ void __launch_bounds__(BLK_TAB) k_cc_tab_count(CcTab t) {
    const CcGene g = t.genes[blockIdx.y];
    const uint32_t nw = cmc::cc_n_windows(g.len, t.ws);
    if (g.seq_off + g.len > t.seq_len) return;
    const uint8_t *s = t.seq + g.seq_off;
    for (uint32_t i = blockIdx.x * BLK_TAB + threadIdx.x; i < nw; i += gridDim.x * BLK_TAB) {
        const int hv = cmc::cc_tab_bucket(s, i, t.ws);
        if (hv >= 0 && g.cnt_base + (uint32_t)hv < t.cnt_words) atomicAdd(&t.cnt[g.cnt_base + (uint32_t)hv], 1u);
    }
}

// scan pass: one workgroup per gene; thread x owns the buckets [x * per, (x + 1) * per).  Leaves off[] and turns the count words
// into the place counters of the next pass (0, or EMPTIED)
__global__ void __launch_bounds__(BLK_TAB) k_cc_tab_scan(CcTab t) {
    __shared__ uint32_t part[BLK_TAB];
    const CcGene g = t.genes[blockIdx.x];
    const uint32_t per = t.n_buckets / BLK_TAB;           // 4^ws >= 4096: a multiple of 256
    const uint32_t h0 = threadIdx.x * per;
    if (g.cnt_base + t.n_buckets > t.cnt_words || g.off_base + t.n_buckets + 1 > t.off_words) return;
    uint32_t *cnt = t.cnt + g.cnt_base, *off = t.off + g.off_base;
    uint32_t sum = 0;
    for (uint32_t h = h0; h < h0 + per; ++h) sum += cmc::cc_tab_kept(cnt[h]);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < BLK_TAB; d <<= 1) {
        const uint32_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t h = h0; h < h0 + per; ++h) {
        const uint32_t n = cnt[h], kept = cmc::cc_tab_kept(n);
        off[h] = run;
        run += kept;
        cnt[h] = (n > 0 && kept == 0) ? EMPTIED : 0u;
    }
    if (threadIdx.x == BLK_TAB - 1) off[t.n_buckets] = run;
}

// place pass: position i takes the next place of its bucket
__global__ void __launch_bounds__(BLK_TAB) k_cc_tab_place(CcTab t) {
    const CcGene g = t.genes[blockIdx.y];
    const uint32_t nw = cmc::cc_n_windows(g.len, t.ws);
    if (g.seq_off + g.len > t.seq_len || g.cnt_base + t.n_buckets > t.cnt_words || g.off_base + t.n_buckets + 1 > t.off_words) return;
    const uint8_t *s = t.seq + g.seq_off;
    uint32_t *cnt = t.cnt + g.cnt_base;
    const uint32_t *off = t.off + g.off_base;
    for (uint32_t i = blockIdx.x * BLK_TAB + threadIdx.x; i < nw; i += gridDim.x * BLK_TAB) {
        const int hv = cmc::cc_tab_bucket(s, i, t.ws);
        if (hv < 0 || cnt[hv] == EMPTIED) continue;
        const uint32_t place = atomicAdd(&cnt[hv], 1u), at = off[hv] + place;
        if (place < off[hv + 1] - off[hv] && at < nw && g.loc_base + at < t.loc_words) t.loc[g.loc_base + at] = i;
    }
}

// order pass: one wave per 64 buckets of gene blockIdx.y; a bucket of more than one entry is ranked in LDS
__global__ void __launch_bounds__(64) k_cc_tab_order(CcTab t) {
    __shared__ uint32_t vals[cmc::CC_MAXHIT];
    const CcGene g = t.genes[blockIdx.y];
    const uint32_t nw = cmc::cc_n_windows(g.len, t.ws);
    if (g.off_base + t.n_buckets + 1 > t.off_words) return;
    const uint32_t *off = t.off + g.off_base;
    const uint32_t h = blockIdx.x * 64 + threadIdx.x;
    const uint32_t mine = h < t.n_buckets ? off[h + 1] - off[h] : 0;
    unsigned long long todo = __ballot(mine > 1);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t hb = blockIdx.x * 64 + (uint32_t)l, first = off[hb], n = off[hb + 1] - first;
        if (n > cmc::CC_MAXHIT || first + n > nw || g.loc_base + first + n > t.loc_words) continue;       // (uniform: cannot happen after the scan)
        uint32_t *loc = t.loc + g.loc_base + first;
        for (uint32_t k = threadIdx.x; k < n; k += 64) vals[k] = loc[k];
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < n; k += 64) {
            const uint32_t v = vals[k], r = cmc::cc_tab_rank(vals, n, v);
            if (r < n) loc[r] = v;
        }
        __syncthreads();
    }
}

// ---- chaining
struct CcRes { uint32_t n_chains, n_stored, listed, flags; };
struct CcWork {
    const cm_circ_chain_req *req;
    const uint32_t *order;          // the requests of this group
    uint32_t n_order, n_req, n_genes;
    uint64_t seqs_len, off_words, loc_words;      // bytes behind seqs, words behind tab_off / tab_loc
    const uint32_t *gene_of;        // request -> gene of the group
    const CcGene *genes;
    const uint32_t *tab_off, *tab_loc;
    const uint8_t *seqs;
    int ws;
    double *cell_score;             // per resident wave: cell_cap cells, log_cap events, seen_cap words
    int32_t *cell_prev;
    cmc::CcEv *log;
    uint32_t *seen;
    uint32_t cell_cap, log_cap, seen_cap;
    CcRes *res;                     // per request
    float *cscore;                  // per request CC_TOPCHAIN
    uint32_t *clen;
    const uint64_t *frag_base;      // per request: CC_TOPCHAIN * positions fragment places from here
    uint32_t *rpos;
    int32_t *qpos;
    uint64_t frag_cap;
    unsigned int *cursor;
    unsigned long long *counters;   // [0] cells, [1] log events, [2] refused
};

__device__ inline double wv_max(double v) {
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}
__device__ inline double wv_excl_max(double v, int lane) {          // maximum over the lanes before this one, CC_NEG for lane 0
    for (int d = 1; d < 64; d <<= 1) {
        const double y = __shfl_up(v, d);
        if (lane >= d) v = fmax(v, y);
    }
    const double e = __shfl_up(v, 1);
    return lane ? e : cmc::CC_NEG;
}
__device__ inline uint32_t wv_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ inline uint32_t wv_excl_sum(uint32_t v, int lane) {
    const uint32_t own = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    return v - own;
}

// what cc_replay (cm_circ_chain.h) asks of a wave: every lane runs the replay with the same values, lane 0 stores
struct WaveReplay {
    int lane;
    uint32_t kc, log_n;
    const uint32_t *s_first, *s_n, *s_cell0;
    const int32_t *s_q;
    const uint32_t *tloc;
    const double *score;
    const int32_t *prev_;
    const cmc::CcEv *log;
    uint32_t *seen;
    uint32_t seen_cap, seen_n;
    uint32_t *rpos;
    int32_t *qpos_;
    uint64_t frag_cap, fb;
    uint32_t npos;
    float *cscore;
    uint32_t *clen;
    __device__ bool next(double after_s, uint32_t after_o, bool any_after, double &bs, uint32_t &bo) const {
        bool have = false;
        for (uint32_t e = (uint32_t)lane; e < log_n; e += 64) {
            const double s = log[e].score;
            if (cmc::cc_better(s, e, after_s, after_o, any_after, have, bs, bo)) {
                have = true;
                bs = s;
                bo = e;
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const int oh = __shfl_xor((int)have, d);
            const double os = __shfl_xor(bs, d);
            const uint32_t oo = __shfl_xor(bo, d);
            if (oh && (!have || cmc::cc_before(os, oo, bs, bo))) {
                have = true;
                bs = os;
                bo = oo;
            }
        }
        return have;
    }
    __device__ cmc::CcEv event(uint32_t o) const { return log[o]; }
    __device__ uint32_t lists() const { return kc; }
    __device__ uint32_t hits(uint32_t l) const { return s_n[l]; }
    __device__ uint32_t hit(uint32_t l, uint32_t i) const { return tloc[s_first[l] + i]; }
    __device__ int32_t qpos(uint32_t l) const { return s_q[l]; }
    __device__ int32_t prev(uint32_t l, uint32_t i) const { return prev_[s_cell0[l] + i]; }
    __device__ double cell(uint32_t l, uint32_t i) const { return score[s_cell0[l] + i]; }
    __device__ bool seen_has(uint32_t v) const {
        bool hit = false;
        for (uint32_t k = (uint32_t)lane; k < seen_n && k < seen_cap; k += 64) hit |= seen[k] == v;
        return __any(hit);
    }
    __device__ void seen_push(uint32_t v) {
        if (lane == 0 && seen_n < seen_cap) seen[seen_n] = v;
        ++seen_n;
    }
    __device__ void seen_sync() const { __syncthreads(); }          // lane 0's entries of `seen` are read by every lane
    __device__ void frag(uint32_t chain, uint32_t at, uint32_t rp, int32_t qp) const {
        const uint64_t x = fb + (uint64_t)chain * npos + at;
        if (lane == 0 && chain < (uint32_t)cmc::CC_TOPCHAIN && at < npos && x < frag_cap) {
            rpos[x] = rp;
            qpos_[x] = qp;
        }
    }
    __device__ void chain(uint32_t chain, float sc, uint32_t len) const {
        if (lane == 0 && chain < (uint32_t)cmc::CC_TOPCHAIN) {
            cscore[chain] = sc;
            clen[chain] = len;
        }
    }
};

__global__ void __launch_bounds__(64) k_cc_chain(cmc::KCore kcore, CcWork w) {
    __shared__ uint32_t s_first[cmc::CC_MAX_LISTS], s_n[cmc::CC_MAX_LISTS], s_cell0[cmc::CC_MAX_LISTS];
    __shared__ int32_t s_q[cmc::CC_MAX_LISTS];
    __shared__ uint32_t s_take, s_kc, s_cells;
    const cmc::Core c = cmc::to_core(kcore);
    const int lane = (int)threadIdx.x;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int kmer = w.ws;
    const uint32_t max_best = (uint32_t)c.P.max_chain_len;
    double *score = w.cell_score + (size_t)blockIdx.x * w.cell_cap;
    int32_t *prev = w.cell_prev + (size_t)blockIdx.x * w.cell_cap;
    cmc::CcEv *log = w.log + (size_t)blockIdx.x * w.log_cap;
    uint32_t *seen = w.seen + (size_t)blockIdx.x * w.seen_cap;
    for (;;) {
        __syncthreads();
        if (lane == 0) s_take = atomicAdd(w.cursor, 1u);
        __syncthreads();
        const uint32_t take = s_take;
        if (take >= w.n_order) break;
        const uint32_t r = w.order[take];
        if (r >= w.n_req) continue;                                   // (cannot happen: the order lists requests)
        const cm_circ_chain_req q = w.req[r];
        const uint32_t gi = w.gene_of[r];
        const CcGene g = gi < w.n_genes ? w.genes[gi] : CcGene{0, 0, 0, 0, 0, 0};
        const uint32_t n_win = cmc::cc_n_windows(g.len, w.ws), n_buckets = 1u << (2 * w.ws);
        const bool gathers_ok = gi < w.n_genes && g.off_base + n_buckets + 1 <= w.off_words && g.loc_base + n_win <= w.loc_words &&
                                q.seq_off <= w.seqs_len && q.seq_len <= w.seqs_len - q.seq_off && q.qe <= q.seq_len;
        const uint32_t *toff = w.tab_off + (gathers_ok ? g.off_base : 0), *tloc = w.tab_loc + (gathers_ok ? g.loc_base : 0);
        const uint8_t *seq = w.seqs + (gathers_ok ? q.seq_off : 0);
        const uint32_t npos = cmc::cc_n_positions(q.qs, q.qe, w.ws);
        const uint64_t fb = w.frag_base[r];
        CcRes out{0, 0, 0, 0};
        bool refused = npos > (uint32_t)cmc::CC_MAX_LISTS || !gathers_ok;
        uint32_t listed = 0, kc = 0, cells = 0, log_n = 0;
        if (!refused && npos > 0) {
            // plan: two positions per lane, valid seeds packed in position order
            for (int half = 0; half < 2; ++half) {
                const uint32_t p = (uint32_t)(half * 64 + lane);
                cmc::CcSeed s{0, 0, 0, false};
                if (p < npos) s = cmc::cc_plan_seed(seq, q.qs, p, w.ws, toff, c.P.seed_lim);
                const unsigned long long m = __ballot(s.listed);
                const uint32_t at = listed + (uint32_t)__popcll(m & below);
                if (s.listed && at < (uint32_t)cmc::CC_MAX_LISTS) {
                    s_first[at] = s.first;
                    s_n[at] = s.n;
                    s_q[at] = s.qpos;
                }
                listed += (uint32_t)__popcll(m);
            }
            __syncthreads();
            if (lane == 0) {
                uint32_t k = listed, sum = 0;
                bool beyond = false;                                  // a list that reaches past the gene's hits (cannot happen after the scan)
                while (k >= 1 && s_n[k - 1] == 0) --k;
                for (uint32_t a = 0; a < k; ++a) {
                    s_cell0[a] = sum;
                    sum += s_n[a] <= cmc::CC_MAXHIT ? s_n[a] : cmc::CC_MAXHIT;
                    beyond |= s_n[a] > cmc::CC_MAXHIT || s_first[a] > n_win || s_n[a] > n_win - s_first[a];
                }
                s_kc = k;
                s_cells = beyond ? 0xFFFFFFFFu : sum;                 // refused below
            }
            __syncthreads();
            kc = s_kc;
            cells = s_cells;
            if (cells > w.cell_cap) refused = true;
        }
        if (!refused && kc > 0) {
            for (uint32_t x = (uint32_t)lane; x < cells; x += 64) {
                score[x] = (double)kmer;
                prev[x] = -1;
            }
            __syncthreads();
            auto nothing = [](double, uint32_t) {};
            for (int a = (int)kc - 2; a >= 0 && !refused; --a) {
                const uint32_t na = s_n[a];
                if (na == 0) continue;
                const uint32_t *hita = tloc + s_first[a];
                const int32_t qa = s_q[a];
                const uint32_t b0 = (uint32_t)a + 1 + (uint32_t)lane, b1 = b0 + 64;
                const bool in0 = b0 < kc, in1 = b1 < kc;
                const uint32_t nb0 = in0 ? s_n[b0] : 0, nb1 = in1 ? s_n[b1] : 0;
                const uint32_t *hit0 = tloc + (in0 ? s_first[b0] : 0), *hit1 = tloc + (in1 ? s_first[b1] : 0);
                const double *sc0 = score + (in0 ? s_cell0[b0] : 0), *sc1 = score + (in1 ? s_cell0[b1] : 0);
                const int rd0 = in0 ? s_q[b0] - qa - kmer : 0, rd1 = in1 ? s_q[b1] - qa - kmer : 0;
                uint32_t cur0 = 0, cur1 = 0;
                for (uint32_t i = 0; i < na; ++i) {
                    const int32_t here = (int32_t)hita[i];
                    const bool act0 = cmc::cc_cursor_step(here, c.P.max_intron, hit0, nb0, cur0);
                    const bool act1 = cmc::cc_cursor_step(here, c.P.max_intron, hit1, nb1, cur1);
                    if (!__any(act0 || act1)) continue;
                    const cmc::CcCell x = cmc::cc_cell_bounds(c, here, kmer, (int)q.qe, qa);
                    // pass 1: the best of every later list
                    const double m0 = act0 ? cmc::cc_cell_list(c, x, kmer, rd0, hit0, nb0, cur0, sc0, cmc::CC_NEG, nothing) : cmc::CC_NEG;
                    const double m1 = act1 ? cmc::cc_cell_list(c, x, kmer, rd1, hit1, nb1, cur1, sc1, cmc::CC_NEG, nothing) : cmc::CC_NEG;
                    const double all0 = wv_max(m0), all = fmax(all0, wv_max(m1));
                    const double init = (double)kmer;
                    if (!(all > init)) continue;
                    const double f0 = fmax(init, wv_excl_max(m0, lane)), f1 = fmax(init, fmax(all0, wv_excl_max(m1, lane)));
                    // pass 2: the improvements each list contributes above the score it would have met serially
                    uint32_t n0 = 0, n1 = 0, j0 = 0, j1 = 0;
                    double e0 = f0, e1 = f1;
                    if (act0 && m0 > f0) e0 = cmc::cc_cell_list(c, x, kmer, rd0, hit0, nb0, cur0, sc0, f0, [&](double, uint32_t j) { ++n0; j0 = j; });
                    if (act1 && m1 > f1) e1 = cmc::cc_cell_list(c, x, kmer, rd1, hit1, nb1, cur1, sc1, f1, [&](double, uint32_t j) { ++n1; j1 = j; });
                    const uint32_t tot0 = wv_sum(n0), tot = tot0 + wv_sum(n1);
                    if (log_n + tot > w.log_cap) {
                        refused = true;
                        break;
                    }
                    // pass 3: into the log, in the reference's order
                    const uint32_t o0 = log_n + wv_excl_sum(n0, lane), o1 = log_n + tot0 + wv_excl_sum(n1, lane);
                    if (n0) {
                        uint32_t at = o0;
                        cmc::cc_cell_list(c, x, kmer, rd0, hit0, nb0, cur0, sc0, f0, [&](double sc, uint32_t) {
                            if (at < w.log_cap) log[at] = cmc::CcEv{sc, (uint32_t)a, i};
                            ++at;
                        });
                    }
                    if (n1) {
                        uint32_t at = o1;
                        cmc::cc_cell_list(c, x, kmer, rd1, hit1, nb1, cur1, sc1, f1, [&](double sc, uint32_t) {
                            if (at < w.log_cap) log[at] = cmc::CcEv{sc, (uint32_t)a, i};
                            ++at;
                        });
                    }
                    log_n += tot;
                    // the cell keeps its last improvement
                    const unsigned long long w1 = __ballot(n1 > 0), w0 = __ballot(n0 > 0);
                    const uint32_t cell = s_cell0[a] + i;
                    if (cell < w.cell_cap) {
                        if (w1) {
                            if (lane == 63 - __clzll((long long)w1)) {
                                score[cell] = e1;
                                prev[cell] = cmc::cc_prev_pack(b1, j1);
                            }
                        } else if (w0 && lane == 63 - __clzll((long long)w0)) {
                            score[cell] = e0;
                            prev[cell] = cmc::cc_prev_pack(b0, j0);
                        }
                    }
                }
                __syncthreads();          // the cells of list a are read by the lists before it
            }
        }
        if (!refused && kc > 0) {
            __syncthreads();
            double top = cmc::CC_NEG;
            for (uint32_t e = (uint32_t)lane; e < log_n; e += 64) top = fmax(top, log[e].score);
            top = wv_max(top);
            WaveReplay ops{lane, kc, log_n, s_first, s_n, s_cell0, s_q, tloc, score, prev, log, seen, w.seen_cap, 0,
                           w.rpos, w.qpos, w.frag_cap, fb, npos, w.cscore + (size_t)r * cmc::CC_TOPCHAIN, w.clen + (size_t)r * cmc::CC_TOPCHAIN};
            const uint32_t n_out = cmc::cc_replay(ops, log_n, top, max_best, g.gene_start, (int)listed);
            out.n_chains = n_out;
            out.n_stored = n_out < (uint32_t)cmc::CC_TOPCHAIN ? n_out : (uint32_t)cmc::CC_TOPCHAIN;
        }
        if (lane == 0) {
            if (refused) {
                out = CcRes{0, 0, 0, CM_CIRC_CHAIN_REFUSED};
                atomicAdd(&w.counters[2], 1ull);
            } else {
                out.listed = listed;
                atomicAdd(&w.counters[0], (unsigned long long)cells);
                atomicAdd(&w.counters[1], (unsigned long long)log_n);
            }
            w.res[r] = out;
        }
    }
}

struct Ev2 {
    hipEvent_t a = nullptr, b = nullptr;
    ~Ev2() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v ? (uint64_t)v : dflt;
}

}  // namespace

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail((e_ == hipErrorOutOfMemory) ? CM_ENOMEM : CM_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// annot: the slot's cmc::AnnotDev (device pointers), annot_bytes its sizeof in the caller's build.  d_contig / contig_len: the
// slot's resident sequence (device memory), used when genome == NULL.  wsp: the context's workspace (cm_circ_chain_ws.h): every
// device buffer of the call lives there and stays there; CM_CIRC_TRACE prints what the call allocated and what is held.
extern "C" int cm_circ_chain_run(hipStream_t so, cm_circ_chain_ws *wsp, const cm_params *P, const void *annot, size_t annot_bytes, const uint8_t *d_contig, uint32_t contig_len,
                                 int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs, uint64_t seqs_len,
                                 const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                                 uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                                 uint64_t *n_frags_out, uint64_t stats[8], char *err, size_t err_cap) {
    auto fail = [&](int code, const char *fmt, auto... a) {      // the message goes to the caller, who owns the context
        if (err && err_cap) snprintf(err, err_cap, fmt, a...);
        return code;
    };
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n_chains_out) *n_chains_out = 0;
    if (n_frags_out) *n_frags_out = 0;
    if (!P || !wsp || !annot || (n_req && (!req || !res || !seqs))) return fail(CM_EINVAL, "null argument");
    if (annot_bytes != sizeof(cmc::AnnotDev)) return fail(CM_EINVAL, "AnnotDev of %zu bytes, %zu here", annot_bytes, sizeof(cmc::AnnotDev));
    const int ws = window_size == 0 ? 8 : window_size;
    if (ws < 6 || ws > 10) return fail(CM_ELIMIT, "window size %d (6 .. 10)", ws);
    if (!genome) {
        if (!d_contig) return fail(CM_EINVAL, "genome == NULL and no contig is resident in the slot");
        ref_len = contig_len;
    }
    if (P->max_chain_len < 1 || P->max_chain_len > 4096) return fail(CM_EINVAL, "max_chain_len %d", P->max_chain_len);
    if (n_req > (1u << 24)) return fail(CM_EINVAL, "batch too large");
    for (uint32_t i = 0; i < n_req; ++i) {
        const cm_circ_chain_req &q = req[i];
        if (q.qs == 0 || q.qe > q.seq_len || q.seq_off > seqs_len || q.seq_len > seqs_len - q.seq_off || q.gene_end < q.gene_start)
            return fail(CM_EINVAL, "request %u: qs >= 1, qe <= seq_len, the mate inside the arena, gene_start <= gene_end", i);
    }
    if (n_req == 0) return CM_OK;
    if ((cap_chains && (!chain_score || !chain_len || !chain_frag_off)) || (cap_frags && (!rpos || !qpos))) return fail(CM_EINVAL, "null output array");

    // distinct genes in first-use order, their table sizes, the groups that fit the budget
    const uint32_t S = 1u << (2 * ws);
    const uint64_t budget = env_u64("CM_CIRC_TABLE_BYTES", TABLE_BYTES_DEFAULT);
    const uint32_t log_cap = (uint32_t)std::min<uint64_t>(env_u64("CM_CIRC_LOG_CAP", LOG_CAP_DEFAULT), 1u << 24);
    struct Gene { uint32_t start, end, len; uint64_t bytes; int group; uint32_t local; };
    std::vector<Gene> genes;
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> gene_ix;
    std::vector<uint32_t> gene_of(n_req);
    for (uint32_t i = 0; i < n_req; ++i) {
        const auto key = std::make_pair(req[i].gene_start, req[i].gene_end);
        auto it = gene_ix.find(key);
        if (it == gene_ix.end()) {
            const bool ok = key.first != 0 && (int32_t)key.first >= 0 && key.second <= ref_len;       // genome_at (pac2char_otf) takes it
            const uint32_t len = ok ? key.second - key.first + 1 : 0;
            const uint64_t bytes = 4ull * (2ull * S + 1 + cmc::cc_n_windows(len, ws));
            it = gene_ix.emplace(key, (uint32_t)genes.size()).first;
            genes.push_back(Gene{key.first, key.second, len, bytes, -1, 0});
        }
        gene_of[i] = it->second;
    }
    struct Group { std::vector<uint32_t> genes; uint64_t bytes = 0; };
    std::vector<Group> groups;
    for (uint32_t gi = 0; gi < genes.size(); ++gi) {
        Gene &g = genes[gi];
        if (g.bytes > budget) continue;                       // alone beyond the budget: its problems are refused
        if (groups.empty() || groups.back().bytes + g.bytes > budget || groups.back().genes.size() >= 65535) groups.emplace_back();
        g.group = (int)groups.size() - 1;
        g.local = (uint32_t)groups.back().genes.size();
        groups.back().genes.push_back(gi);
        groups.back().bytes += g.bytes;
    }

    // per-request fragment places on the device: CC_TOPCHAIN chains of at most `positions` fragments
    std::vector<uint64_t> frag_base(n_req + 1, 0);
    for (uint32_t i = 0; i < n_req; ++i)
        frag_base[i + 1] = frag_base[i] + (uint64_t)cmc::CC_TOPCHAIN * std::min<uint32_t>(cmc::cc_n_positions(req[i].qs, req[i].qe, ws), cmc::CC_MAX_LISTS);
    const uint64_t frag_cap = std::max<uint64_t>(frag_base[n_req], 1);

    cmc::KCore kc{};
    kc.P = *P;
    kc.A = *(const cmc::AnnotDev *)annot;

    // resident waves: as many as a quarter of the free device memory holds workspace slices for, 1024 at the most -- decided when
    // the slices are first sized, and again when CM_CIRC_LOG_CAP has changed the size of a slice
    const uint32_t seen_cap = (uint32_t)P->max_chain_len * cmc::CC_MAX_LISTS;
    const uint64_t slice_bytes = (uint64_t)CELL_CAP * (sizeof(double) + sizeof(int32_t)) + (uint64_t)log_cap * sizeof(cmc::CcEv) + (uint64_t)seen_cap * 4;
    const uint64_t allocs_before = wsp->allocations;
    if (wsp->max_workers == 0 || wsp->log_cap != log_cap || wsp->seen_cap != seen_cap) {
        for (int b : {CCW_SCORE, CCW_PREV, CCW_LOG, CCW_SEEN}) cc_ws_drop(*wsp, b);
        wsp->max_workers = 0;
        size_t mem_free = 0, mem_total = 0;
        HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
        if (slice_bytes > mem_free / 4)
            return fail(CM_ELIMIT, "CM_CIRC_LOG_CAP %u: one problem's workspace of %llu bytes against %llu free", log_cap, (unsigned long long)slice_bytes,
                        (unsigned long long)mem_free);
        wsp->max_workers = (uint32_t)std::min<uint64_t>(MAX_WORKERS, mem_free / 4 / slice_bytes);
        wsp->log_cap = log_cap;
        wsp->seen_cap = seen_cap;
    }
    const uint32_t workers = std::min<uint32_t>(n_req, wsp->max_workers);
    struct Dev { void *p; } d_req, d_seqs, d_geneof, d_fragbase, d_res, d_cscore, d_clen, d_rpos, d_qpos, d_cursor, d_counters, d_score, d_prev, d_log, d_seen;
#define WS_BUF(dst, which, need)                      \
    do {                                              \
        HIPCHK(cc_ws_ensure(*wsp, which, (need)));     \
        (dst).p = wsp->p[which];                       \
    } while (0)
    WS_BUF(d_req, CCW_REQ, (size_t)n_req * sizeof(cm_circ_chain_req));
    WS_BUF(d_seqs, CCW_SEQS, (size_t)std::max<uint64_t>(seqs_len, 1));
    WS_BUF(d_geneof, CCW_GENEOF, (size_t)n_req * 4);
    WS_BUF(d_fragbase, CCW_FRAGBASE, (size_t)n_req * 8);
    WS_BUF(d_res, CCW_RES, (size_t)n_req * sizeof(CcRes));
    WS_BUF(d_cscore, CCW_CSCORE, (size_t)n_req * cmc::CC_TOPCHAIN * 4);
    WS_BUF(d_clen, CCW_CLEN, (size_t)n_req * cmc::CC_TOPCHAIN * 4);
    WS_BUF(d_rpos, CCW_RPOS, (size_t)frag_cap * 4);
    WS_BUF(d_qpos, CCW_QPOS, (size_t)frag_cap * 4);
    WS_BUF(d_cursor, CCW_CURSOR, 4);
    WS_BUF(d_counters, CCW_COUNTERS, 8 * 8);
    WS_BUF(d_score, CCW_SCORE, (size_t)workers * CELL_CAP * sizeof(double));
    WS_BUF(d_prev, CCW_PREV, (size_t)workers * CELL_CAP * sizeof(int32_t));
    WS_BUF(d_log, CCW_LOG, (size_t)workers * log_cap * sizeof(cmc::CcEv));
    WS_BUF(d_seen, CCW_SEEN, (size_t)workers * seen_cap * 4);
    HIPCHK(hipMemcpyAsync(d_req.p, req, (size_t)n_req * sizeof(cm_circ_chain_req), hipMemcpyHostToDevice, so));
    if (seqs_len) HIPCHK(hipMemcpyAsync(d_seqs.p, seqs, (size_t)seqs_len, hipMemcpyHostToDevice, so));
    HIPCHK(hipMemcpyAsync(d_fragbase.p, frag_base.data(), (size_t)n_req * 8, hipMemcpyHostToDevice, so));
    HIPCHK(hipMemsetAsync(d_res.p, 0, (size_t)n_req * sizeof(CcRes), so));
    HIPCHK(hipMemsetAsync(d_cscore.p, 0, (size_t)n_req * cmc::CC_TOPCHAIN * 4, so));
    HIPCHK(hipMemsetAsync(d_clen.p, 0, (size_t)n_req * cmc::CC_TOPCHAIN * 4, so));
    HIPCHK(hipMemsetAsync(d_counters.p, 0, 8 * 8, so));

    // requests by group (a request of a gene beyond the budget has none and is refused here)
    std::vector<std::vector<uint32_t>> order(groups.size());
    std::vector<uint32_t> local_gene(n_req, 0);
    uint64_t refused_host = 0;
    std::vector<uint8_t> refused(n_req, 0);
    for (uint32_t i = 0; i < n_req; ++i) {
        const Gene &g = genes[gene_of[i]];
        if (g.group < 0) {
            refused[i] = 1;
            ++refused_host;
            continue;
        }
        order[(size_t)g.group].push_back(i);
        local_gene[i] = g.local;
    }
    HIPCHK(hipMemcpyAsync(d_geneof.p, local_gene.data(), (size_t)n_req * 4, hipMemcpyHostToDevice, so));

    Ev2 ev_t, ev_c;
    HIPCHK(hipEventCreate(&ev_t.a));
    HIPCHK(hipEventCreate(&ev_t.b));
    HIPCHK(hipEventCreate(&ev_c.a));
    HIPCHK(hipEventCreate(&ev_c.b));
    double ms_tab = 0, ms_chain = 0;
    uint64_t max_group_bytes = 0;
    for (size_t gr = 0; gr < groups.size(); ++gr) {
        const Group &G = groups[gr];
        max_group_bytes = std::max(max_group_bytes, G.bytes);
        // the sequence of the group's genes: merged spans of the host genome, or the resident contig as it is
        std::vector<CcGene> gd(G.genes.size());
        std::vector<uint8_t> arena;
        uint64_t loc_words = 0;
        uint32_t max_nw = 1;
        {
            std::vector<uint32_t> by_start(G.genes.begin(), G.genes.end());
            std::sort(by_start.begin(), by_start.end(), [&](uint32_t a, uint32_t b) { return genes[a].start < genes[b].start; });
            uint32_t span_s = 0, span_e = 0;          // current merged span [span_s, span_e], 1-based
            uint64_t span_at = 0;
            for (uint32_t gi : by_start) {
                const Gene &g = genes[gi];
                CcGene &d = gd[g.local];
                d = CcGene{0, g.len, g.start, 0, 0, 0};
                if (g.len == 0) continue;
                if (!genome) {
                    d.seq_off = (uint64_t)g.start - 1;
                    continue;
                }
                if (span_e == 0 || g.start > span_e) {       // a new span
                    span_s = g.start;
                    span_e = g.end;
                    span_at = arena.size();
                    arena.insert(arena.end(), genome + (g.start - 1), genome + g.end);
                } else if (g.end > span_e) {                 // extends the span
                    arena.insert(arena.end(), genome + span_e, genome + g.end);
                    span_e = g.end;
                }
                d.seq_off = span_at + (g.start - span_s);
            }
        }
        for (size_t k = 0; k < gd.size(); ++k) {
            const uint32_t nw = cmc::cc_n_windows(gd[k].len, ws);
            gd[k].off_base = (uint64_t)k * (S + 1);
            gd[k].cnt_base = (uint64_t)k * S;
            gd[k].loc_base = loc_words;
            loc_words += nw;
            max_nw = std::max(max_nw, nw);
        }
        Dev d_genes, d_arena, d_off, d_cnt, d_loc, d_order;
        CcTab t{};
        t.n_genes = (uint32_t)gd.size();
        t.ws = ws;
        t.n_buckets = S;
        t.off_words = (uint64_t)gd.size() * (S + 1);
        t.cnt_words = (uint64_t)gd.size() * S;
        t.loc_words = std::max<uint64_t>(loc_words, 1);
        WS_BUF(d_genes, CCW_GENES, gd.size() * sizeof(CcGene));
        WS_BUF(d_off, CCW_OFF, (size_t)t.off_words * 4);
        WS_BUF(d_cnt, CCW_CNT, (size_t)t.cnt_words * 4);
        WS_BUF(d_loc, CCW_LOC, (size_t)t.loc_words * 4);
        HIPCHK(hipMemcpyAsync(d_genes.p, gd.data(), gd.size() * sizeof(CcGene), hipMemcpyHostToDevice, so));
        if (genome) {
            WS_BUF(d_arena, CCW_ARENA, std::max<size_t>(arena.size(), 1));
            if (!arena.empty()) HIPCHK(hipMemcpyAsync(d_arena.p, arena.data(), arena.size(), hipMemcpyHostToDevice, so));
            t.seq = (const uint8_t *)d_arena.p;
            t.seq_len = arena.size();
        } else {
            t.seq = d_contig;
            t.seq_len = contig_len;
        }
        t.genes = (const CcGene *)d_genes.p;
        t.off = (uint32_t *)d_off.p;
        t.cnt = (uint32_t *)d_cnt.p;
        t.loc = (uint32_t *)d_loc.p;
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, (size_t)t.cnt_words * 4, so));
        HIPCHK(hipMemsetAsync(d_loc.p, 0, (size_t)t.loc_words * 4, so));
        HIPCHK(hipEventRecord(ev_t.a, so));
        const dim3 by_pos(std::min<uint32_t>((max_nw + BLK_TAB - 1) / BLK_TAB, 1024), t.n_genes);
        hipLaunchKernelGGL(k_cc_tab_count, by_pos, dim3(BLK_TAB), 0, so, t);
        hipLaunchKernelGGL(k_cc_tab_scan, dim3(t.n_genes), dim3(BLK_TAB), 0, so, t);
        hipLaunchKernelGGL(k_cc_tab_place, by_pos, dim3(BLK_TAB), 0, so, t);
        hipLaunchKernelGGL(k_cc_tab_order, dim3(S / 64, t.n_genes), dim3(64), 0, so, t);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev_t.b, so));

        const std::vector<uint32_t> &ord = order[gr];
        if (!ord.empty()) {
            WS_BUF(d_order, CCW_ORDER, ord.size() * 4);
            HIPCHK(hipMemcpyAsync(d_order.p, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, so));
            HIPCHK(hipMemsetAsync(d_cursor.p, 0, 4, so));
            CcWork w{};
            w.req = (const cm_circ_chain_req *)d_req.p;
            w.order = (const uint32_t *)d_order.p;
            w.n_order = (uint32_t)ord.size();
            w.n_req = n_req;
            w.n_genes = t.n_genes;
            w.seqs_len = seqs_len;
            w.off_words = t.off_words;
            w.loc_words = t.loc_words;
            w.gene_of = (const uint32_t *)d_geneof.p;
            w.genes = t.genes;
            w.tab_off = t.off;
            w.tab_loc = t.loc;
            w.seqs = (const uint8_t *)d_seqs.p;
            w.ws = ws;
            w.cell_score = (double *)d_score.p;
            w.cell_prev = (int32_t *)d_prev.p;
            w.log = (cmc::CcEv *)d_log.p;
            w.seen = (uint32_t *)d_seen.p;
            w.cell_cap = CELL_CAP;
            w.log_cap = log_cap;
            w.seen_cap = seen_cap;
            w.res = (CcRes *)d_res.p;
            w.cscore = (float *)d_cscore.p;
            w.clen = (uint32_t *)d_clen.p;
            w.frag_base = (const uint64_t *)d_fragbase.p;
            w.rpos = (uint32_t *)d_rpos.p;
            w.qpos = (int32_t *)d_qpos.p;
            w.frag_cap = frag_cap;
            w.cursor = (unsigned int *)d_cursor.p;
            w.counters = (unsigned long long *)d_counters.p;
            HIPCHK(hipEventRecord(ev_c.a, so));
            hipLaunchKernelGGL(k_cc_chain, dim3(std::min<uint32_t>(w.n_order, workers)), dim3(64), 0, so, kc, w);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ev_c.b, so));
        }
        HIPCHK(hipStreamSynchronize(so));            // the next group takes the group's buffers
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_t.a, ev_t.b) == hipSuccess) ms_tab += ms;
        if (!ord.empty() && hipEventElapsedTime(&ms, ev_c.a, ev_c.b) == hipSuccess) ms_chain += ms;
    }

    // results back, packed into running offsets in request order
    std::vector<CcRes> h_res(n_req);
    std::vector<float> h_score((size_t)n_req * cmc::CC_TOPCHAIN);
    std::vector<uint32_t> h_len((size_t)n_req * cmc::CC_TOPCHAIN), h_rpos((size_t)frag_cap);
    std::vector<int32_t> h_qpos((size_t)frag_cap);
    unsigned long long h_cnt[8];
    HIPCHK(hipMemcpyAsync(h_res.data(), d_res.p, (size_t)n_req * sizeof(CcRes), hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(h_score.data(), d_cscore.p, h_score.size() * 4, hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(h_len.data(), d_clen.p, h_len.size() * 4, hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(h_rpos.data(), d_rpos.p, (size_t)frag_cap * 4, hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(h_qpos.data(), d_qpos.p, (size_t)frag_cap * 4, hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(h_cnt, d_counters.p, sizeof h_cnt, hipMemcpyDeviceToHost, so));
    HIPCHK(hipStreamSynchronize(so));
    uint64_t need_chains = 0, need_frags = 0;
    for (uint32_t i = 0; i < n_req; ++i) {
        if (refused[i]) h_res[i] = CcRes{0, 0, 0, CM_CIRC_CHAIN_REFUSED};
        const CcRes &v = h_res[i];
        const uint32_t npos = std::min<uint32_t>(cmc::cc_n_positions(req[i].qs, req[i].qe, ws), cmc::CC_MAX_LISTS);
        if (v.n_stored > (uint32_t)cmc::CC_TOPCHAIN) return fail(CM_EHIP, "request %u: %u stored chains", i, v.n_stored);
        need_chains += v.n_stored;
        for (uint32_t k = 0; k < v.n_stored; ++k) {
            if (h_len[(size_t)i * cmc::CC_TOPCHAIN + k] > npos) return fail(CM_EHIP, "request %u: a chain of %u fragments", i, h_len[(size_t)i * cmc::CC_TOPCHAIN + k]);
            need_frags += h_len[(size_t)i * cmc::CC_TOPCHAIN + k];
        }
    }
    if (getenv("CM_CIRC_TRACE"))
        fprintf(stderr, "[circ] workspace: %llu allocations, %llu held\n", (unsigned long long)(wsp->allocations - allocs_before), (unsigned long long)wsp->held);
    if (n_chains_out) *n_chains_out = need_chains;
    if (n_frags_out) *n_frags_out = need_frags;
    if (stats) {
        stats[0] = genes.size();
        stats[1] = max_group_bytes;
        stats[2] = groups.size();
        stats[3] = h_cnt[0];
        stats[4] = h_cnt[1];
        stats[5] = h_cnt[2] + refused_host;
        stats[6] = (uint64_t)(ms_tab * 1000.0);          // microseconds, as integers travel in this array
        stats[7] = (uint64_t)(ms_chain * 1000.0);
    }
    if (need_chains > cap_chains || need_frags > cap_frags)
        return fail(CM_ELIMIT, "%llu chains / %llu fragments, room for %llu / %llu", (unsigned long long)need_chains, (unsigned long long)need_frags,
                    (unsigned long long)cap_chains, (unsigned long long)cap_frags);
    uint64_t c_at = 0, f_at = 0;
    for (uint32_t i = 0; i < n_req; ++i) {
        const CcRes &v = h_res[i];
        const uint32_t npos = std::min<uint32_t>(cmc::cc_n_positions(req[i].qs, req[i].qe, ws), cmc::CC_MAX_LISTS);
        res[i] = cm_circ_chain_res{v.n_chains, v.n_stored, v.listed, v.flags, c_at};
        for (uint32_t k = 0; k < v.n_stored; ++k) {
            const uint32_t len = h_len[(size_t)i * cmc::CC_TOPCHAIN + k];
            chain_score[c_at] = h_score[(size_t)i * cmc::CC_TOPCHAIN + k];
            chain_len[c_at] = len;
            chain_frag_off[c_at] = f_at;
            const uint64_t from = frag_base[i] + (uint64_t)k * npos;
            for (uint32_t f = 0; f < len; ++f) {
                rpos[f_at + f] = h_rpos[from + f];
                qpos[f_at + f] = h_qpos[from + f];
            }
            f_at += len;
            ++c_at;
        }
    }
    return CM_OK;
}
#undef WS_BUF
