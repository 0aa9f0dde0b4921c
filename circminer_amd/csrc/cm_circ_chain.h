// cm_circ_chain.h — the bodies of stage 2's seeding and k-best chaining (ProcessCirc::chaining, reference src/process_circ.cpp:677-737;
// chain_seeds_sorted_kbest2, src/chain.cpp:310-539; RegionalHashTable::create_table, src/hash_table.cpp:58-112), written once for
// hipcc and g++ like cm_index_build.h and cm_remain_order.h: the kernels of cm_circ_chain.hip and the emulation of
// tests/hostemu_circ_chain.cpp call the same functions, so what the emulation shows against Caller::chains_of (host_circ_call.cpp,
// the serial statement) holds for the device code up to the orchestration around them.
//
// Include after cm_core.h: upper_bound / check_junction / Core are the includer's build of the kernel bodies (namespace cmc).
//
// How one problem (gene, oriented mate, [qs, qe]) is split up
//   plan     one seed every CC_STEP bases; a seed with an invalid code is not listed, one with more than seed_lim hits is listed with
//            n = 0, trailing n == 0 lists are trimmed for the DP (kc lists) but count in `listed`
//   DP       lists from kc - 2 down to 0, cells of a list in ascending order.  The candidates of one cell come from the later lists
//            b = a + 1 .. kc - 1 in that order; the LATER LISTS are what runs in parallel (one lane per later list).  That keeps the
//            carried cursor of a later list (the reference advances it from cell to cell and tests max_intron against the hit under
//            it, not against the first hit beyond the cell) in the lane that owns the list: no pre-pass, no cursor array.
//            Per cell: pass 1 = best candidate score of each later list (cc_cell_list with a floor of -inf), an exclusive prefix
//            maximum over the lists in list order gives each list the running score it would have met serially; pass 2 counts the
//            strict improvements above that floor, an exclusive prefix sum gives their places in the log; pass 3 stores them.
//            The log so gets the reference's insertion order: list descending, cell ascending, (later list, hit) ascending.
//   replay   (cc_replay, one body for both) stable order by score descending = repeated "next entry after (score, order)" (cc_better); at most max_chain_len
//            entries of one score count, the `repeats` filter applies below the top score only; nothing chained: single seeds,
//            last list first; the list is cut at the first chain whose count of unused seeds rises (cc_cut_keeps)
#pragma once
#include <stdint.h>

namespace cmc {

constexpr int CC_STEP = 3;                 // one seed every 3 bases (src/process_circ.cpp:59)
constexpr uint32_t CC_MAXHIT = 1000;       // a bucket with more hits is emptied (src/hash_table.h MAXHIT)
constexpr int CC_TOPCHAIN = 10;            // chains a consumer reads per gene and read (src/process_circ.cpp:19)
constexpr int CC_MAX_LISTS = 128;          // seed positions of one problem the parallel form takes (2 per lane); more: refused
constexpr double CC_NEG = -1e300;          // floor below every score

// ---- seed code (RegionalHashTable::hash_val): upper and lower case, -1 for any other byte
template <class P8> CM_HD inline int cc_code(P8 s, int ws) {
    int v = 0;
    for (int i = 0; i < ws; ++i) {
        int b;
        switch (s[i]) {
            case 'A': case 'a': b = 0; break;
            case 'C': case 'c': b = 1; break;
            case 'G': case 'g': b = 2; break;
            case 'T': case 't': b = 3; break;
            default: return -1;
        }
        v = v * 4 + b;
    }
    return v;
}

// ---- regional table: per-position and per-bucket bodies
// windows of a gene of `len` bases
CM_HD inline uint32_t cc_n_windows(uint32_t len, int ws) { return len >= (uint32_t)ws ? len - (uint32_t)ws + 1 : 0; }
// count pass / place pass of position i: its bucket, or -1
template <class P8> CM_HD inline int cc_tab_bucket(P8 gene, uint32_t i, int ws) { return cc_code(gene + i, ws); }
// scan pass of one bucket: what it contributes to the offsets (an over-full bucket is emptied)
CM_HD inline uint32_t cc_tab_kept(uint32_t count) { return count <= CC_MAXHIT ? count : 0; }
// order pass: the place of value v among the n distinct values of its bucket
template <class P32> CM_HD inline uint32_t cc_tab_rank(P32 vals, uint32_t n, uint32_t v) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; ++k) r += vals[k] < v ? 1u : 0u;
    return r;
}

// ---- plan of a problem
// seed positions: i = qs - 1 + CC_STEP * p with i + ws <= qe; 0 when the span is shorter than a window
CM_HD inline uint32_t cc_n_positions(uint32_t qs, uint32_t qe, int ws) {
    if (qs == 0 || qe < qs || (int)(qe - qs + 1) < ws) return 0;
    return (qe - qs + 1 - (uint32_t)ws) / CC_STEP + 1;
}
struct CcSeed { uint32_t first, n; int32_t qpos; bool listed; };      // first: offset of its bucket in the table's loc
// seed at position p of the plan
template <class P8, class P32> CM_HD inline CcSeed cc_plan_seed(P8 seq, uint32_t qs, uint32_t p, int ws, P32 tab_off, int32_t seed_lim) {
    CcSeed s{0, 0, (int32_t)(qs - 1 + (uint32_t)CC_STEP * p), false};
    const int hv = cc_code(seq + s.qpos, ws);
    if (hv < 0) return s;
    s.listed = true;
    s.first = tab_off[hv];
    s.n = tab_off[hv + 1] - tab_off[hv];
    if (s.n > (uint32_t)seed_lim) s.n = 0;
    return s;
}

// ---- DP
// The carried cursor of one later list at one cell (here = the cell's hit): advances `cur` as the reference does and says whether
// the list takes part in this cell.
template <class P32> CM_HD inline bool cc_cursor_step(int32_t here, int32_t max_intron, P32 hit, uint32_t n, uint32_t &cur) {
    if (n == 0 || cur >= n) return false;
    if (here + max_intron < (int32_t)hit[cur]) return false;
    while (cur < n && (int32_t)hit[cur] <= here) ++cur;
    return cur < n;
}
// what a cell knows once some later list takes part (upper_bound on the bare gene offset, as the reference)
struct CcCell { uint32_t seg_start, seg_end, limit, max_exon_end; int ol; };
CM_HD inline CcCell cc_cell_bounds(const Core &c, int32_t here, int kmer, int seq_len, int32_t qpos) {
    CcCell x;
    x.seg_start = (uint32_t)here;
    x.seg_end = x.seg_start + (uint32_t)kmer - 1;
    x.max_exon_end = 0;
    x.ol = -1;
    x.limit = upper_bound(c, x.seg_start, (uint32_t)kmer, (uint32_t)(seq_len - qpos - kmer), x.max_exon_end, x.ol);
    return x;
}
// One DP cell against one later list, from the list's cursor on: every candidate whose score is strictly above `running` raises
// it and is handed to rec(score, j).  Pass 1 runs it with running = CC_NEG and no-op rec (the result is the list's best), the
// count pass and the store pass with the floor the prefix maximum gives.  fp64, no contraction: dp + 2e4 * kmer - 0.1 * (hi - lo).
template <class P32, class PD, class F>
CM_HD inline double cc_cell_list(const Core &c, const CcCell &x, int kmer, int read_dist, P32 hit, uint32_t n, uint32_t cur, PD dp_score, double running, F rec) {
    for (uint32_t j = cur; j < n && hit[j] <= x.limit; ++j) {
        const uint32_t there = hit[j];
        int gdist = INF_I, tdist, dist;
        if (x.max_exon_end == 0 || there + (uint32_t)kmer - 1 <= x.max_exon_end) gdist = (int)(there - x.seg_end - 1);
        if (cabs(gdist - read_dist) <= c.P.max_ed) dist = gdist;
        else if (check_junction(c, x.seg_start, there, x.ol, kmer, read_dist, tdist)) dist = tdist;
        else continue;
        const int hi = cmax(read_dist, dist), lo = cmin(read_dist, dist);
        const double sc = dp_score[j] + 2e4 * kmer - 0.1 * (hi - lo);
        if (sc > running) {
            running = sc;
            rec(sc, j);
        }
    }
    return running;
}

// ---- replay
struct CcEv { double score; uint32_t list, ind; };      // one improvement; its order is its index in the log
// (s, o) comes before (s2, o2) in the replay: score descending, insertion order inside a score
CM_HD inline bool cc_before(double s, uint32_t o, double s2, uint32_t o2) { return s > s2 || (s == s2 && o < o2); }
// is log entry (s, o) a candidate for "the next one after (after_s, after_o)", and better than the best found so far?
CM_HD inline bool cc_better(double s, uint32_t o, double after_s, uint32_t after_o, bool any_after, bool have, double best_s, uint32_t best_o) {
    if (any_after && !cc_before(after_s, after_o, s, o)) return false;
    return !have || cc_before(s, o, best_s, best_o);
}
// the `repeats` filter: below the top score an entry is dropped when the BARE offset of its first hit equals a shifted position
// some earlier chain used for a non-first fragment (the reference compares exactly these two)
CM_HD inline bool cc_repeat_applies(double score, double top) { return score < top; }
// the cut by unused seeds: chain of `len` fragments after chains whose least count of unused seeds was `least`
CM_HD inline bool cc_cut_keeps(int listed, uint32_t len, int &least) {
    const int missing = listed - (int)len;
    if (missing > least) return false;
    least = missing;
    return true;
}
// back pointer of a cell: (list << 16 | ind), -1 = none
CM_HD inline int32_t cc_prev_pack(uint32_t list, uint32_t ind) { return (int32_t)((list << 16) | ind); }

// The replay of one problem, written once: the kernel and the emulation hand in how a wave (or a loop) does the four things that
// are not the same code for them.  Ops:
//   bool     next(double after_s, uint32_t after_o, bool any_after, double &s, uint32_t &o)   the log entry that follows (after_s,
//                                                          after_o) in the order of cc_before (cc_better over the whole log)
//   CcEv     event(uint32_t o)                             log entry o
//   uint32_t lists(), hits(list)                           kc and a list's n
//   uint32_t hit(list, ind), int32_t qpos(list), int32_t prev(list, ind), double cell(list, ind)
//   bool     seen_has(uint32_t v); void seen_push(uint32_t v); void seen_sync()     the `repeats` list (sync: pushes become visible)
//   void     frag(uint32_t chain, uint32_t at, uint32_t rpos, int32_t qpos)         fragment `at` of kept chain `chain`
//   void     chain(uint32_t chain, float score, uint32_t len)                       (both called for every chain; the receiver keeps CC_TOPCHAIN)
// Returns the number of chains kept.  log_n == 0: nothing chained, single seeds, last list first.
template <class Ops> CM_HD inline uint32_t cc_replay(Ops &o, uint32_t log_n, double top, uint32_t max_best, uint32_t gene_start, int listed) {
    uint32_t n_out = 0;
    int least = INF_I;
    const uint32_t kc = o.lists();
    if (log_n == 0) {
        for (int a = (int)kc - 1; a >= 0 && n_out < max_best; --a)
            for (uint32_t i = 0; i < o.hits((uint32_t)a) && n_out < max_best; ++i) {
                if (!cc_cut_keeps(listed, 1, least)) return n_out;
                o.frag(n_out, 0, gene_start + o.hit((uint32_t)a, i), o.qpos((uint32_t)a));
                o.chain(n_out, (float)o.cell((uint32_t)a, i), 1);
                ++n_out;
            }
        return n_out;
    }
    bool any_after = false;
    double after_s = 0, run_s = 0;
    uint32_t after_o = 0, run_n = 0;
    while (n_out < max_best) {
        double bs = 0;
        uint32_t bo = 0;
        if (!o.next(after_s, after_o, any_after, bs, bo)) break;
        if (any_after && bs == run_s) ++run_n;
        else {
            run_s = bs;
            run_n = 0;
        }
        any_after = true;
        after_s = bs;
        after_o = bo;
        if (run_n >= max_best) {           // only the first max_best entries of a score count: on to the next score
            after_o = 0xFFFFFFFFu;
            continue;
        }
        const CcEv ev = o.event(bo);
        if (ev.list >= kc || ev.ind >= o.hits(ev.list)) break;          // (cannot happen: the log holds cells of this problem)
        if (cc_repeat_applies(bs, top) && o.seen_has(o.hit(ev.list, ev.ind))) continue;
        // walk the chain along the cells' final back pointers
        uint32_t len = 0, l = ev.list, i = ev.ind;
        for (;;) {
            const uint32_t rp = gene_start + o.hit(l, i);
            o.frag(n_out, len, rp, o.qpos(l));
            if (len >= 1) o.seen_push(rp);
            ++len;
            const int32_t pv = o.prev(l, i);
            if (pv < 0 || len >= kc) break;
            l = (uint32_t)pv >> 16;
            i = (uint32_t)pv & 0xFFFFu;
            if (l >= kc || i >= o.hits(l)) break;                       // (cannot happen)
        }
        o.seen_sync();
        if (!cc_cut_keeps(listed, len, least)) break;
        o.chain(n_out, (float)bs, len);
        ++n_out;
    }
    return n_out;
}

}  // namespace cmc
