// Host emulation of cm_circ_chain.hip — test infrastructure only.  The bodies of circminer_amd/csrc/cm_circ_chain.h under g++,
// in the kernels' shapes: tables by count / scan / place / order with the positions placed in shuffled order; one problem = one
// "wave" of 64 lanes that own two later lists each, every phase between two wave collectives run over the lanes in shuffled
// order, the problems themselves in shuffled order.  What comes out is compared with cm_circ_chain_host (Caller::chains_of) byte
// for byte (tests/test_circ_chain_cpu.py), so a dependence on lane, cell or problem order shows here, without a device.
//
//   g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -I include -I circminer_amd/csrc tests/hostemu_circ_chain.cpp -o libccemu.so
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_core.h"
#include "cm_aos.h"
#include "cm_circ_chain.h"

namespace {

constexpr int W = 64;

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    std::vector<uint32_t> perm(uint32_t n) {
        std::vector<uint32_t> p(n);
        std::iota(p.begin(), p.end(), 0u);
        std::shuffle(p.begin(), p.end(), g);
        return p;
    }
};

// the four table passes for one gene (len 0: no window)
void table_build(const uint8_t *gene, uint32_t len, int ws, Rng &rng, std::vector<uint32_t> &off, std::vector<uint32_t> &loc) {
    const uint32_t S = 1u << (2 * ws), nw = cmc::cc_n_windows(len, ws);
    std::vector<uint32_t> cnt(S, 0);
    const std::vector<uint32_t> order = rng.perm(nw);
    for (uint32_t i : order) {                                   // count
        const int hv = cmc::cc_tab_bucket(gene, i, ws);
        if (hv >= 0) ++cnt[hv];
    }
    off.assign(S + 1, 0);
    uint32_t run = 0;
    for (uint32_t h = 0; h < S; ++h) {                           // scan; the count word becomes the place counter
        const uint32_t n = cnt[h], kept = cmc::cc_tab_kept(n);
        off[h] = run;
        run += kept;
        cnt[h] = (n > 0 && kept == 0) ? 0xFFFFFFFFu : 0u;
    }
    off[S] = run;
    loc.assign(std::max<uint32_t>(nw, 1), 0);
    for (uint32_t i : order) {                                   // place
        const int hv = cmc::cc_tab_bucket(gene, i, ws);
        if (hv < 0 || cnt[hv] == 0xFFFFFFFFu) continue;
        const uint32_t place = cnt[hv]++;
        if (place < off[hv + 1] - off[hv]) loc[off[hv] + place] = i;
    }
    std::vector<uint32_t> vals;
    for (uint32_t h = 0; h < S; ++h) {                           // order
        const uint32_t n = off[h + 1] - off[h];
        if (n <= 1) continue;
        vals.assign(loc.begin() + off[h], loc.begin() + off[h] + n);
        for (uint32_t k : rng.perm(n)) loc[off[h] + cmc::cc_tab_rank(vals.data(), n, vals[k])] = vals[k];
    }
}

struct Out {
    uint32_t n_chains = 0, listed = 0, flags = 0;
    std::vector<float> score;
    std::vector<std::vector<uint32_t>> r;
    std::vector<std::vector<int32_t>> q;
    uint64_t cells = 0, log = 0;
};

// one problem as k_cc_chain runs it
void problem(const cmc::Core &c, int ws, const cm_circ_chain_req &rq, const uint8_t *seqs, const uint32_t *toff, const uint32_t *tloc, uint32_t log_cap,
             uint32_t cell_cap, Rng &rng, Out &out) {
    out = Out{};
    const int kmer = ws;
    const uint32_t max_best = (uint32_t)c.P.max_chain_len;
    const uint32_t npos = cmc::cc_n_positions(rq.qs, rq.qe, ws);
    if (npos > (uint32_t)cmc::CC_MAX_LISTS) {
        out.flags = CM_CIRC_CHAIN_REFUSED;
        return;
    }
    if (npos == 0) return;
    const uint8_t *seq = seqs + rq.seq_off;
    // plan: positions in shuffled order, packed by the ballot's rule (a valid seed's place = valid seeds before it)
    std::vector<cmc::CcSeed> at_pos(npos);
    for (uint32_t p : rng.perm(npos)) at_pos[p] = cmc::cc_plan_seed(seq, rq.qs, p, ws, toff, c.P.seed_lim);
    std::vector<uint32_t> s_first, s_n, s_cell0;
    std::vector<int32_t> s_q;
    for (uint32_t p = 0; p < npos; ++p)
        if (at_pos[p].listed) {
            s_first.push_back(at_pos[p].first);
            s_n.push_back(at_pos[p].n);
            s_q.push_back(at_pos[p].qpos);
        }
    const uint32_t listed = (uint32_t)s_first.size();
    uint32_t kc = listed, cells = 0;
    while (kc >= 1 && s_n[kc - 1] == 0) --kc;
    s_cell0.assign(kc, 0);
    for (uint32_t a = 0; a < kc; ++a) {
        s_cell0[a] = cells;
        cells += s_n[a];
    }
    if (cells > cell_cap) {
        out.flags = CM_CIRC_CHAIN_REFUSED;
        return;
    }
    out.listed = listed;
    if (kc == 0) return;
    std::vector<double> score(cells, (double)kmer);
    std::vector<int32_t> prev(cells, -1);
    std::vector<cmc::CcEv> log;
    auto nothing = [](double, uint32_t) {};
    for (int a = (int)kc - 2; a >= 0; --a) {
        const uint32_t na = s_n[a];
        if (na == 0) continue;
        const uint32_t *hita = tloc + s_first[a];
        const int32_t qa = s_q[a];
        uint32_t cur[2][W] = {};
        for (uint32_t i = 0; i < na; ++i) {
            const int32_t here = (int32_t)hita[i];
            bool act[2][W] = {};
            bool any = false;
            struct LaneList { uint32_t b, nb; const uint32_t *hit; const double *sc; int rd; };
            auto list_of = [&](int half, int lane) {
                const uint32_t b = (uint32_t)a + 1 + (uint32_t)lane + 64u * (uint32_t)half;
                const bool in = b < kc;
                return LaneList{b, in ? s_n[b] : 0, tloc + (in ? s_first[b] : 0), score.data() + (in ? s_cell0[b] : 0), in ? s_q[b] - qa - kmer : 0};
            };
            for (uint32_t lane : rng.perm(W))
                for (int half = 0; half < 2; ++half) {
                    const LaneList L = list_of(half, (int)lane);
                    act[half][lane] = cmc::cc_cursor_step(here, c.P.max_intron, L.hit, L.nb, cur[half][lane]);
                    any |= act[half][lane];
                }
            if (!any) continue;
            const cmc::CcCell x = cmc::cc_cell_bounds(c, here, kmer, (int)rq.qe, qa);
            double m[2][W];
            for (uint32_t lane : rng.perm(W))                      // pass 1
                for (int half = 0; half < 2; ++half) {
                    const LaneList L = list_of(half, (int)lane);
                    m[half][lane] = act[half][lane] ? cmc::cc_cell_list(c, x, kmer, L.rd, L.hit, L.nb, cur[half][lane], L.sc, cmc::CC_NEG, nothing) : cmc::CC_NEG;
                }
            const double init = (double)kmer;
            double floor_[2][W], run = cmc::CC_NEG;                // exclusive prefix maximum in list order: half 0's lanes, then half 1's
            for (int half = 0; half < 2; ++half)
                for (int lane = 0; lane < W; ++lane) {
                    floor_[half][lane] = std::max(init, run);
                    run = std::max(run, m[half][lane]);
                }
            if (!(run > init)) continue;
            uint32_t n[2][W] = {}, lastj[2][W] = {};
            double end[2][W];
            for (uint32_t lane : rng.perm(W))                      // pass 2
                for (int half = 0; half < 2; ++half) {
                    const LaneList L = list_of(half, (int)lane);
                    end[half][lane] = floor_[half][lane];
                    if (act[half][lane] && m[half][lane] > floor_[half][lane])
                        end[half][lane] = cmc::cc_cell_list(c, x, kmer, L.rd, L.hit, L.nb, cur[half][lane], L.sc, floor_[half][lane], [&](double, uint32_t j) {
                            ++n[half][lane];
                            lastj[half][lane] = j;
                        });
                }
            uint32_t place[2][W], tot = 0;
            for (int half = 0; half < 2; ++half)
                for (int lane = 0; lane < W; ++lane) {
                    place[half][lane] = (uint32_t)log.size() + tot;
                    tot += n[half][lane];
                }
            if (log.size() + tot > log_cap) {
                out = Out{};
                out.flags = CM_CIRC_CHAIN_REFUSED;
                return;
            }
            const uint32_t base = (uint32_t)log.size();
            log.resize(base + tot);
            for (uint32_t lane : rng.perm(W))                      // pass 3
                for (int half = 0; half < 2; ++half) {
                    if (!n[half][lane]) continue;
                    const LaneList L = list_of(half, (int)lane);
                    uint32_t at = place[half][lane];
                    cmc::cc_cell_list(c, x, kmer, L.rd, L.hit, L.nb, cur[half][lane], L.sc, floor_[half][lane], [&](double sc, uint32_t) {
                        log[at++] = cmc::CcEv{sc, (uint32_t)a, i};
                    });
                }
            for (int half = 1; half >= 0; --half) {                // the cell keeps its last improvement
                int owner = -1;
                for (int lane = 0; lane < W; ++lane)
                    if (n[half][lane]) owner = lane;
                if (owner < 0) continue;
                score[s_cell0[a] + i] = end[half][owner];
                prev[s_cell0[a] + i] = cmc::cc_prev_pack(list_of(half, owner).b, lastj[half][owner]);
                break;
            }
        }
    }
    out.cells = cells;
    out.log = log.size();
    // replay: cc_replay with a loop where the kernel has a wave (the log walked in shuffled order)
    struct LoopReplay {
        Rng &rng;
        uint32_t kc;
        const std::vector<uint32_t> &s_first, &s_n, &s_cell0;
        const std::vector<int32_t> &s_q;
        const uint32_t *tloc;
        const std::vector<double> &score;
        const std::vector<int32_t> &prev_;
        const std::vector<cmc::CcEv> &log;
        Out &out;
        std::vector<uint32_t> seen;
        bool next(double after_s, uint32_t after_o, bool any_after, double &bs, uint32_t &bo) {
            bool have = false;
            for (uint32_t e : rng.perm((uint32_t)log.size()))
                if (cmc::cc_better(log[e].score, e, after_s, after_o, any_after, have, bs, bo)) {
                    have = true;
                    bs = log[e].score;
                    bo = e;
                }
            return have;
        }
        cmc::CcEv event(uint32_t o) const { return log[o]; }
        uint32_t lists() const { return kc; }
        uint32_t hits(uint32_t l) const { return s_n[l]; }
        uint32_t hit(uint32_t l, uint32_t i) const { return tloc[s_first[l] + i]; }
        int32_t qpos(uint32_t l) const { return s_q[l]; }
        int32_t prev(uint32_t l, uint32_t i) const { return prev_[s_cell0[l] + i]; }
        double cell(uint32_t l, uint32_t i) const { return score[s_cell0[l] + i]; }
        bool seen_has(uint32_t v) const { return std::find(seen.begin(), seen.end(), v) != seen.end(); }
        void seen_push(uint32_t v) { seen.push_back(v); }
        void seen_sync() const {}
        void frag(uint32_t chain, uint32_t at, uint32_t rp, int32_t qp) {
            if (chain >= (uint32_t)cmc::CC_TOPCHAIN) return;
            if (out.r.size() <= chain) {
                out.r.resize(chain + 1);
                out.q.resize(chain + 1);
            }
            out.r[chain].resize(at + 1);          // (a chain the cut drops leaves its fragments here: trimmed below)
            out.q[chain].resize(at + 1);
            out.r[chain][at] = rp;
            out.q[chain][at] = qp;
        }
        void chain(uint32_t chain, float sc, uint32_t len) {
            if (chain >= (uint32_t)cmc::CC_TOPCHAIN) return;
            out.score.push_back(sc);
            out.r[chain].resize(len);
            out.q[chain].resize(len);
        }
    } ops{rng, kc, s_first, s_n, s_cell0, s_q, tloc, score, prev, log, out, {}};
    double top = cmc::CC_NEG;
    for (const auto &e : log) top = std::max(top, e.score);
    const uint32_t n_out = cmc::cc_replay(ops, (uint32_t)log.size(), top, max_best, rq.gene_start, (int)listed);
    out.r.resize(out.score.size());
    out.q.resize(out.score.size());
    out.n_chains = n_out;
}

}  // namespace

extern "C" {

// the emulated table of one gene: off (4^ws + 1 words) and loc (max(len - ws + 1, 1) words), the caller's arrays
int cm_cc_emu_table(const uint8_t *gene, uint32_t len, int32_t ws, uint64_t seed, uint32_t *off, uint32_t *loc) {
    if (ws < 6 || ws > 10 || (len && !gene) || !off || !loc) return CM_EINVAL;
    Rng rng(seed);
    std::vector<uint32_t> o, l;
    table_build(gene, len, ws, rng, o, l);
    std::copy(o.begin(), o.end(), off);
    std::copy(l.begin(), l.begin() + std::max<uint32_t>(cmc::cc_n_windows(len, ws), 1), loc);
    return CM_OK;
}

// cm_circ_chain_host's arguments and layout; log_cap / cell_cap 0 = no bound; log_len (may be NULL): every problem's log length
// (0 for a refused one).  stats as cm_circ_chain_batch: [0] genes, [3] cells, [4] log events, [5] refused.
int cm_cc_emu(const cm_params *P, const cm_annot_view *av, int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs, uint64_t seqs_len,
              const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len, uint64_t *chain_frag_off,
              uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out, uint64_t *n_frags_out, uint64_t stats[8],
              uint32_t log_cap, uint32_t cell_cap, uint64_t seed, uint32_t *log_len) {
    if (!P || !av || !genome || (n_req && (!req || !res || !seqs))) return CM_EINVAL;
    const int ws = window_size == 0 ? 8 : window_size;
    if (ws < 6 || ws > 10) return CM_ELIMIT;
    for (uint32_t i = 0; i < n_req; ++i) {
        const cm_circ_chain_req &q = req[i];
        if (q.qs == 0 || q.qe > q.seq_len || q.seq_off > seqs_len || q.seq_len > seqs_len - q.seq_off || q.gene_end < q.gene_start) return CM_EINVAL;
    }
    cmc::AnnotAosHost aos;
    cmc::build_annot_aos(*av, aos);
    cmc::KCore kc;
    kc.P = *P;
    kc.X = cm_index_view{};
    kc.A = cmc::annot_dev_host(*av, aos);
    const cmc::Core c = cmc::to_core(kc);
    Rng rng(seed);
    struct Tab { std::vector<uint32_t> off, loc; };
    std::map<uint64_t, Tab> tabs;
    for (uint32_t i = 0; i < n_req; ++i) {
        const uint64_t key = (uint64_t)req[i].gene_start << 32 | req[i].gene_end;
        if (tabs.count(key)) continue;
        const uint32_t gs = req[i].gene_start, ge = req[i].gene_end;
        const bool ok = gs != 0 && (int32_t)gs >= 0 && ge <= ref_len;
        table_build(ok ? genome + (gs - 1) : nullptr, ok ? ge - gs + 1 : 0, ws, rng, tabs[key].off, tabs[key].loc);
    }
    std::vector<Out> outs(n_req);
    uint64_t cells = 0, events = 0, refused = 0;
    for (uint32_t i : rng.perm(n_req)) {
        const Tab &t = tabs[(uint64_t)req[i].gene_start << 32 | req[i].gene_end];
        problem(c, ws, req[i], seqs, t.off.data(), t.loc.data(), log_cap ? log_cap : 0xFFFFFFFFu, cell_cap ? cell_cap : 0xFFFFFFFFu, rng, outs[i]);
    }
    uint64_t c_at = 0, f_at = 0;
    for (uint32_t i = 0; i < n_req; ++i) {
        const Out &o = outs[i];
        if (log_len) log_len[i] = (uint32_t)o.log;
        cells += o.cells;
        events += o.log;
        refused += o.flags & 1u;
        res[i] = cm_circ_chain_res{o.n_chains, (uint32_t)o.score.size(), o.listed, o.flags, c_at};
        for (size_t k = 0; k < o.score.size(); ++k) {
            if (c_at < cap_chains) {
                chain_score[c_at] = o.score[k];
                chain_len[c_at] = (uint32_t)o.r[k].size();
                chain_frag_off[c_at] = f_at;
            }
            for (size_t f = 0; f < o.r[k].size(); ++f)
                if (f_at + f < cap_frags) {
                    rpos[f_at + f] = o.r[k][f];
                    qpos[f_at + f] = o.q[k][f];
                }
            f_at += o.r[k].size();
            ++c_at;
        }
    }
    if (n_chains_out) *n_chains_out = c_at;
    if (n_frags_out) *n_frags_out = f_at;
    if (stats) {
        memset(stats, 0, 8 * sizeof(uint64_t));
        stats[0] = tabs.size();
        stats[3] = cells;
        stats[4] = events;
        stats[5] = refused;
    }
    return (c_at > cap_chains || f_at > cap_frags) ? CM_ELIMIT : CM_OK;
}

}  // extern "C"
