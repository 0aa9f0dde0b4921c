// Stand-alone sanitizer pass over the bodies of circminer_amd/csrc/cm_circ_chain.h through the host emulation
// (tests/hostemu_circ_chain.cpp): a fabricated contig of 60 kb with one gene of three exons (introns of 1.5 and 4 kb) whose start is
// position 1, so that the annotation look-ups of the chaining -- which the reference runs on bare gene offsets -- see the junctions;
// a tandem gene whose buckets hold 1000 and 1001 hits; genes of 0, ws - 1 and ws bases; mates that lie inside an exon, run over a
// junction, hold N / NUL / lower case, hit a repeat family 64 times per seed, are shorter than a window, fill 128 seed positions
// (389 bases) and exceed them (refused); windows of 6, 8 and 10; log and cell capacities of 0 (no bound), 1 and the largest log.
// Every argument array is an exact-size heap block.  Checked here: the tables against cm_regional_table_build, the answers of two
// lane / cell / problem orders against each other, offsets and counts against the capacities.  (Equality with Caller::chains_of is
// tests/test_circ_chain_cpu.py's.)  CPU only, no Python.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I circminer_amd/csrc \
//       tests/diag/circ_chain_san_main.cpp tests/hostemu_circ_chain.cpp circminer_amd/csrc/host_annot.cpp circminer_amd/csrc/host_circ.cpp \
//       -o /tmp/circ_chain_san && /tmp/circ_chain_san
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "circminer_hot.h"

extern "C" int cm_cc_emu_table(const uint8_t *gene, uint32_t len, int32_t ws, uint64_t seed, uint32_t *off, uint32_t *loc);
extern "C" int cm_cc_emu(const cm_params *P, const cm_annot_view *av, int32_t window_size, const uint8_t *genome, uint32_t ref_len, const uint8_t *seqs,
                         uint64_t seqs_len, const cm_circ_chain_req *req, uint32_t n_req, cm_circ_chain_res *res, float *chain_score, uint32_t *chain_len,
                         uint64_t *chain_frag_off, uint64_t cap_chains, uint32_t *rpos, int32_t *qpos, uint64_t cap_frags, uint64_t *n_chains_out,
                         uint64_t *n_frags_out, uint64_t stats[8], uint32_t log_cap, uint32_t cell_cap, uint64_t seed, uint32_t *log_len);

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T> &v) {          // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static std::mt19937_64 rng(2024);
static std::string bases(size_t n) {
    std::string s(n, 'A');
    for (char &c : s) c = "ACGT"[rng() & 3];
    return s;
}

static int tables(const std::string &gene, int ws) {
    const size_t S = (size_t)1 << (2 * ws), nw = gene.size() >= (size_t)ws ? gene.size() - ws + 1 : 0;
    std::unique_ptr<uint8_t[]> g(new uint8_t[gene.size()]);
    memcpy(g.get(), gene.data(), gene.size());
    std::unique_ptr<uint32_t[]> off(new uint32_t[S + 1]), loc(new uint32_t[nw ? nw : 1]);
    CHECK(cm_cc_emu_table(gene.empty() ? nullptr : g.get(), (uint32_t)gene.size(), ws, rng(), off.get(), loc.get()) == CM_OK);
    uint32_t *ho = nullptr, *hl = nullptr;
    CHECK(cm_regional_table_build(g.get(), 0, (int32_t)gene.size(), ws, &ho, &hl) == CM_OK);
    CHECK(memcmp(ho, off.get(), (S + 1) * 4) == 0 && memcmp(hl, loc.get(), (size_t)ho[S] * 4) == 0);
    cm_regional_table_free(ho, hl);
    return 0;
}

int main() {
    // contig: exons at 201-400, 1901-2100, 6101-6400 (1-based), a repeat family from 10 001, a tandem gene from 30 001
    std::string contig = bases(60000);
    const std::string unit = bases(40);
    for (int c = 0; c < 64; ++c) contig.replace(10000 + (size_t)c * 90, 40, unit);
    const std::string tandem_unit = "ACGTTGCAGA";
    for (size_t i = 0; i < 10020; ++i) contig[30000 + i] = tandem_unit[i % 10];
    const char *gtf_path = "/tmp/circ_chain_san.gtf";
    {
        FILE *f = fopen(gtf_path, "w");
        CHECK(f);
        fprintf(f, "chr1\tsan\tgene\t201\t6400\t.\t+\t.\tgene_id \"G1\"; gene_name \"G1\";\n");
        fprintf(f, "chr1\tsan\ttranscript\t201\t6400\t.\t+\t.\tgene_id \"G1\"; transcript_id \"T1\"; gene_name \"G1\";\n");
        const int ex[3][2] = {{201, 400}, {1901, 2100}, {6101, 6400}};
        for (int e = 0; e < 3; ++e)
            fprintf(f, "chr1\tsan\texon\t%d\t%d\t.\t+\t.\tgene_id \"G1\"; transcript_id \"T1\"; exon_number \"%d\"; gene_name \"G1\";\n", ex[e][0], ex[e][1], e + 1);
        fclose(f);
    }
    const cm_chr_info chr{"chr1", 1, 0, (uint32_t)contig.size()};
    const uint32_t clen = (uint32_t)contig.size();
    cm_annot_view av;
    CHECK(cm_host_build_annotation(gtf_path, &chr, 1, &clen, 1, 300, &av) == CM_OK);
    remove(gtf_path);

    for (int ws : {6, 8, 10}) {
        CHECK(tables(contig.substr(30000, 10005 + ws - 1), ws) == 0);          // buckets of 1000 and of 1001 hits
        CHECK(tables("", ws) == 0 && tables(bases(ws - 1), ws) == 0 && tables(bases(ws), ws) == 0);
        std::string odd = bases(700);
        odd.replace(100, 30, std::string(30, 'N'));
        odd[300] = 0;
        for (size_t i = 400; i < 500; ++i) odd[i] = (char)(odd[i] | 0x20);
        CHECK(tables(odd, ws) == 0);
    }

    struct Gene { uint32_t s, e; };
    const Gene annotated{1, 7000}, family{10001, 10000 + 64 * 90}, tandem{30001, 40020}, beyond{59000, 61000}, zero{0, 100}, tiny{5000, 5005};
    std::vector<cm_circ_chain_req> req;
    std::string seqs;
    auto ask = [&](Gene g, const std::string &mate, uint32_t qs, uint32_t qe) {
        req.push_back(cm_circ_chain_req{g.s, g.e, seqs.size(), (uint32_t)mate.size(), qs, qe, 0});
        seqs += mate;
    };
    const std::string inside = contig.substr(220, 150), over1 = contig.substr(340, 60) + contig.substr(1900, 60), over2 = contig.substr(2040, 60) + contig.substr(6100, 90);
    ask(annotated, inside, 1, 150);
    ask(annotated, inside, 40, 150);
    ask(annotated, over1, 1, 120);
    ask(annotated, over2, 1, 150);
    ask(annotated, over1 + over2.substr(60), 1, 210);
    std::string dirty = inside;
    dirty[10] = 'N';
    dirty[50] = 0;
    for (size_t i = 80; i < 120; ++i) dirty[i] = (char)(dirty[i] | 0x20);
    ask(annotated, dirty, 1, 150);
    ask(annotated, std::string(150, 'N'), 1, 150);
    ask(annotated, inside, 1, 5);
    ask(annotated, inside, 150, 150);
    ask(annotated, inside, 151, 150);                                              // qe < qs
    ask(family, unit + bases(20), 1, 60);
    ask(family, unit, 1, 40);
    ask(tandem, contig.substr(30000, 63), 1, 63);
    ask(beyond, contig.substr(59000, 100), 1, 100);
    ask(zero, contig.substr(0, 100), 1, 100);
    ask(tiny, contig.substr(4990, 60), 1, 60);
    ask(annotated, contig.substr(200, 200) + contig.substr(1900, 189), 1, 389);      // 128 seed positions at ws = 8 (and at 6; 127 at 10)
    ask(annotated, contig.substr(200, 200) + contig.substr(1900, 200), 1, 400);      // more: refused

    for (int32_t max_intron : {2000000, 1000}) {
        cm_params P{};
        P.kmer = 20; P.seed_lim = 500; P.max_read_len = 300; P.max_ed = 4; P.max_sc = 7; P.band = 3; P.max_tlen = 500;
        P.max_intron = max_intron;
        P.max_chain_len = 30;
        for (int ws : {6, 8, 10}) {
            const uint32_t n = (uint32_t)req.size();
            uint64_t cap_c = 10ull * n, cap_f = 0;
            for (const auto &q : req) cap_f += 10ull * ((q.qe >= q.qs ? q.qe - q.qs + 1 : 0) / 3 + 1);
            const auto g = exact(std::vector<uint8_t>(contig.begin(), contig.end()));
            const auto sq = exact(std::vector<uint8_t>(seqs.begin(), seqs.end()));
            const auto rq = exact(req);
            struct Run {
                std::unique_ptr<cm_circ_chain_res[]> res;
                std::unique_ptr<float[]> score;
                std::unique_ptr<uint32_t[]> len, rpos, log_len;
                std::unique_ptr<uint64_t[]> frag_off;
                std::unique_ptr<int32_t[]> qpos;
                uint64_t nc = 0, nf = 0, stats[8];
            };
            auto run = [&](Run &r, uint32_t log_cap, uint32_t cell_cap, uint64_t seed) {
                r.res.reset(new cm_circ_chain_res[n]);
                r.score.reset(new float[cap_c]);
                r.len.reset(new uint32_t[cap_c]);
                r.frag_off.reset(new uint64_t[cap_c]);
                r.rpos.reset(new uint32_t[cap_f]);
                r.qpos.reset(new int32_t[cap_f]);
                r.log_len.reset(new uint32_t[n]);
                return cm_cc_emu(&P, &av, ws, g.get(), clen, sq.get(), seqs.size(), rq.get(), n, r.res.get(), r.score.get(), r.len.get(), r.frag_off.get(), cap_c,
                                 r.rpos.get(), r.qpos.get(), cap_f, &r.nc, &r.nf, r.stats, log_cap, cell_cap, seed, r.log_len.get());
            };
            Run a, b;
            CHECK(run(a, 0, 0, 1) == CM_OK && run(b, 0, 0, 99) == CM_OK);
            CHECK(a.nc == b.nc && a.nf == b.nf && memcmp(a.res.get(), b.res.get(), n * sizeof(cm_circ_chain_res)) == 0);
            CHECK(memcmp(a.score.get(), b.score.get(), a.nc * 4) == 0 && memcmp(a.len.get(), b.len.get(), a.nc * 4) == 0);
            CHECK(memcmp(a.rpos.get(), b.rpos.get(), a.nf * 4) == 0 && memcmp(a.qpos.get(), b.qpos.get(), a.nf * 4) == 0);
            uint64_t c_at = 0, f_at = 0;
            uint32_t top = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const cm_circ_chain_res &v = a.res[i];
                CHECK(v.chain_off == c_at && v.n_stored == (v.n_chains < 10 ? v.n_chains : 10) && v.n_chains <= (uint32_t)P.max_chain_len);
                for (uint32_t k = 0; k < v.n_stored; ++k, ++c_at) {
                    CHECK(a.frag_off[c_at] == f_at && a.len[c_at] >= 1 && a.len[c_at] <= v.listed);
                    for (uint32_t f = 0; f < a.len[c_at]; ++f, ++f_at) CHECK(a.rpos[f_at] >= req[i].gene_start && a.rpos[f_at] <= req[i].gene_end && a.qpos[f_at] >= 0);
                }
                top = a.log_len[i] > top ? a.log_len[i] : top;
            }
            CHECK(c_at == a.nc && f_at == a.nf);
            CHECK((a.res[n - 1].flags & 1u) == 1u && a.res[n - 2].flags == 0 && a.res[n - 2].n_chains >= 1 && a.stats[5] == 1);      // more than 128 positions: refused
            CHECK(a.res[0].n_chains >= 1 && a.res[6].listed == 0 && a.res[9].n_chains == 0 && a.res[13].n_chains == 0 && a.res[14].n_chains == 0);
            if (ws == 8 && max_intron == 2000000) CHECK(a.len[a.res[2].chain_off] > 30);      // the chain runs over the junction
            Run c;
            CHECK(run(c, top, 0, 5) == CM_OK && c.stats[5] == a.stats[5] && c.nc == a.nc);
            CHECK(run(c, 1, 0, 6) == CM_OK && c.stats[5] > a.stats[5]);
            CHECK(run(c, 0, 1, 7) == CM_OK && c.stats[5] > a.stats[5]);
            cap_c = a.nc - 1;                                                   // one short: CM_ELIMIT, nothing beyond the blocks
            CHECK(run(c, 0, 0, 8) == CM_ELIMIT);
            cap_c = 10ull * n;
            cap_f = a.nf - 1;
            CHECK(run(c, 0, 0, 8) == CM_ELIMIT);
        }
    }
    cm_host_free_annotation(&av, 1);
    printf("circ_chain_san: ok\n");
    return 0;
}
