// annot_san_main.cpp — emu_annot_batch (tests/hostemu.cpp: the host build of cmc::annot_req_run) under the host sanitizers, as a
// stand-alone program: every array of the annotation is read into a heap block of exactly its size (the bitsets: (n_bits + 63) / 64
// words), so a look-up that reads one element outside any of them is an error here.  Built and run by
// tests/test_annot_requests_cpu.py::test_lookups_stay_inside_their_arrays over the files annot_requests_util.dump() writes:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -I include -I circminer_amd/csrc \
//       tests/diag/annot_san_main.cpp tests/hostemu.cpp -o annot_san && ./annot_san dense.anq long.anq
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "circminer_hot.h"

extern "C" int emu_annot_batch(const cm_params *P, const cm_annot_view *A, const cm_annot_req *req, uint32_t n_req, cm_annot_res *out, uint32_t *out_tids);

namespace {
template <class T> bool get(FILE *f, std::vector<T> &v) {
    uint64_t n;
    if (fread(&n, 8, 1, f) != 1) return false;
    v.resize(n);
    v.shrink_to_fit();
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
bool get64(FILE *f, uint64_t &x) { return fread(&x, 8, 1, f) == 1; }
}  // namespace

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint32_t> iv_spos, iv_epos, iv_max_end, iv_min_end, iv_max_next, iv_seg_off, iv_seg, seg_start, seg_end, seg_next, seg_gene, seg_tid_off,
            seg_tid, t2s_off, gene_start, gene_end, chr_shift, bucket;
        std::vector<int32_t> trans_start, chr_id;
        std::vector<uint8_t> t2s;
        std::vector<uint64_t> near, intr;
        uint64_t n_bits, shift, n_parts;
        bool ok = get(f, iv_spos) && get(f, iv_epos) && get(f, iv_max_end) && get(f, iv_min_end) && get(f, iv_max_next) && get(f, iv_seg_off) && get(f, iv_seg) &&
                  get(f, seg_start) && get(f, seg_end) && get(f, seg_next) && get(f, seg_gene) && get(f, seg_tid_off) && get(f, seg_tid) && get(f, trans_start) &&
                  get(f, t2s_off) && get(f, t2s) && get(f, gene_start) && get(f, gene_end) && get(f, near) && get(f, intr) && get(f, chr_shift) && get(f, chr_id) &&
                  get64(f, n_bits) && get(f, bucket) && get64(f, shift) && get64(f, n_parts);
        if (!ok || near.size() != (n_bits + 63) / 64 || intr.size() != near.size()) { fprintf(stderr, "%s: bad file\n", argv[a]); return 2; }
        cm_annot_view A{};
        A.n_iv = (uint32_t)iv_spos.size(); A.iv_spos = iv_spos.data(); A.iv_epos = iv_epos.data(); A.iv_max_end = iv_max_end.data(); A.iv_min_end = iv_min_end.data();
        A.iv_max_next_exon = iv_max_next.data(); A.iv_seg_off = iv_seg_off.data(); A.iv_seg = iv_seg.data();
        A.n_seg = (uint32_t)seg_start.size(); A.seg_start = seg_start.data(); A.seg_end = seg_end.data(); A.seg_next_exon_beg = seg_next.data();
        A.seg_gene_id = seg_gene.data(); A.seg_tid_off = seg_tid_off.data(); A.seg_tid = seg_tid.data();
        A.n_trans = (uint32_t)trans_start.size(); A.trans_start_ind = trans_start.data(); A.t2s_off = t2s_off.data(); A.t2s = t2s.data();
        A.n_gene = (uint32_t)gene_start.size(); A.gene_start = gene_start.data(); A.gene_end = gene_end.data();
        A.n_bits = n_bits; A.near_border_bits = near.data(); A.intronic_bits = intr.data();
        A.n_chr = (uint32_t)chr_shift.size(); A.chr_shift = chr_shift.data(); A.chr_id = chr_id.data();
        for (int table = 0; table < 2; ++table) {             // with the bucket table, and with the plain search
            A.iv_bucket = table && !bucket.empty() ? bucket.data() : nullptr;
            A.iv_bucket_shift = table ? (uint32_t)shift : 0;
            A.n_iv_bucket = table ? (uint32_t)bucket.size() : 0;
            const long at = ftell(f);
            for (uint64_t p = 0; p < n_parts; ++p) {
                cm_params P;
                std::vector<uint8_t> rq, ex;
                std::vector<uint32_t> want_tids;
                if (fread(&P, sizeof P, 1, f) != 1 || !get(f, rq) || !get(f, ex) || !get(f, want_tids)) return 2;
                const uint32_t n = (uint32_t)(rq.size() / sizeof(cm_annot_req));
                std::vector<cm_annot_req> req(n);
                std::vector<cm_annot_res> want(n), got(n);
                if (n) memcpy(req.data(), rq.data(), rq.size()), memcpy(want.data(), ex.data(), ex.size());
                std::vector<uint32_t> tids((size_t)n * 64);
                const int rc = emu_annot_batch(&P, &A, req.data(), n, got.data(), tids.data());
                size_t diff = 0;
                for (uint32_t i = 0; i < n; ++i) diff += memcmp(&got[i], &want[i], sizeof(cm_annot_res)) != 0;
                diff += tids != want_tids;
                printf("%s: table %d part %llu: rc %d, %u requests, %zu differ\n", argv[a], table, (unsigned long long)p, rc, n, diff);
                bad += rc != 0 || diff != 0;
            }
            if (table == 0) fseek(f, at, SEEK_SET);
        }
        fclose(f);
    }
    return bad ? 1 : 0;
}
