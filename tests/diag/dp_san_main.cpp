// dp_san_main.cpp — emu_dp_batch (tests/hostemu.cpp) under the host sanitizers, as a stand-alone program: the staging buffers of
// the hook hold exactly str_cap / 8 + 1 words, so an access past them is an error here and nowhere else.  Not part of the suite.
//
//   python -c "import sys; sys.path[:0] = ['.', 'tests']; import dp_requests_util as dq; [dq.dump(n, f'/tmp/{n}.dpq') for n in dq.ALL_BATCHES if n[0] in 'bcde']"
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -I include -I circminer_amd/csrc \
//       tests/diag/dp_san_main.cpp tests/hostemu.cpp -o /tmp/dp_san && /tmp/dp_san /tmp/*.dpq
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "circminer_hot.h"

extern "C" int emu_dp_batch(const cm_params *P, const uint8_t *arena, uint64_t arena_len, const cm_dp_req *req, uint32_t n_req, int str_cap, uint32_t lds_fill,
                            int arrangement, cm_dp_res *out);

int main(int argc, char **argv) {
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        cm_params P;
        int32_t cap;
        uint32_t n;
        uint64_t alen;
        if (fread(&P, sizeof P, 1, f) != 1 || fread(&cap, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&alen, 8, 1, f) != 1) return 2;
        std::vector<uint8_t> arena(alen);                 // exactly the arena: a read outside the pads is an error too
        std::vector<cm_dp_req> req(n);
        std::vector<cm_dp_res> want(n), got(n);
        if ((alen && fread(arena.data(), 1, alen, f) != alen) || (n && (fread(req.data(), sizeof(cm_dp_req), n, f) != n || fread(want.data(), sizeof(cm_dp_res), n, f) != n))) return 2;
        fclose(f);
        std::vector<cm_dp_req> k2;                         // the resumable form takes kind 2 at band 3
        std::vector<cm_dp_res> want2;
        for (uint32_t i = 0; i < n; ++i)
            if (req[i].kind == 2) { k2.push_back(req[i]); want2.push_back(want[i]); }
        for (int arr = 0; arr < (P.band == 3 ? 2 : 1); ++arr)
            for (uint32_t fill : {0x00000000u, 0x45454545u}) {
                const std::vector<cm_dp_req> &q = arr ? k2 : req;
                const std::vector<cm_dp_res> &w = arr ? want2 : want;
                const int rc = emu_dp_batch(&P, arena.data(), alen, q.data(), (uint32_t)q.size(), cap, fill, arr, got.data());
                size_t diff = 0;
                for (size_t i = 0; i < q.size(); ++i) diff += memcmp(&got[i], &w[i], sizeof(cm_dp_res)) != 0;
                printf("%s: arrangement %d fill %08x: rc %d, %zu requests, %zu differ\n", argv[a], arr, fill, rc, q.size(), diff);
                bad += rc != 0 || diff != 0;
            }
    }
    return bad ? 1 : 0;
}
