// Host emulation of cm_format_remain_sorted -- test infrastructure only.
//
// The order is made by the bodies of circminer_amd/csrc/cm_remain_order.h, the very functions the kernels of cm_hot.hip run, a lane
// at a time in a SHUFFLED order (seed): the keys, the heads, the groups' starts and sizes, and per mate file every entry's rank in
// its group.  Only the device's library calls are stood in for: std::stable_sort for the radix sort by the radix key, a plain loop
// for the scan.  Every list is an exact-size heap block, and either file's list is checked to be a permutation before it is used.
// The records are then hostemu_remain.cpp's business: cmrm::Format<MATE> over the file's own list, through the plan under shadow
// buffers, both files sized before either is written.
#include "hostemu_remain.cpp"

#include "cm_remain_order.h"

// cm_format_remain_sorted over host arrays: emu_format_remain's arguments, the offsets (nullable, count + 1 words each) and the cap
// of a tie group (0: cmro::TIE_CAP).  -102: a list is no permutation of the active set.
extern "C" int emu_format_remain_sorted(const cm_mapped_read *states, uint64_t n_pairs, const uint32_t *sel, uint64_t n_sel, const uint8_t *names1,
                                        const uint32_t *name_off1, const uint8_t *names2, const uint32_t *name_off2, const uint8_t *seq1, const uint64_t *off1,
                                        const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1, const uint8_t *qual2, const cm_chr_info *chrs,
                                        uint32_t n_chr, uint64_t first, uint64_t count, uint8_t *out1, uint64_t cap1, uint8_t *out2, uint64_t cap2,
                                        uint64_t *out_bytes, int64_t *out_keys, uint32_t *out_off1, uint32_t *out_off2, uint64_t *n_records, uint64_t *stats,
                                        uint64_t seed, uint32_t window, uint32_t tie_cap, uint32_t *tie_stats) {
    if (!out_bytes || (n_chr && !chrs)) return CM_EINVAL;
    out_bytes[0] = out_bytes[1] = 0;
    if (n_records) *n_records = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n_pairs == 0) return CM_ESTATE;
    if (n_records) *n_records = n_sel;
    if (!name_off1 || !name_off2 || !qual1 || !qual2) return CM_ESTATE;
    if (count == ~0ull && first <= n_sel) count = n_sel - first;
    if (first > n_sel || count > n_sel - first) return CM_EINVAL;
    if ((!out1 && cap1) || (!out2 && cap2)) return CM_EINVAL;
    if (count == 0) return CM_OK;
    if (window == 0) window = cmrt::WINDOW;
    if (window > cmrt::WINDOW) return CM_EINVAL;
    if (tie_cap == 0 || tie_cap > cmro::TIE_CAP) tie_cap = cmro::TIE_CAP;
    std::mt19937_64 rng(seed * 77 + 5);
    const uint32_t n = (uint32_t)n_sel;
    const ChrTable table(chrs, n_chr);
    const cmrt::ChrTab ct = table.tab();
    const std::vector<uint32_t> selv(sel, sel + n_sel);
    std::vector<uint32_t> shv(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) shv[c] = chrs[c].start_pos;
    uint32_t *p_sel = exact(selv), *p_sh = exact(shv);
    const Source s1(seq1, (size_t)off1[n_pairs]), s2(seq2, (size_t)off2[n_pairs]), q1(qual1, (size_t)off1[n_pairs]), q2(qual2, (size_t)off2[n_pairs]);
    int64_t *keys = (int64_t *)malloc(count * sizeof(int64_t));
    memset(keys, 0xa5, count * sizeof(int64_t));
    cmrm::Src S{p_sel, states, {names1, names2}, {name_off1, name_off2}, {s1.bytes(), s2.bytes()}, {q1.bytes(), q2.bytes()}, {off1, off2}, p_sh, out_keys ? keys : nullptr};
    // the plan of cm_remain_order.h
    auto block = [](size_t words, size_t size) { void *p = malloc(words * size ? words * size : 1); memset(p, 0xa5, words * size); return p; };
    uint64_t *rkey0 = (uint64_t *)block(n, 8), *rkey1 = (uint64_t *)block(n, 8);
    uint32_t *pair0 = (uint32_t *)block(n, 4), *by_key = (uint32_t *)block(n, 4), *heads = (uint32_t *)block((size_t)n + 1, 4), *gstart = (uint32_t *)block((size_t)n + 1, 4);
    uint32_t *list[2] = {(uint32_t *)block(n, 4), (uint32_t *)block(n, 4)};
    for (uint32_t q : shuffled(n, rng)) cmro::entry_key(S, ct.n, q, rkey0, pair0);
    {   // (the radix sort: stable, by the radix key)
        std::vector<uint32_t> idx(n);
        std::iota(idx.begin(), idx.end(), 0u);
        std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return rkey0[a] < rkey0[b]; });
        for (uint32_t i = 0; i < n; ++i) rkey1[i] = rkey0[idx[i]], by_key[i] = pair0[idx[i]];
    }
    for (uint32_t i : shuffled(n + 1, rng)) cmro::group_head(rkey1, n, i, heads);
    exclusive_scan(heads, (size_t)n + 1);
    for (uint32_t i : shuffled(n + 1, rng)) cmro::group_start(heads, n, i, gstart);
    uint32_t ties[3] = {0, 0, 0};
    for (uint32_t g : shuffled(n, rng)) {                          // (k_remain_gsizes: a lane per entry, the groups are the first of them)
        const uint32_t sz = cmro::group_size(gstart, heads[n], g);
        if (sz >= 2) ties[0] = std::max(ties[0], sz), ++ties[1], ties[2] += sz;
    }
    if (tie_stats) memcpy(tie_stats, ties, sizeof ties);
    int rc = CM_OK;
    if (ties[0] > tie_cap) rc = CM_ELIMIT;
    if (rc == CM_OK) {
        for (uint32_t i : shuffled(n, rng)) cmro::rank_in_group<0>(S, ct, by_key, heads, gstart, n, i, list[0]);
        for (uint32_t i : shuffled(n, rng)) cmro::rank_in_group<1>(S, ct, by_key, heads, gstart, n, i, list[1]);
        std::vector<uint32_t> want(selv);
        std::sort(want.begin(), want.end());
        for (int m = 0; m < 2; ++m) {
            std::vector<uint32_t> got(list[m], list[m] + n);
            std::sort(got.begin(), got.end());
            if (got != want) rc = -102;
        }
    }
    // the records of either file over its own list
    uint64_t need[2] = {0, 0}, w[2][3] = {{0, 0, 0}, {0, 0, 0}}, st[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    std::vector<uint32_t> offs[2] = {std::vector<uint32_t>(count + 1), std::vector<uint32_t>(count + 1)};
    auto run = [&](int m, uint8_t *out, uint64_t cap, uint64_t *bytes, uint64_t *sts, uint64_t *wr) {
        S.sel = list[m];
        return m ? format<cmrm::Format<1>>(S, chrs, n_chr, first, count, out, cap, bytes, sts, seed + 1, window, offs[1].data(), wr)
                 : format<cmrm::Format<0>>(S, chrs, n_chr, first, count, out, cap, bytes, sts, seed, window, offs[0].data(), wr);
    };
    if (rc == CM_OK) {
        for (int m = 0; m < 2; ++m) (void)run(m, nullptr, 0, &need[m], nullptr, nullptr);
        out_bytes[0] = need[0];
        out_bytes[1] = need[1];
        if (need[0] >= (1ull << 32) || need[1] >= (1ull << 32) || need[0] > cap1 || need[1] > cap2) rc = CM_ELIMIT;
    }
    for (int m = 0; m < 2 && rc == CM_OK; ++m) rc = run(m, m ? out2 : out1, m ? cap2 : cap1, &need[m], st[m], w[m]);
    if (rc == CM_OK) {
        if (w[0][0] != 1 || w[0][1] != 1 || w[1][0] != 1 || w[1][1] != 1) rc = -101;       // every byte of either file written once
        if (out_keys) memcpy(out_keys, keys, count * sizeof(int64_t));
        if (out_off1) memcpy(out_off1, offs[0].data(), (count + 1) * sizeof(uint32_t));
        if (out_off2) memcpy(out_off2, offs[1].data(), (count + 1) * sizeof(uint32_t));
        if (stats)
            for (int k = 0; k < 4; ++k) stats[k] = st[0][k] + st[1][k];
    }
    for (void *p : {(void *)rkey0, (void *)rkey1, (void *)pair0, (void *)by_key, (void *)heads, (void *)gstart, (void *)list[0], (void *)list[1], (void *)keys, (void *)p_sh, (void *)p_sel}) free(p);
    return rc;
}

// cmro::cmp_pairs of two pairs of mate file `mate`, for the directed comparator cases
extern "C" int emu_remain_cmp(const cm_mapped_read *states, uint64_t n_pairs, const uint8_t *names1, const uint32_t *name_off1, const uint8_t *names2,
                              const uint32_t *name_off2, const uint8_t *seq1, const uint64_t *off1, const uint8_t *seq2, const uint64_t *off2, const uint8_t *qual1,
                              const uint8_t *qual2, const cm_chr_info *chrs, uint32_t n_chr, uint32_t mate, uint32_t a, uint32_t b) {
    const ChrTable table(chrs, n_chr);
    const cmrt::ChrTab ct = table.tab();
    std::vector<uint32_t> shv(n_chr);
    for (uint32_t c = 0; c < n_chr; ++c) shv[c] = chrs[c].start_pos;
    uint32_t *p_sh = exact(shv);
    const Source s1(seq1, (size_t)off1[n_pairs]), s2(seq2, (size_t)off2[n_pairs]), q1(qual1, (size_t)off1[n_pairs]), q2(qual2, (size_t)off2[n_pairs]);
    const cmrm::Src S{nullptr, states, {names1, names2}, {name_off1, name_off2}, {s1.bytes(), s2.bytes()}, {q1.bytes(), q2.bytes()}, {off1, off2}, p_sh, nullptr};
    const int c = mate ? cmro::cmp_pairs<1>(S, ct, a, b) : cmro::cmp_pairs<0>(S, ct, a, b);
    free(p_sh);
    return c;
}
