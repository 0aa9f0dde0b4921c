// cm_index_build.h — the per-position and per-bucket bodies of the device-side k-mer index builder (cm_build_contig).
//
// Shared by the HIP kernels (cm_hot.hip: k_ib_positions, k_ib_order_lane, k_ib_order_wg, k_ib_over_*) and by a host
// emulation (tests/hostemu_index.cpp) that g++ compiles, the way cm_core.h is shared.  The rules are those stated at the
// top of host_index.cpp:
//   * a k-mer (k = 14 + c) is indexed iff all k bases are upper-case A/C/G/T; its bucket is the 2-bit value of the first
//     14 bases, its checksum the 2-bit value of the remaining c bases, its position the 1-based start;
//   * inside a bucket entries are ordered by (checksum, position).
// The builder is a counting sort: count per bucket, scan, scatter in arbitrary order, then order every bucket by the 48-bit
// key (checksum, position).  Positions are unique, so the ordered result does not depend on the scatter order.
#ifndef CM_INDEX_BUILD_H
#define CM_INDEX_BUILD_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CMIB_HD __host__ __device__ inline
#else
#define CMIB_HD inline
#endif

namespace cmib {

constexpr int WINDOW = 14;                 // CM_WINDOW_SIZE
constexpr uint32_t CODE_BAD = 4;           // anything but upper-case A/C/G/T
// Which path orders a bucket of n entries: n <= LANE_MAX one lane (insertion sort in place), n <= WG_MAX one workgroup
// (bitonic sort of the packed keys in LDS: WG_MAX x 8 bytes = 32 KB), beyond that the listed oversize path (radix sort).
constexpr uint32_t LANE_MAX = 16;
constexpr uint32_t WG_MAX = 4096;

CMIB_HD uint32_t base_code(uint8_t ch) {
    switch (ch) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return CODE_BAD;
    }
}

// The k-mer starts of one stretch of sequence.  codes[0 .. n_codes) are the base codes from the stretch's first start
// position on; f(j, bucket, checksum) is called for every start j < n_pos whose k bases codes[j .. j + k) exist
// (j + k <= n_codes) and are all valid, in ascending j.  A lane of k_ib_positions walks its few consecutive starts with it,
// the emulation whole contigs.
template <class Codes, class F>
CMIB_HD void scan_positions(Codes codes, uint32_t n_codes, uint32_t n_pos, int k, int c, F f) {
    const uint64_t kmask = (1ull << (2 * k)) - 1, cmask = (1ull << (2 * c)) - 1;      // k <= 22
    const uint64_t want = (uint64_t)n_pos + (uint64_t)k - 1;
    const uint32_t lim = want < n_codes ? (uint32_t)want : n_codes;
    uint64_t v = 0;
    int run = 0;
    for (uint32_t i = 0; i < lim; ++i) {
        const uint32_t b = codes[i];
        if (b >= CODE_BAD) {
            run = 0;
            v = 0;
            continue;
        }
        v = ((v << 2) | (uint64_t)b) & kmask;
        if (++run >= k) f(i + 1 - (uint32_t)k, (uint32_t)(v >> (2 * c)), (uint32_t)(v & cmask));
    }
}

// -1: empty bucket, 0: lane, 1: workgroup, 2: oversize
CMIB_HD int bucket_path(uint32_t n, uint32_t lane_max, uint32_t wg_max) { return n == 0 ? -1 : (n <= lane_max ? 0 : (n <= wg_max ? 1 : 2)); }

CMIB_HD uint64_t pack_key(uint32_t checksum, uint32_t pos) { return ((uint64_t)checksum << 32) | pos; }
CMIB_HD uint16_t key_checksum(uint64_t key) { return (uint16_t)(key >> 32); }
CMIB_HD uint32_t key_pos(uint64_t key) { return (uint32_t)key; }
// keys of the oversize path: the bucket's rank in its chunk of the oversize list on top (a chunk holds up to 2^16 buckets)
constexpr uint32_t OVER_CHUNK = 1u << 16;
CMIB_HD uint64_t over_key(uint32_t rank, uint32_t checksum, uint32_t pos) { return ((uint64_t)rank << 48) | pack_key(checksum, pos); }

// lane path: the n entries at cs[] / ps[] ordered in place by (checksum, position)
CMIB_HD void lane_sort(uint16_t *cs, uint32_t *ps, uint32_t n) {
    for (uint32_t i = 1; i < n; ++i) {
        const uint64_t x = pack_key(cs[i], ps[i]);
        uint32_t j = i;
        while (j > 0 && pack_key(cs[j - 1], ps[j - 1]) > x) {
            cs[j] = cs[j - 1];
            ps[j] = ps[j - 1];
            --j;
        }
        if (j != i) {
            cs[j] = key_checksum(x);
            ps[j] = key_pos(x);
        }
    }
}

CMIB_HD uint32_t pow2_at_least(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}
// workgroup path: element i's part of step (size, stride) of a bitonic sort of np2 keys (np2 a power of two, the keys past
// the bucket's n are ~0).  All elements of a step are independent; a barrier separates the steps:
//   for (size = 2; size <= np2; size <<= 1) for (stride = size >> 1; stride > 0; stride >>= 1) { every i; barrier; }
CMIB_HD void bitonic_step(uint64_t *keys, uint32_t i, uint32_t size, uint32_t stride) {
    const uint32_t l = i ^ stride;
    if (l > i) {
        const uint64_t a = keys[i], b = keys[l];
        const bool up = (i & size) == 0;
        if ((a > b) == up) {
            keys[i] = b;
            keys[l] = a;
        }
    }
}

}  // namespace cmib
#endif /* CM_INDEX_BUILD_H */
