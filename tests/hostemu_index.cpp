// Host emulation of the device-side index builder (cm_build_contig) -- test infrastructure only.
//
// Runs the bodies of circminer_amd/csrc/cm_index_build.h the way the kernels of cm_hot.hip call them: tiles of TILE k-mer starts
// with k - 1 bases of halo as base codes, PER consecutive starts per lane (scan_positions), counters -> inclusive scan -> bucket
// ends, a scatter that takes slots from the end downwards, then every bucket ordered on the path bucket_path() names.  The lanes
// of the scatter run in a SHUFFLED order (seed), the order inside a bucket before the ordering pass is therefore arbitrary, as
// it is on the device.  The thresholds are arguments so that small inputs reach the workgroup and the oversize path.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "circminer_hot.h"
#include "cm_index_build.h"

namespace {
constexpr uint32_t TILE = 2048, PER = 8;
}

extern "C" int emu_index_build(const uint8_t *genome, uint32_t ref_len, int k, uint32_t lane_max, uint32_t wg_max, uint64_t seed, uint32_t *bucket_off,
                               uint16_t *checksum, uint32_t *pos, uint64_t cap_entries, uint64_t *n_entries, uint64_t paths[3], uint32_t *max_bucket) {
    if (!bucket_off || !n_entries || !paths || !max_bucket || k < cmib::WINDOW || k > cmib::WINDOW + 8 || lane_max < 1 || wg_max < lane_max) return CM_EINVAL;
    const int c = k - cmib::WINDOW;
    const uint64_t n_all = 1ull << (2 * cmib::WINDOW);
    const uint32_t n_pos = ref_len >= (uint32_t)k ? ref_len - (uint32_t)k + 1u : 0u;
    uint32_t *cursor = bucket_off;
    memset(cursor, 0, (n_all + 1) * sizeof(uint32_t));
    // one "lane" = PER consecutive starts of a tile; codes of the tile staged first, as the workgroup does in LDS
    struct Lane { uint32_t tile, first; };
    std::vector<Lane> lanes;
    for (uint64_t t0 = 0; t0 < n_pos; t0 += TILE)
        for (uint32_t f = 0; f < TILE && t0 + f < n_pos; f += PER) lanes.push_back(Lane{(uint32_t)(t0 / TILE), f});
    std::vector<uint8_t> codes(TILE + 32);
    auto run_lane = [&](const Lane &ln, auto &&f) {
        const uint64_t t0 = (uint64_t)ln.tile * TILE;
        const uint32_t tile_pos = (uint32_t)std::min<uint64_t>(n_pos - t0, TILE), n_codes = tile_pos + (uint32_t)k - 1;
        for (uint32_t i = 0; i < n_codes; ++i) codes[i] = (uint8_t)cmib::base_code(genome[t0 + i]);
        const uint32_t mine = std::min(tile_pos - ln.first, PER);
        cmib::scan_positions(codes.data() + ln.first, n_codes - ln.first, mine, k, c,
                             [&](uint32_t j, uint32_t hv, uint32_t ck) { f(hv, ck, (uint32_t)(t0 + ln.first + j) + 1u); });
    };
    for (const Lane &ln : lanes) run_lane(ln, [&](uint32_t hv, uint32_t, uint32_t) { ++cursor[hv]; });
    uint64_t run = 0;
    for (uint64_t h = 0; h <= n_all; ++h) {          // inclusive scan: cursor[h] = end of bucket h, cursor[4^14] = all entries
        run += cursor[h];
        cursor[h] = (uint32_t)run;
    }
    const uint64_t total = run;
    *n_entries = total;
    if (total > cap_entries) return CM_ELIMIT;
    std::mt19937_64 rng(seed);
    std::shuffle(lanes.begin(), lanes.end(), rng);
    for (const Lane &ln : lanes)
        run_lane(ln, [&](uint32_t hv, uint32_t ck, uint32_t p) {
            const uint32_t at = --cursor[hv];         // atomicSub(&cursor[hv], 1) - 1: the cursors finish as the bucket starts
            checksum[at] = (uint16_t)ck;
            pos[at] = p;
        });
    // ordering
    paths[0] = paths[1] = paths[2] = 0;
    *max_bucket = 0;
    std::vector<uint32_t> med, over;
    for (uint64_t h = 0; h < n_all; ++h) {
        const uint32_t b0 = bucket_off[h], n = bucket_off[h + 1] - b0;
        const int path = cmib::bucket_path(n, lane_max, wg_max);
        if (path < 0) continue;
        ++paths[path];
        *max_bucket = std::max(*max_bucket, n);
        if (path == 0) cmib::lane_sort(checksum + b0, pos + b0, n);
        else (path == 1 ? med : over).push_back((uint32_t)h);
    }
    std::shuffle(med.begin(), med.end(), rng);       // the lists are filled through an atomic counter: any order
    std::shuffle(over.begin(), over.end(), rng);
    std::vector<uint64_t> keys;
    for (uint32_t h : med) {                         // workgroup path: bitonic steps, every element of a step before the next step
        const uint32_t b0 = bucket_off[h], n = bucket_off[h + 1] - b0, np2 = cmib::pow2_at_least(n);
        keys.assign(np2, ~0ull);
        for (uint32_t i = 0; i < n; ++i) keys[i] = cmib::pack_key(checksum[b0 + i], pos[b0 + i]);
        for (uint32_t size = 2; size <= np2; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1)
                for (uint32_t i = np2; i-- > 0;) cmib::bitonic_step(keys.data(), i, size, stride);      // (descending: the order within a step is free)
        for (uint32_t i = 0; i < n; ++i) {
            checksum[b0 + i] = cmib::key_checksum(keys[i]);
            pos[b0 + i] = cmib::key_pos(keys[i]);
        }
    }
    for (size_t r0 = 0; r0 < over.size(); r0 += cmib::OVER_CHUNK) {     // oversize path: one sort of the packed keys per chunk of the list
        const size_t r1 = std::min(over.size(), r0 + (size_t)cmib::OVER_CHUNK);
        keys.clear();
        for (size_t r = r0; r < r1; ++r) {
            const uint32_t b0 = bucket_off[over[r]], n = bucket_off[over[r] + 1] - b0;
            for (uint32_t i = 0; i < n; ++i) keys.push_back(cmib::over_key((uint32_t)(r - r0), checksum[b0 + i], pos[b0 + i]));
        }
        std::sort(keys.begin(), keys.end());
        size_t at = 0;
        for (size_t r = r0; r < r1; ++r) {
            const uint32_t b0 = bucket_off[over[r]], n = bucket_off[over[r] + 1] - b0;
            for (uint32_t i = 0; i < n; ++i, ++at) {
                checksum[b0 + i] = cmib::key_checksum(keys[at]);
                pos[b0 + i] = cmib::key_pos(keys[at]);
            }
        }
    }
    return CM_OK;
}
