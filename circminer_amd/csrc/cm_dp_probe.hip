// cm_dp_probe.hip — test hook behind cm_dp_batch (include/circminer_hot.h): the three alignment DPs of cm_core.h, one request
// at a time on the device, against staging buffers laid out as the pair kernels lay them out.
//
// A translation unit of its own, compiled once: the DP bodies do not depend on CM_MAX_CHAIN_FRAGS, and with the probe in
// cm_hot.hip the compiler inlines the bodies differently into k_pair, k_pair_heavy and k_hp_tasks (other scratch sizes and spill
// counts) -- a test hook must not change the product's kernels.  What runs here is the same source as theirs (the DP bodies of
// cm_core.h, the staging layout and the queue loop of cm_dp_engine.h), compiled apart.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "circminer_hot.h"
#define cmc cmc_dp                     // the bodies' namespace: every build of them has its own (cm_dispatch.cpp)
#include "cm_core.h"

using cmc::Core;

namespace {

#include "cm_dp_engine.h"              // BLK_PAIR, lbuf_bytes, lane_dp_mem, dp_queue_loop: what the product's kernels use

// DpMem as every pair kernel of cm_hot.hip sets it up (lane_dp_mem): dynamic LDS of 2 * lbuf_bytes(str_cap) * 64 bytes; sm.err = the
// request's own err word.
// arrangement 0: the call as k_pair / k_hp_tasks make it, 64 different requests per wave.  arrangement 1: dp_queue_loop, the loop
// k_hp_dp (cm_heavy_pipe.h) runs -- that kernel's requests come from the pipeline's tables, here the queue is the request array itself.
__global__ void __launch_bounds__(BLK_PAIR, CM_PAIR_WAVES) k_dp_probe(cm_params P, const uint8_t *arena, const cm_dp_req *req, uint32_t n_req, int str_cap,
                                                                       uint32_t lds_fill, int arrangement, unsigned int *cursor, cm_dp_res *out) {
    extern __shared__ uint32_t lds_words[];
    const int lane = threadIdx.x;
    for (int i = lane; i < 2 * lbuf_bytes(str_cap) * BLK_PAIR / 4; i += BLK_PAIR) lds_words[i] = lds_fill;      // what the buffers hold before the first request
    __syncthreads();
    cmc::DpMem sm = lane_dp_mem((CM_S uint8_t *)lds_words, lane, str_cap, nullptr);
    Core c{};
    c.P = P;
    const cmc::g_u8 ar = (cmc::g_u8)arena;
    auto put = [&](uint32_t r, const int32_t v[4]) {           // (not the err word: the DP's own atomics write that one)
        out[r].ret = v[0];
        out[r].sc_len = v[1];
        out[r].indel = v[2];
        out[r].score = v[3];
    };
    if (arrangement == 0) {
        for (uint64_t r = (uint64_t)blockIdx.x * BLK_PAIR + lane; r < n_req; r += (uint64_t)gridDim.x * BLK_PAIR) {
            const cm_dp_req q = req[r];
            sm.err = (cmc::g_err)&out[r].err;
            int32_t v[4];
            cmc::dp_req_run(c, sm, ar, q, v);
            put((uint32_t)r, v);
        }
        return;
    }
    uint32_t my_r = 0;
    dp_queue_loop(sm, lane, cursor, n_req,
        [&](unsigned int mine, cmc::XdropLane &L, int) {                    // (dp_req_begin_w3 works the band's top out itself)
            my_r = mine;
            const cm_dp_req q = req[my_r];
            sm.err = (cmc::g_err)&out[my_r].err;
            int32_t v[4];
            if (!cmc::dp_req_begin_w3(c, sm, ar, q, L, v)) return true;
            put(my_r, v);                                                   // answered without a DP: the lane stays idle
            return false;
        },
        [&](const cmc::XdropLane &L) {
            int32_t v[4];
            v[0] = cmc::xdrop_w3_end(c, L, v[1], v[2], v[3]);          // (ret, sc_len, indel, score)
            put(my_r, v);
        });
}

}  // namespace

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail((e_ == hipErrorOutOfMemory) ? CM_ENOMEM : CM_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

extern "C" int cm_dp_probe_run(hipStream_t so, const cm_params *P, const uint8_t *arena, uint64_t arena_len, const cm_dp_req *req, uint32_t n_req,
                               int str_cap, uint32_t lds_fill, int arrangement, uint32_t grid, cm_dp_res *out, char *err, size_t err_cap) {
    auto fail = [&](int code, const char *fmt, auto... a) {      // the message goes to the caller, who owns the context
        if (err && err_cap) snprintf(err, err_cap, fmt, a...);
        return code;
    };
    if (!P || !arena || (n_req && (!req || !out))) return fail(CM_EINVAL, "null argument");
    if (n_req > (1u << 30) || arena_len > 0x7fffffffull) return fail(CM_EINVAL, "batch or arena too large");
    const long long bad = cmc::dp_req_check(*P, arena_len, req, n_req, str_cap, arrangement);
    if (bad < 0) return fail(CM_EINVAL, "str_cap %d, band %d or arrangement %d not supported", str_cap, P->band, arrangement);
    if (bad > 0)
        return fail(CM_EINVAL, "request %lld is not one the hook runs, or a view of it (with its pad of %d bytes) leaves the arena", bad - 1,
                    cmc::CM_STAGE_PAD);
    if (n_req == 0) return CM_OK;
    if (grid == 0) grid = (n_req + BLK_PAIR - 1) / BLK_PAIR;
    if (grid > 65536u) return fail(CM_EINVAL, "grid %u", grid);
    struct Tmp {                                   // the hook's own device memory, gone when it returns
        void *p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } d_arena, d_req, d_out, d_cur;
    HIPCHK(hipMalloc(&d_arena.p, arena_len));
    HIPCHK(hipMalloc(&d_req.p, (size_t)n_req * sizeof(cm_dp_req)));
    HIPCHK(hipMalloc(&d_out.p, (size_t)n_req * sizeof(cm_dp_res)));
    HIPCHK(hipMalloc(&d_cur.p, sizeof(unsigned int)));
    HIPCHK(hipMemcpyAsync(d_arena.p, arena, arena_len, hipMemcpyHostToDevice, so));
    HIPCHK(hipMemcpyAsync(d_req.p, req, (size_t)n_req * sizeof(cm_dp_req), hipMemcpyHostToDevice, so));
    HIPCHK(hipMemsetAsync(d_out.p, 0, (size_t)n_req * sizeof(cm_dp_res), so));
    HIPCHK(hipMemsetAsync(d_cur.p, 0, sizeof(unsigned int), so));
    const size_t lds_bytes = (size_t)2 * lbuf_bytes(str_cap) * BLK_PAIR;
    {   // dynamic-LDS limit of the kernel: a process-wide property, only ever raised (as for the pair kernels)
        static std::atomic<size_t> lim{48u * 1024u};
        if (lds_bytes > lim.load()) {
            HIPCHK(hipFuncSetAttribute((const void *)k_dp_probe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            lim.store(lds_bytes);
        }
    }
    hipLaunchKernelGGL(k_dp_probe, dim3(grid), dim3(BLK_PAIR), lds_bytes, so, *P, (const uint8_t *)d_arena.p, (const cm_dp_req *)d_req.p, n_req, str_cap,
                       lds_fill, arrangement, (unsigned int *)d_cur.p, (cm_dp_res *)d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, (size_t)n_req * sizeof(cm_dp_res), hipMemcpyDeviceToHost, so));
    HIPCHK(hipStreamSynchronize(so));
    return CM_OK;
}
