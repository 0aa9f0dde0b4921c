// cm_annot_probe.hip — test hook behind cm_annot_batch (include/circminer_hot.h): the annotation look-ups of cm_core.h, one
// request per lane on the device, against the AnnotDev of a loaded slot (the caller's: nothing is uploaded here but the requests).
//
// A translation unit of its own, compiled once, for the reason cm_dp_probe.hip gives: a test hook must not change how the
// product's kernels compile.  The look-ups do not depend on CM_MAX_CHAIN_FRAGS, and AnnotDev is the same struct in every build.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "circminer_hot.h"
#define cmc cmc_an                     // the bodies' namespace: every build of them has its own (cm_dispatch.cpp)
#include "cm_core.h"

namespace {

constexpr int BLK_ANNOT = 64;          // one wave per workgroup

// Lane l of workgroup v runs request 64 v + l: 64 different look-ups in flight per wave, through to_core() and the qualified
// pointers every kernel of cm_hot.hip reads the annotation with.  The common transcripts of kind 9 go to a lane-private array
// first, as in the pair kernels (process_mates), and from there to the request's 64 words of out_tids.
__global__ void __launch_bounds__(BLK_ANNOT) k_annot_probe(cmc::KCore kc, const cm_annot_req *req, uint32_t n_req, cm_annot_res *out, uint32_t *out_tids) {
    const uint64_t r = (uint64_t)blockIdx.x * BLK_ANNOT + threadIdx.x;
    if (r >= n_req) return;
    const cmc::Core c = cmc::to_core(kc);
    const cm_annot_req q = req[r];
    cm_annot_res v;
    uint32_t tids[cmc::MAX_TID];
    cmc::annot_req_run(c, q, v, tids);
    out[r] = v;
    if (q.kind == 9)
        for (int i = 0; i < v.ret && i < cmc::MAX_TID; ++i) out_tids[r * cmc::MAX_TID + i] = tids[i];
}

}  // namespace

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail((e_ == hipErrorOutOfMemory) ? CM_ENOMEM : CM_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// annot: the slot's cmc::AnnotDev (device pointers), annot_bytes its sizeof in the caller's build
extern "C" int cm_annot_probe_run(hipStream_t so, const cm_params *P, const void *annot, size_t annot_bytes, const cm_annot_req *req, uint32_t n_req,
                                  cm_annot_res *out, uint32_t *out_tids, char *err, size_t err_cap) {
    auto fail = [&](int code, const char *fmt, auto... a) {      // the message goes to the caller, who owns the context
        if (err && err_cap) snprintf(err, err_cap, fmt, a...);
        return code;
    };
    if (!P || !annot || (n_req && (!req || !out || !out_tids))) return fail(CM_EINVAL, "null argument");
    if (annot_bytes != sizeof(cmc::AnnotDev)) return fail(CM_EINVAL, "AnnotDev of %zu bytes, %zu here", annot_bytes, sizeof(cmc::AnnotDev));
    if (n_req > (1u << 24)) return fail(CM_EINVAL, "batch too large");
    cmc::KCore kc{};
    kc.P = *P;
    kc.A = *(const cmc::AnnotDev *)annot;
    const long long bad = cmc::annot_req_check(kc.A, req, n_req);
    if (bad < 0) return fail(CM_EINVAL, "no interval, or iv_bucket_shift %u (1 .. 31: a 32-bit position's bucket + 1 must not wrap)", kc.A.iv_bucket_shift);
    if (bad > 0) return fail(CM_EINVAL, "request %lld is not one the hook runs (kind, interval index in [-1, %u), mlen, order of the two positions)", bad - 1, kc.A.n_iv);
    if (n_req == 0) return CM_OK;
    struct Tmp {                                   // the hook's own device memory, gone when it returns
        void *p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } d_req, d_out, d_tids;
    const size_t tid_bytes = (size_t)n_req * cmc::MAX_TID * sizeof(uint32_t);
    HIPCHK(hipMalloc(&d_req.p, (size_t)n_req * sizeof(cm_annot_req)));
    HIPCHK(hipMalloc(&d_out.p, (size_t)n_req * sizeof(cm_annot_res)));
    HIPCHK(hipMalloc(&d_tids.p, tid_bytes));
    HIPCHK(hipMemcpyAsync(d_req.p, req, (size_t)n_req * sizeof(cm_annot_req), hipMemcpyHostToDevice, so));
    HIPCHK(hipMemsetAsync(d_out.p, 0, (size_t)n_req * sizeof(cm_annot_res), so));
    HIPCHK(hipMemsetAsync(d_tids.p, 0, tid_bytes, so));
    hipLaunchKernelGGL(k_annot_probe, dim3((n_req + BLK_ANNOT - 1) / BLK_ANNOT), dim3(BLK_ANNOT), 0, so, kc, (const cm_annot_req *)d_req.p, n_req,
                       (cm_annot_res *)d_out.p, (uint32_t *)d_tids.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, (size_t)n_req * sizeof(cm_annot_res), hipMemcpyDeviceToHost, so));
    HIPCHK(hipMemcpyAsync(out_tids, d_tids.p, tid_bytes, hipMemcpyDeviceToHost, so));
    HIPCHK(hipStreamSynchronize(so));
    return CM_OK;
}
