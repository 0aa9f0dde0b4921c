// cm_dp_engine.h -- what the kernels that run the alignment DPs of cm_core.h share: the shape of a pair workgroup, the staging layout
// of the two DP strings in dynamic LDS, the loop that feeds a wave's lanes with DPs from a queue.  Included behind cm_core.h inside the
// anonymous namespace of cm_hot.hip (in front of cm_heavy_pipe.h) and of cm_dp_probe.hip; cmc:: is the includer's.
constexpr int BLK_PAIR = 64;
#ifndef CM_PAIR_WAVES
#define CM_PAIR_WAVES 4       // waves per SIMD the pair kernels are compiled for (128 VGPRs; LDS: 2 x lbuf_bytes x 64 per wave)
#endif
// bytes one staged string of `cap` characters takes per lane (cm_core.h LBuf: eight codes per word + one spare word)
__host__ __device__ constexpr int lbuf_bytes(int cap) { return (cap / 8 + 1) * 4; }

// The DpMem of one lane over `lds`, the workgroup's dynamic LDS: two buffers of lbuf_bytes(str_cap) * BLK_PAIR bytes, each
// word-interleaved across the wave (lane l owns the words l, l + 64, ...).  tick: -DCM_DIAG builds (DpMem has the member) pass &tick.
template <class... Tick>
__device__ __forceinline__ cmc::DpMem lane_dp_mem(CM_S uint8_t *lds, int lane, int str_cap, cmc::g_err err, Tick... tick) {
    CM_S uint8_t *lane_base = lds + 4 * lane;
    const int str_stride = lbuf_bytes(str_cap) * BLK_PAIR;
    return cmc::DpMem{cmc::LBuf{lane_base, str_cap}, cmc::LBuf{lane_base + str_stride, str_cap}, err, tick...};
}

// A wave works off the requests [0, tail) of a queue, one band-3 DP in flight per lane (cmc::XdropLane over sm.a / sm.b).  When
// REFILL lanes are idle they take the next requests from `cursor` (shared by all waves, one atomic per hand-out); the busy lanes
// advance in bursts of BURST double anti-diagonals; a lane whose DP has ended retires it and is idle again.  A wave is `dry` once a
// hand-out reached the tail, and leaves when it is dry and idle.
//   begin(mine, L, top) -> bool   request `mine` of the queue: stages its strings, cmc::xdrop_w3_begin(L, ...) -> true; or answers it
//                            without a DP -> false (the lane stays idle)
//   retire(L)                the DP this lane began last has ended: cmc::xdrop_w3_end and the answer to wherever it goes
template <class Begin, class Retire>
__device__ __forceinline__ void dp_queue_loop(const cmc::DpMem &sm, int lane, unsigned int *cursor, unsigned int tail, Begin begin, Retire retire) {
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    constexpr int REFILL = 16, BURST = 4;
    const int top = (sm.a.cap < sm.b.cap ? sm.a.cap : sm.b.cap) - 1;
    cmc::XdropLane L;
    L.go = false;
    bool busy = false, dry = false;
    for (;;) {
        const unsigned long long idle_m = __ballot(!busy);
        const int n_idle = __popcll(idle_m);
        if (!dry && (n_idle >= REFILL)) {
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(cursor, (unsigned int)n_idle);
            base = (unsigned int)__shfl((int)base, 0);
            if (base + (unsigned int)n_idle >= tail) dry = true;             // the queue has nothing beyond this hand-out
            const unsigned int mine = base + (unsigned int)__popcll(idle_m & lt_mask);
            if (!busy && mine < tail) busy = begin(mine, L, top);
        } else if (n_idle == 64) break;                                  // nothing in flight, nothing left to hand out
        for (int it = 0; it < BURST; ++it) {
            if (busy && L.go) cmc::xdrop_w3_advance(L, sm.a, sm.b, top);
            if (__ballot(busy && L.go) == 0ull) break;
        }
        if (busy && !L.go) {                                             // ended: its answer out, the lane is free
            retire(L);
            busy = false;
        }
    }
}
