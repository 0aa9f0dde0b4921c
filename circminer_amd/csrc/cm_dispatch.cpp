// cm_dispatch.cpp — the public entry points of the device path.
//
// The kernels (cm_hot.hip) are compiled twice: once for reads of up to 16 seeds (floor(read length / k) <= 16: every 2x150 bp run,
// 300 bp down to k = 19) and once for up to 24 (300 bp at k = 14..18, reference src/commandline_parser.cpp:14,242-247).  The
// seed count sizes per-lane arrays and the chain records (136 vs 200 bytes each, 30 per problem), so the common case keeps the
// narrow build; cm_create picks the build from max_read_len / kmer and every other call follows the context.  Both builds
// export the same functions under a suffix (_k16 / _k24, renamed on the compiler command line by circminer_amd/_build.py).
//
// Everything below the four hand-written bodies comes from cm_device_abi.def, the one list of these functions (_build.py takes the
// names to rename from it too).  It is included three times: twice to declare the variants with the context types the renames give
// them (cm_ctx_k16 / cm_ctx_k24), once to hold every line against the declaration in circminer_hot.h -- a line whose parameter list
// differs from the header's does not compile -- and to emit the forwarding wrapper of every CM_DEV line.
#include <type_traits>

#include "circminer_hot.h"

struct cm_ctx_k16;
struct cm_ctx_k24;
struct cm_ctx {
    int wide;        // 0: _k16 build, 1: _k24 build
    union {
        cm_ctx_k16 *k16;
        cm_ctx_k24 *k24;
    };
};

#define CM_DEV(ret, name, params, args) CM_DEV_OWN(ret, name, params)
#define CM_DEV_OWN(ret, name, params) extern "C" ret name##_k16 params;
#define CM_CTX cm_ctx_k16
#include "cm_device_abi.def"
#undef CM_DEV_OWN
#undef CM_CTX
#define CM_DEV_OWN(ret, name, params) extern "C" ret name##_k24 params;
#define CM_CTX cm_ctx_k24
#include "cm_device_abi.def"
#undef CM_DEV
#undef CM_DEV_OWN
#undef CM_CTX

#define CM_DEV_OWN(ret, name, params) \
    static_assert(std::is_same<decltype(&name), ret (*) params>::value, #name ": cm_device_abi.def and circminer_hot.h declare it differently");
#define CM_DEV(ret, name, params, args)                       \
    CM_DEV_OWN(ret, name, params)                             \
    extern "C" ret name params {                              \
        if (!ctx) return CM_EINVAL;                           \
        if (ctx->wide) {                                      \
            cm_ctx_k24 *in = ctx->k24;                        \
            return name##_k24 args;                           \
        }                                                     \
        cm_ctx_k16 *in = ctx->k16;                            \
        return name##_k16 args;                               \
    }
#define CM_CTX cm_ctx
#include "cm_device_abi.def"

extern "C" {

int cm_create(const cm_params *p, cm_ctx **out) {
    if (!p || !out) return CM_EINVAL;
    *out = nullptr;
    if (p->kmer < CM_WINDOW_SIZE) return CM_EINVAL;
    const int seeds = p->max_read_len / p->kmer;
    cm_ctx *c = new cm_ctx{seeds > 16 ? 1 : 0, {nullptr}};
    const int rc = c->wide ? cm_create_k24(p, &c->k24) : cm_create_k16(p, &c->k16);
    if (rc != CM_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return CM_OK;
}
void cm_destroy(cm_ctx *ctx) {
    if (!ctx) return;
    if (ctx->wide) cm_destroy_k24(ctx->k24);
    else cm_destroy_k16(ctx->k16);
    delete ctx;
}
const char *cm_last_error(const cm_ctx *ctx) { return !ctx ? "null context" : (ctx->wide ? cm_last_error_k24(ctx->k24) : cm_last_error_k16(ctx->k16)); }
int cm_chain_batch(cm_ctx *ctx, int slot, cm_chain *out_chains, int32_t *out_nchain, int32_t *out_high) {
    if (!ctx) return CM_EINVAL;
    if (ctx->wide) return CM_ELIMIT;          // cm_chain of this ABI holds 16 fragments; the mapping entry points are not affected
    return cm_chain_batch_k16(ctx->k16, slot, out_chains, out_nchain, out_high);      // (the narrow build's cm_chain_k16 is this header's cm_chain)
}

}  // extern "C"
