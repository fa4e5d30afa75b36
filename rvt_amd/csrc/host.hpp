// Host-side helpers shared by the capi_*.hip translation units (argument checks, launch geometry, the tuning record).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "common.hpp"
#include "../../include/rvt_hip.h"

namespace rvt {
// The process-wide tuning / routing record (include/rvt_hip.h: RvtTuning, rvt_set_tuning).  Defined in capi_core.hip.
static inline const RvtTuning& tuning() { return g_tuning; }

static inline int pow2_ge(int v) { int p = 1; while (p < v) p <<= 1; return p; }
static inline int imin(int a, int b) { return a < b ? a : b; }
static inline int imax(int a, int b) { return a > b ? a : b; }
static inline int grid_for(size_t units, int cap = 2048) {
    size_t g = (units + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > (size_t)cap ? cap : g);
}
// one workgroup per CU (stem kernels, chain-MLP weight gradient); tuning.one_per_cu_grid: a smaller grid (tests: multi-tile walks)
static inline int one_per_cu_grid(int n_tiles) {
    const int cap = tuning().one_per_cu_grid > 0 ? tuning().one_per_cu_grid : 256;
    return n_tiles < 1 ? 1 : (n_tiles < cap ? n_tiles : cap);
}
// ---- shared by the stage drivers (capi_stage.hip, capi_train.hip) ----
static inline size_t elt_bytes(int dtype) { return dtype == RVT_F32 ? 4 : 2; }
static inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }
// bump allocator over the caller's workspace: every piece starts on an `align` boundary and is rounded up to one.  256 bytes for the
// no-grad driver; 2 MiB, like the caching allocator's large blocks, for the backward's temporaries (256-byte aligned pieces measured
// 0.15 ms per step slower at RVT-Base)
struct Carver {
    char* p; size_t left; size_t align; bool ok = true;
    void* take(size_t bytes) {
        const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(p) & (align - 1));
        if (mis) { const size_t skip = align - mis; if (skip > left) { ok = false; return nullptr; } p += skip; left -= skip; }
        bytes = (bytes + align - 1) & ~(align - 1);
        if (bytes > left) { ok = false; return nullptr; }
        void* r = p; p += bytes; left -= bytes;
        return r;
    }
};
// The forward launch sequence of one stage, written once for the no-grad and the training driver (defined in capi_stage.hip).
// stage_blocks_fwd: down-sampling conv + LayerNorm into y0 / x0, then the blocks; blk[bi] names the buffers of block bi, NULL where
// the route keeps nothing (RvtBlockSaved is that table: the training driver passes the saved activations, the no-grad driver its
// ping-pong buffers and shared scratch).  prepack: scratch for uint8 planes without a stem kernel, or NULL to refuse them.
int stage_blocks_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const void* inp, void* prepack, void* y0, void* x0,
                     const RvtBlockSaved* blk, int T, int B, void* stream);
// stage_lstm_scan_fwd: the ConvLSTM tail on the scan routes (r.lstm_route != 0); Hall slot 0 already holds the incoming h.
int stage_lstm_scan_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const void* x, void* Hall, const float* c0, float* c_last,
                        void* Csave, void* gates, const void* wp3, int T, int B, void* stream);
}  // namespace rvt
#define RVT_TRY(call) do { if ((call) != 0) return 1; } while (0)

// persistent grid = exactly the workgroups the chip holds at once for THIS kernel instantiation (registers + LDS)
// resident workgroups per CU of a kernel, queried once per kernel (the occupancy API is not free and must not run per
// launch; keyed by the kernel's address because several instantiations share one function type)
template <class K> static int resident_per_cu(K kernel, int threads, int fallback) {
#ifdef RVT_EMU
    return fallback;
#else
    struct Entry { const void* k; int v; };
    static Entry cache[64];
    static int n = 0;
    const void* key = reinterpret_cast<const void*>(kernel);
    for (int i = 0; i < n; i++) if (cache[i].k == key) return cache[i].v;
    int nb = 0, v = fallback;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0) == hipSuccess && nb > 0) v = nb;
    if (n < 64) cache[n++] = Entry{key, v};
    return v;
#endif
}

#define DISPATCH_DTYPE(dtype, ...)                                   \
    do {                                                             \
        if ((dtype) == RVT_F32) { typedef float T; __VA_ARGS__; }    \
        else if ((dtype) == RVT_BF16) { typedef bf16 T; __VA_ARGS__; } \
        else { set_last_error("bad dtype %d", (int)(dtype)); return 1; } \
    } while (0)

#define DISPATCH_BN(N, ...)                                          \
    do {                                                             \
        if ((N) <= 64) { constexpr int BN = 64; __VA_ARGS__; }       \
        else { constexpr int BN = 128; __VA_ARGS__; }                \
    } while (0)
