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
#define RVT_TRY(call) do { if ((call) != 0) return 1; } while (0)
// an asynchronous copy / memset of the HIP runtime inside a driver: RVT_HIP(hipMemsetAsync(..), "stage_seq_fwd: memset")
#define RVT_HIP(call, what) do { if ((call) != hipSuccess) { ::rvt::set_last_error("%s failed", what); return 1; } } while (0)
// ---- shared by the stage drivers (capi_stage.hip, capi_train.hip) ----
static inline size_t elt_bytes(int dtype) { return dtype == RVT_F32 ? 4 : 2; }
static inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }
// The shape arithmetic of one stage over T steps of B sequences, written once: output resolution, frames, token rows (all steps /
// one step), element size, bytes of one [M][C] activation, elements of one [B][H][W][C] state.  `who` names a driver: then the checks
// every driver makes before it launches anything are made here (the route planner and the *_ws_bytes functions pass NULL: they size
// and plan any shape, the driver refuses it).
struct StageShape { int H, W, F, M, Ms; size_t e, act, state; };
static inline int stage_shape(const RvtStageDesc& d, int T, int B, const char* who, StageShape* s) {
    s->H = conv_out(d.H_in, d.k, d.stride, d.pad); s->W = conv_out(d.W_in, d.k, d.stride, d.pad);
    s->F = T * B; s->Ms = B * s->H * s->W;
    const size_t tok = (size_t)T * s->Ms;
    s->M = (int)tok; s->e = elt_bytes(d.dtype); s->act = tok * d.C * s->e; s->state = (size_t)s->Ms * d.C;
    if (who == nullptr) return 0;
    RVT_CHECK(s->H % d.ph == 0 && s->W % d.pw == 0, "%s: %dx%d not divisible by the partition %dx%d", who, s->H, s->W, d.ph, d.pw);
    RVT_CHECK(tok * 4 * d.C < ((size_t)1 << 31), "%s: %zu token rows exceed the operators' 32-bit sizes", who, tok);
    return 0;
}
// bump allocator over the caller's workspace: every piece starts on an `align` boundary and is rounded up to one.  256 bytes for the
// no-grad driver; 2 MiB, like the caching allocator's large blocks, for the backward's temporaries (256-byte aligned pieces measured
// 0.15 ms per step slower at RVT-Base).  Without a base pointer it only counts: a driver's carve function run on such a Carver IS the
// driver's size function (bytes(): the rounded pieces plus one alignment unit for a base that is not aligned).
struct Carver {
    char* p; size_t left; size_t align; bool ok = true; size_t used = 0;
    static Carver counting(size_t align) { return Carver{nullptr, 0, align}; }
    size_t bytes() const { return used + align; }
    void* take(size_t n) {
        n = (n + align - 1) & ~(align - 1);
        used += n;
        if (p == nullptr) return nullptr;
        const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(p) & (align - 1));
        if (mis) { const size_t skip = align - mis; if (skip > left) { ok = false; return nullptr; } p += skip; left -= skip; }
        if (n > left) { ok = false; return nullptr; }
        void* r = p; p += n; left -= n;
        return r;
    }
};
// The forward launch sequence of one stage, written once for the no-grad and the training driver (defined in capi_stage.hip).
// stage_blocks_fwd: down-sampling conv + LayerNorm into y0 / x0, then the blocks; blk[bi] names the buffers of block bi, NULL where
// the route keeps nothing (RvtBlockSaved is that table: the training driver passes the saved activations, the no-grad driver its
// ping-pong buffers and shared scratch).  prepack: scratch for uint8 planes without a stem kernel, or NULL to refuse them.
int stage_blocks_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s, const void* inp, void* prepack, void* y0, void* x0,
                     const RvtBlockSaved* blk, void* stream);
// stage_lstm_fwd: the ConvLSTM tail (rnn.py:43-67) over the T steps of x on every lstm_route.  Scan routes: one launch; Hall slot 0
// already holds the incoming h, c0 NULL = zeros, Csave / gates NULL = not kept, wp3 the packed weights of route 3.  Per-step route:
// one rvt_lstm_fwd per row of `steps` - the driver's table of what step t reads (h, c) and writes (h, c, gates or NULL).
struct LstmStep { const void* h_in; const float* c_in; void* h_out; float* c_out; void* gates; };
int stage_lstm_fwd(const RvtStageDesc& d, const RvtStageRoutes& r, const StageShape& s, const void* x, void* Hall, const float* c0,
                   float* c_last, void* Csave, void* gates, const void* wp3, const LstmStep* steps, int T, void* stream);
}  // namespace rvt

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
