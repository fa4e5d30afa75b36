// Raw event streams -> a whole (T, B, 2*bins, H', W') sequence of stacked histograms, window slicing and the 1 Mpx half-scale
// down-sampling included (reference scripts/genx/preprocess_dataset.py:480-534: two searchsorted over the timestamps, one
// StackedHistogram.construct per window, interpolate(scale_factor=0.5, mode='nearest-exact') of the full-size histogram).
//
//   bounds:   end = searchsorted(t, ts_end, 'right');  start = searchsorted(t, ts_end - delta, 'left')  or  max(end - N, 0)
//   count:    per window, the bin rule of events.hpp (hist_count_kernel) on t0 = t[start], t1 = t[end-1] of the WHOLE window;
//             one 32-bit atomicAdd per kept event into a scratch image, so the result does not depend on the arrival order
//   finalize: accumulator wrap (uint8 / int16 + clamp(min=0)), min(cutoff), narrow to uint8, 16 cells per lane and one 16-byte
//             store, straight into out + window * cells; the scratch cells it has read are zeroed for the next chunk
//
// Half-scale nearest-exact picks source pixel 2i + 1: out[c][i][j] = full[c][2i+1][2j+1], and the per-cell wrap / clamp commute
// with that selection.  With `ds` the count kernel therefore drops every event with even x or even y BEFORE the atomic and
// counts the rest at (y >> 1, x >> 1) of an H/2 x W/2 image: a quarter of the atomics, and no full-resolution image anywhere.
// For odd x < W, x >> 1 <= (W - 2) / 2 < W / 2, so an odd-sized sensor's last (even) row / column drops out by the same test.
//
// The grids cannot depend on the bounds (they live on the device: no host synchronisation, graph-capturable, and the event
// count n of every stream is read on the device too), so grid y is the window and a fixed number of workgroups stride over
// [start, end).  Event loads are 16-byte vectors over groups of 8 events aligned to absolute index 8k (windows start anywhere:
// the head and tail of at most 7 events each are peeled), when the four base pointers are 16-byte aligned; element loads else.
//
// The same skeleton builds the reference's second representation, MixedDensityEventStack (data/utils/representations.py:130-218;
// EVSEQ_MIXED below): bounds and the load / peel loop are shared, the cell rule and the narrowing pass differ.
//   count:    tn = clamp(float32(t - t0) / float32(max(t1 - t0, 1)), 1e-6f, float32(1 - 1e-6));  bin = max(bins + e, 0) with e the
//             unbiased binary exponent of tn, which IS floor(bins - log(tn) / log(1/2)) as tn < 1 (no logarithm: exact for every
//             span, and equal to the reference's fp32 log quotient wherever that one is right, i.e. spans up to 2^20 us);
//             atomicAdd(+1 / -1) for polarity 1 / 0 into an int32 image [bins][H'][W']
//   finalize: per pixel the running sum over the bin axis (the reference's cumsum_channel), the int8 wrap (low 8 bits: one wrap
//             at the end equals the reference's wrap after the scatter and again after the sum, arithmetic modulo 256), the
//             clamp to [-cutoff, cutoff] when there is a cutoff, int8 out; 16 pixels per lane and one 16-byte store per bin
// The per-pixel sum, wrap and clamp commute with the half-scale selection of odd pixels, so `ds` works as above.
#pragma once
#include "common.hpp"

namespace rvt {

// One row of the stream table, declared in include/rvt_hip.h; the empty derived struct keeps the kernels' symbol names.
struct EvStream : RvtEventStream {};

typedef __attribute__((ext_vector_type(2))) long long i64x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));          // dword-aligned 16-byte access (scratch cells behind a peeled head)

// The event arrays are reached through pointers read from the table: without this the compiler has to assume the generic
// address space and emits flat loads (which also tick the LDS counter) instead of global loads.
#ifdef RVT_EMU
#define EVSEQ_GLOBAL
#else
#define EVSEQ_GLOBAL __attribute__((address_space(1)))
#endif

constexpr int EVSEQ_THREADS = 256;
constexpr int EVSEQ_HIST = 0, EVSEQ_MIXED = 1;               // the representation a count kernel is instantiated for

// ---------------------------------------------------------------------------------------------------------- window bounds
__global__ void __launch_bounds__(EVSEQ_THREADS)
evseq_bounds_kernel(const EvStream* __restrict__ table, int B, int T, long long delta_us, long long n_events,
                    long long* __restrict__ bounds) {
    const int i = blockIdx.x * EVSEQ_THREADS + threadIdx.x;
    if (i >= B * T) return;
    const int b = i / T, w = i - b * T;
    const EvStream s = table[b];
    const long long n = s.n > 0 ? s.n : 0;
    const EVSEQ_GLOBAL long long* t = (const EVSEQ_GLOBAL long long*)s.t;
    const long long te = ((const EVSEQ_GLOBAL long long*)s.ts_end)[w];
    long long lo = 0, hi = n;                                  // side='right': first index with t > te
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (t[mid] <= te) lo = mid + 1; else hi = mid;
    }
    const long long end = lo;
    long long start;
    if (n_events > 0) {
        start = end - n_events > 0 ? end - n_events : 0;
    } else {
        const long long ts = te - delta_us;
        lo = 0; hi = end;                                      // side='left': first index with t >= ts (<= end as ts <= te)
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (t[mid] < ts) lo = mid + 1; else hi = mid;
        }
        start = lo;
    }
    bounds[2 * (size_t)i] = start;
    bounds[2 * (size_t)i + 1] = end;
}

// ------------------------------------------------------------------------------------------------------------------ count
// a coordinate or polarity of any width as an int: negative stays negative, anything beyond int saturates (out of range for
// every sensor, and > 1 for a polarity)
template <class CT> __device__ __forceinline__ int evseq_narrow(CT c) {
    if constexpr (sizeof(CT) == 8) return c < 0 ? -1 : (c > 0x7fffffffLL ? 0x7fffffff : (int)c);
    else return (int)c;
}

// the scratch cell of one event, or -1 when the event does not count
__device__ __forceinline__ long long evseq_cell_of(int xi, int yi, int pi, long long ti64, long long t0, float den, int bins, int H, int W,
                                                   int ds, int Ho, int Wo) {
    float tn = (float)(ti64 - t0) / den;          // correctly rounded fp32 division, as torch's
    tn = tn * (float)bins;
    int ti = (int)floorf(tn);
    ti = ti < bins - 1 ? ti : bins - 1;
    pi = pi < 0 ? 0 : pi;                                                                  // the reader's clip(p, a_min=0)
    if (xi < 0 || xi >= W || yi < 0 || yi >= H || pi > 1 || ti < 0) return -1;             // (reference: index error)
    if (ds) {
        if (!(xi & 1) || !(yi & 1)) return -1;                                            // only odd x AND odd y reach the half-scale image
        xi >>= 1; yi >>= 1;
    }
    return (long long)((((size_t)pi * bins + ti) * Ho + yi) * Wo + xi);
}

// MixedDensityEventStack: the bin of one timestamp (see the head of this file)
__device__ __forceinline__ int evseq_md_bin(long long ti64, long long t0, float den, int bins) {
    float tn = (float)(ti64 - t0) / den;          // correctly rounded fp32 division, as torch's
    const float lo = 1e-6f, hi = (float)(1.0 - 1e-6);
    tn = tn < lo ? lo : (tn > hi ? hi : tn);
    const int e = (int)((__builtin_bit_cast(unsigned, tn) >> 23) & 0xffu) - 127;         // tn >= 1e-6 is a normal number
    return bins + e > 0 ? bins + e : 0;
}

// the scratch cell of one event in the [bins][Ho][Wo] image of the mixed-density stack, or -1 when the event does not count
__device__ __forceinline__ long long evseq_md_cell_of(int xi, int yi, int pi, long long ti64, long long t0, float den, int bins, int H,
                                                      int W, int ds, int Ho, int Wo) {
    if (xi < 0 || xi >= W || yi < 0 || yi >= H || pi > 1) return -1;
    if (ds) {
        if (!(xi & 1) || !(yi & 1)) return -1;
        xi >>= 1; yi >>= 1;
    }
    return (long long)((((size_t)evseq_md_bin(ti64, t0, den, bins)) * Ho + yi) * Wo + xi);
}

template <int REP>
__device__ __forceinline__ void evseq_count_one(int xi, int yi, int pi, long long ti64, long long t0, float den, int bins, int H, int W,
                                                int ds, int Ho, int Wo, unsigned* __restrict__ img) {
    if constexpr (REP == EVSEQ_MIXED) {
        const long long c = evseq_md_cell_of(xi, yi, pi, ti64, t0, den, bins, H, W, ds, Ho, Wo);
        if (c >= 0) atomicAdd(reinterpret_cast<int*>(img) + c, pi > 0 ? 1 : -1);          // polarity < 0 counts as 0, as above
    } else {
        const long long c = evseq_cell_of(xi, yi, pi, ti64, t0, den, bins, H, W, ds, Ho, Wo);
        if (c >= 0) atomicAdd(img + c, 1u);
    }
}

// 8 consecutive elements starting at an index that is a multiple of 8 of a 16-byte aligned array: 16-byte loads
template <class CT> __device__ __forceinline__ void evseq_load8(const EVSEQ_GLOBAL CT* __restrict__ p, long long i, int (&v)[8]) {
    constexpr int PER = 16 / (int)sizeof(CT);
    typedef CT vec_t __attribute__((ext_vector_type(PER)));
#pragma unroll
    for (int k = 0; k < 8 / PER; k++) {
        const vec_t q = *reinterpret_cast<const EVSEQ_GLOBAL vec_t*>(p + i + k * PER);
#pragma unroll
        for (int j = 0; j < PER; j++) v[k * PER + j] = evseq_narrow<CT>(q[j]);
    }
}

// grid (blocks per window, windows of this chunk).  Window g = g0 + blockIdx.y is time step g / B of sample g % B and counts
// into scratch image blockIdx.y (slot_cells apart).  REP selects the cell rule; loads and peeling are the same for both.
template <class CT, int REP> __global__ void __launch_bounds__(EVSEQ_THREADS)
evseq_count_kernel(const EvStream* __restrict__ table, const long long* __restrict__ bounds, int g0, int B, int T, int bins, int H,
                   int W, int ds, size_t slot_cells, unsigned* __restrict__ scratch) {
    const int g = g0 + blockIdx.y;
    const int w = g / B, b = g - w * B;
    const long long start = bounds[2 * ((size_t)b * T + w)], end = bounds[2 * ((size_t)b * T + w) + 1];
    if (end <= start) return;
    const EvStream s = table[b];
    const EVSEQ_GLOBAL CT* __restrict__ x = (const EVSEQ_GLOBAL CT*)s.x;
    const EVSEQ_GLOBAL CT* __restrict__ y = (const EVSEQ_GLOBAL CT*)s.y;
    const EVSEQ_GLOBAL CT* __restrict__ pol = (const EVSEQ_GLOBAL CT*)s.p;
    const EVSEQ_GLOBAL long long* __restrict__ time = (const EVSEQ_GLOBAL long long*)s.t;
    const int Ho = ds ? H >> 1 : H, Wo = ds ? W >> 1 : W;
    unsigned* __restrict__ img = scratch + (size_t)blockIdx.y * slot_cells;
    const long long t0 = time[start], t1 = time[end - 1];
    const float den = (float)((t1 - t0) > 1 ? (t1 - t0) : 1);

    const bool vec = ((((uintptr_t)s.x) | ((uintptr_t)s.y) | ((uintptr_t)s.p) | ((uintptr_t)s.t)) & 15) == 0;
    long long a0 = end, a1 = end;                               // [a0, a1): whole groups of 8 at absolute indices 8k
    if (vec) {
        a0 = (start + 7) & ~7LL;
        a0 = a0 < end ? a0 : end;
        a1 = end & ~7LL;
        a1 = a1 > a0 ? a1 : a0;
    }
    if (vec) {
        const long long groups = (a1 - a0) >> 3;
        for (long long q = (long long)blockIdx.x * EVSEQ_THREADS + threadIdx.x; q < groups; q += (long long)gridDim.x * EVSEQ_THREADS) {
            const long long i = a0 + 8 * q;
            int xv[8], yv[8], pv[8];
            evseq_load8<CT>(x, i, xv);
            evseq_load8<CT>(y, i, yv);
            evseq_load8<CT>(pol, i, pv);
            long long tv[8];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const i64x2 tq = *reinterpret_cast<const EVSEQ_GLOBAL i64x2*>(time + i + 2 * k);
                tv[2 * k] = tq[0]; tv[2 * k + 1] = tq[1];
            }
#ifdef EVSEQ_AGGREGATE
            static_assert(REP == EVSEQ_HIST, "EVSEQ_AGGREGATE is a variant of the stacked-histogram count only");
            long long cur = -1;
            unsigned cnt = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const long long c = evseq_cell_of(xv[k], yv[k], pv[k], tv[k], t0, den, bins, H, W, ds, Ho, Wo);
                if (c == cur) { cnt++; continue; }
                if (cur >= 0) atomicAdd(img + cur, cnt);
                cur = c; cnt = 1;
            }
            if (cur >= 0) atomicAdd(img + cur, cnt);
#else
#pragma unroll
            for (int k = 0; k < 8; k++) evseq_count_one<REP>(xv[k], yv[k], pv[k], tv[k], t0, den, bins, H, W, ds, Ho, Wo, img);
#endif
        }
        if (blockIdx.x == 0 && threadIdx.x < 16) {              // peeled head [start, a0) and tail [a1, end): at most 7 events each
            const long long i = threadIdx.x < 8 ? start + threadIdx.x : a1 + (threadIdx.x - 8);
            const long long lim = threadIdx.x < 8 ? a0 : end;
            if (i < lim)
                evseq_count_one<REP>(evseq_narrow<CT>(x[i]), evseq_narrow<CT>(y[i]), evseq_narrow<CT>(pol[i]), time[i], t0, den, bins, H, W,
                                     ds, Ho, Wo, img);
        }
    } else {
        for (long long i = start + (long long)blockIdx.x * EVSEQ_THREADS + threadIdx.x; i < end; i += (long long)gridDim.x * EVSEQ_THREADS)
            evseq_count_one<REP>(evseq_narrow<CT>(x[i]), evseq_narrow<CT>(y[i]), evseq_narrow<CT>(pol[i]), time[i], t0, den, bins, H, W, ds,
                                 Ho, Wo, img);
    }
}

// --------------------------------------------------------------------------------------------------------------- finalize
__device__ __forceinline__ unsigned evseq_cell(unsigned c, int cutoff, int fastmode) {
    int v;
    if (fastmode) v = (int)(c & 0xffu);                            // uint8 accumulator: modulo 256
    else { v = (int)(short)(c & 0xffffu); v = v < 0 ? 0 : v; }     // int16 accumulator, clamp(min=0)
    return (unsigned)(v < cutoff ? v : cutoff);
}

// grid (blocks per window, windows of this chunk): scratch image blockIdx.y -> out + (g0 + blockIdx.y) * cells, and the image
// is left zero.  The 16-byte stores need dst aligned: `head` cells in front of the first aligned byte and the cells behind the
// last whole vector go one by one (at most 15 each; cells is not always a multiple of 16 and out may start anywhere).
__global__ void __launch_bounds__(EVSEQ_THREADS)
evseq_finalize_kernel(unsigned* __restrict__ scratch, unsigned char* __restrict__ out, int g0, size_t cells, size_t slot_cells,
                      int cutoff, int fastmode) {
    unsigned* __restrict__ img = scratch + (size_t)blockIdx.y * slot_cells;
    unsigned char* __restrict__ dst = out + (size_t)(g0 + blockIdx.y) * cells;
    size_t head = (size_t)((16 - ((uintptr_t)dst & 15)) & 15);
    head = head < cells ? head : cells;
    const size_t nvec = (cells - head) >> 4;
    for (size_t q = (size_t)blockIdx.x * EVSEQ_THREADS + threadIdx.x; q < nvec; q += (size_t)gridDim.x * EVSEQ_THREADS) {
        const size_t i = head + 16 * q;
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u32x4 c = *reinterpret_cast<const u32x4_a4*>(img + i + 4 * k);
            o[k] = evseq_cell(c[0], cutoff, fastmode) | (evseq_cell(c[1], cutoff, fastmode) << 8) |
                   (evseq_cell(c[2], cutoff, fastmode) << 16) | (evseq_cell(c[3], cutoff, fastmode) << 24);
            *reinterpret_cast<u32x4_a4*>(img + i + 4 * k) = u32x4{0u, 0u, 0u, 0u};
        }
        *reinterpret_cast<u32x4*>(dst + i) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const size_t body_end = head + 16 * nvec;
        const size_t i = threadIdx.x < 16 ? (size_t)threadIdx.x : body_end + (threadIdx.x - 16);
        const size_t lim = threadIdx.x < 16 ? head : cells;
        if (i < lim) {
            dst[i] = (unsigned char)evseq_cell(img[i], cutoff, fastmode);
            img[i] = 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------- mixed-density stack
// one window given as four int64 arrays (rvt_mixed_density_stack): the cell rule above at full size into one image
__global__ void __launch_bounds__(EVSEQ_THREADS)
evseq_md_window_kernel(const long long* __restrict__ x, const long long* __restrict__ y, const long long* __restrict__ pol,
                       const long long* __restrict__ time, size_t n, int bins, int H, int W, unsigned* __restrict__ img) {
    const long long t0 = time[0], t1 = time[n - 1];
    const float den = (float)((t1 - t0) > 1 ? (t1 - t0) : 1);
    for (size_t i = (size_t)blockIdx.x * EVSEQ_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * EVSEQ_THREADS)
        evseq_count_one<EVSEQ_MIXED>(evseq_narrow<long long>(x[i]), evseq_narrow<long long>(y[i]), evseq_narrow<long long>(pol[i]), time[i],
                                     t0, den, bins, H, W, 0, H, W, img);
}

// running sum (modulo 2^32) -> the reference's int8 value: wrap, then the clamp when there is a cutoff (cutoff < 0: none)
__device__ __forceinline__ unsigned evseq_md_value(unsigned run, int cutoff) {
    int v = (int)(signed char)(run & 0xffu);
    if (cutoff >= 0) { v = v < -cutoff ? -cutoff : v; v = v > cutoff ? cutoff : v; }
    return (unsigned)v & 0xffu;
}

// one pixel through all its bins, cell by cell
__device__ __forceinline__ void evseq_md_pixel(unsigned* __restrict__ img, signed char* __restrict__ dst, size_t i, size_t plane, int bins,
                                               int cutoff) {
    unsigned run = 0u;
    for (int b = 0; b < bins; b++) {
        const size_t c = (size_t)b * plane + i;
        run += img[c];
        img[c] = 0u;
        dst[c] = (signed char)evseq_md_value(run, cutoff);
    }
}

// grid (blocks per window, windows of this chunk): scratch image blockIdx.y [bins][plane] -> out + (g0 + blockIdx.y) * bins * plane,
// and the image is left zero.  A lane owns 16 consecutive pixels and walks the bins with their running sums in registers.  The
// 16-byte stores need every plane's piece aligned, i.e. plane % 16 == 0 and a start behind `head` peeled pixels; the peeled
// pixels (at most 15 at either end) and every pixel of a plane size off that grid (7 x 10, ...) go one pixel per lane.
__global__ void __launch_bounds__(EVSEQ_THREADS)
evseq_md_finalize_kernel(unsigned* __restrict__ scratch, signed char* __restrict__ out, int g0, int bins, size_t plane, size_t slot_cells,
                         int cutoff) {
    unsigned* __restrict__ img = scratch + (size_t)blockIdx.y * slot_cells;
    signed char* __restrict__ dst = out + (size_t)(g0 + blockIdx.y) * bins * plane;
    const size_t lane = (size_t)blockIdx.x * EVSEQ_THREADS + threadIdx.x, lanes = (size_t)gridDim.x * EVSEQ_THREADS;
    if (plane & 15) {
        for (size_t i = lane; i < plane; i += lanes) evseq_md_pixel(img, dst, i, plane, bins, cutoff);
        return;
    }
    size_t head = (size_t)((16 - ((uintptr_t)dst & 15)) & 15);
    head = head < plane ? head : plane;
    const size_t nvec = (plane - head) >> 4;
    for (size_t q = lane; q < nvec; q += lanes) {
        const size_t i = head + 16 * q;
        unsigned run[16];
#pragma unroll
        for (int k = 0; k < 16; k++) run[k] = 0u;
        for (int b = 0; b < bins; b++) {
            unsigned* __restrict__ cell = img + (size_t)b * plane + i;
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u32x4 c = *reinterpret_cast<const u32x4_a4*>(cell + 4 * k);
                *reinterpret_cast<u32x4_a4*>(cell + 4 * k) = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; j++) run[4 * k + j] += c[j];
                o[k] = evseq_md_value(run[4 * k], cutoff) | (evseq_md_value(run[4 * k + 1], cutoff) << 8) |
                       (evseq_md_value(run[4 * k + 2], cutoff) << 16) | (evseq_md_value(run[4 * k + 3], cutoff) << 24);
            }
            *reinterpret_cast<u32x4*>(dst + (size_t)b * plane + i) = o;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 32) {
        const size_t body_end = head + 16 * nvec;
        const size_t i = threadIdx.x < 16 ? (size_t)threadIdx.x : body_end + (threadIdx.x - 16);
        const size_t lim = threadIdx.x < 16 ? head : plane;
        if (i < lim) evseq_md_pixel(img, dst, i, plane, bins, cutoff);
    }
}

}  // namespace rvt
