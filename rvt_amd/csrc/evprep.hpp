// What comes before the event stream: the reference reader's timestamp repair (scripts/genx/preprocess_dataset.py:163-172,
// H5Reader._correct_time) and the decode of packed Prophesee Event2D records (utils/evaluation/prophesee/io/dat_events_tools.py:
// 41-50, load_td_data) into the compact x, y, p, t arrays the sequence builder takes (evseq.hpp).
//
//   repair:  t_out[i] = max(c, t[0], ..., t[i]), c the carry-in (0 without one: the reference starts time_last at 0).  A running
//            maximum, i.e. an inclusive scan with max, over 64-bit values.
//   decode:  record = {uint32 t; int32 w}:  x = w & 16383, y = (w >> 14) & 16383, p = (w >> 28) & 1, t zero-extended.
//
// One skeleton, two launches on the caller's stream, grid (blocks per stream, B).  The grid cannot follow n, which lives on
// the device, so workgroup k owns the k-th of K equal contiguous spans of its stream (a multiple of 8 events long: every
// span starts on the 8-event grid of the 16-byte accesses).  No workgroup waits for another one: the second launch starts
// behind the first, which is the only ordering used.
//   reduce (launch 1): span -> its maximum, ws[b][k]; workgroup 0 also parks the carry-in in ws[b][K].  carry[] is read here only.
//   scan   (launch 2): prefix = max(carry-in, ws[b][0..k-1]), then the span tile by tile (EVPREP_TILE events: 8 consecutive ones
//            per lane): serial scan in the lane, wave scan with shuffles, the four wave totals through LDS, and a running
//            maximum from tile to tile.  The repair entry stores only the timestamps that changed; the decode entry stores
//            everything, the records being read in both launches and the stream written once.  The last workgroup writes carry[b];
//            carry[] is written here only.
// Timestamps are compared as 64-bit values throughout; a 64-bit shuffle is two 32-bit ones.
//
// Accesses are 16 bytes wide for whole groups of 8 events when the base pointer is 16-byte aligned (source and destinations
// decided separately), element by element otherwise and for the last, partial group of a stream.
#pragma once
#include "evseq.hpp"

namespace rvt {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

constexpr int EVPREP_THREADS = 256;
constexpr int EVPREP_PER = 8;                                  // consecutive events of one lane
constexpr int EVPREP_TILE = EVPREP_THREADS * EVPREP_PER;       // 2048 events
constexpr int EVPREP_WAVES = EVPREP_THREADS / 64;
constexpr int EVPREP_MAX_BLOCKS = 4096;                        // workgroups per stream
constexpr int EVPREP_REPAIR = 0, EVPREP_DECODE = 1;            // where a timestamp comes from
constexpr long long EVPREP_LOWEST = -0x7fffffffffffffffLL - 1; // identity of max

__device__ __forceinline__ long long evprep_max(long long a, long long b) { return a > b ? a : b; }

__device__ __forceinline__ long long evprep_join(int lo, int hi) {
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ long long evprep_shfl(long long v, int src) {
    const int lo = __shfl((int)(unsigned)((unsigned long long)v & 0xffffffffULL), src);
    const int hi = __shfl((int)(unsigned)((unsigned long long)v >> 32), src);
    return evprep_join(lo, hi);
}
__device__ __forceinline__ long long evprep_shfl_xor(long long v, int mask) {
    const int lo = __shfl_xor((int)(unsigned)((unsigned long long)v & 0xffffffffULL), mask);
    const int hi = __shfl_xor((int)(unsigned)((unsigned long long)v >> 32), mask);
    return evprep_join(lo, hi);
}

// maximum (or sum) over the workgroup, in every thread.  Every thread of the workgroup calls it.
template <bool SUM> __device__ __forceinline__ long long evprep_block_fold(long long v) {
    __shared__ long long part[EVPREP_WAVES];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = evprep_shfl_xor(v, d);
        v = SUM ? v + o : evprep_max(v, o);
    }
    __syncthreads();                                           // an earlier call's readers are done with `part`
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = part[0];
#pragma unroll
    for (int w = 1; w < EVPREP_WAVES; w++) r = SUM ? r + part[w] : evprep_max(r, part[w]);
    return r;
}

// events of stream b: the table's n (repair) or min(n_records[b], capacity) (decode), never negative
template <int MODE>
__device__ __forceinline__ long long evprep_count(const EvStream& s, const long long* __restrict__ n_records, long long capacity, int b) {
    long long n = s.n;
    if constexpr (MODE == EVPREP_DECODE) {
        n = n_records[b];
        n = n < capacity ? n : capacity;
    }
    return n > 0 ? n : 0;
}

// [s0, e0) of workgroup k of K over n events; s0 is a multiple of 8
__device__ __forceinline__ void evprep_span(long long n, int k, int K, long long& s0, long long& e0) {
    long long span = (n + K - 1) / K;
    span = (span + 7) & ~7LL;
    s0 = (long long)k * span;
    s0 = s0 < n ? s0 : n;
    e0 = s0 + span < n ? s0 + span : n;
}

// the lane's 8 events [i, i + 8) clipped to `end`: timestamps (EVPREP_LOWEST behind the end) and, for records, the data words
template <int MODE>
__device__ __forceinline__ void evprep_load(const EVSEQ_GLOBAL void* src, bool vec, long long i, long long end,
                                            long long (&t)[EVPREP_PER], int (&w)[EVPREP_PER]) {
    if constexpr (MODE == EVPREP_REPAIR) {
        const EVSEQ_GLOBAL long long* p = (const EVSEQ_GLOBAL long long*)src;
        if (vec && i + EVPREP_PER <= end) {
#pragma unroll
            for (int k = 0; k < EVPREP_PER / 2; k++) {
                const i64x2 q = *reinterpret_cast<const EVSEQ_GLOBAL i64x2*>(p + i + 2 * k);
                t[2 * k] = q[0]; t[2 * k + 1] = q[1];
            }
        } else {
#pragma unroll
            for (int j = 0; j < EVPREP_PER; j++) t[j] = i + j < end ? p[i + j] : EVPREP_LOWEST;
        }
#pragma unroll
        for (int j = 0; j < EVPREP_PER; j++) w[j] = 0;
    } else {
        const EVSEQ_GLOBAL unsigned* p = (const EVSEQ_GLOBAL unsigned*)src;
        if (vec && i + EVPREP_PER <= end) {
#pragma unroll
            for (int k = 0; k < EVPREP_PER / 2; k++) {
                const u32x4 q = *reinterpret_cast<const EVSEQ_GLOBAL u32x4*>(p + 2 * (i + 2 * k));
                t[2 * k] = (long long)q[0]; w[2 * k] = (int)q[1];
                t[2 * k + 1] = (long long)q[2]; w[2 * k + 1] = (int)q[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < EVPREP_PER; j++) {
                t[j] = EVPREP_LOWEST; w[j] = 0;
                if (i + j < end) {
                    const u32x2 q = *reinterpret_cast<const EVSEQ_GLOBAL u32x2*>(p + 2 * (i + j));
                    t[j] = (long long)q[0]; w[j] = (int)q[1];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ launch 1: reduce
// grid (K, B): ws[b][k] = maximum timestamp of span k (EVPREP_LOWEST for an empty span); ws[b][K] = the carry-in
template <int MODE> __global__ void __launch_bounds__(EVPREP_THREADS)
evprep_reduce_kernel(const EvStream* __restrict__ table, const void* const* __restrict__ records, const long long* __restrict__ n_records,
                     long long capacity, const long long* __restrict__ carry, long long* __restrict__ ws) {
    const int b = blockIdx.y, k = blockIdx.x, K = gridDim.x;
    const EvStream s = table[b];
    const long long n = evprep_count<MODE>(s, n_records, capacity, b);
    const void* base = MODE == EVPREP_DECODE ? records[b] : (const void*)s.t;
    const bool vec = ((uintptr_t)base & 15) == 0;
    const EVSEQ_GLOBAL void* __restrict__ src = (const EVSEQ_GLOBAL void*)base;
    long long s0, e0;
    evprep_span(n, k, K, s0, e0);
    long long* __restrict__ row = ws + (size_t)b * (K + 1);
    if (s0 >= e0 && k > 0) {                                    // more workgroups than spans: nothing to reduce (same for every thread)
        if (threadIdx.x == 0) row[k] = EVPREP_LOWEST;
        return;
    }
    long long m = EVPREP_LOWEST;
    for (long long i = s0 + (long long)threadIdx.x * EVPREP_PER; i < e0; i += EVPREP_TILE) {
        long long t[EVPREP_PER];
        int w[EVPREP_PER];
        evprep_load<MODE>(src, vec, i, e0, t, w);
#pragma unroll
        for (int j = 0; j < EVPREP_PER; j++) m = evprep_max(m, t[j]);
    }
    m = evprep_block_fold<false>(m);
    if (threadIdx.x == 0) {
        row[k] = m;
        if (k == 0) row[K] = carry ? carry[b] : 0;
    }
}

// -------------------------------------------------------------------------------------------------------- launch 2: scan
template <class CT>
__device__ __forceinline__ void evprep_store_coord(EVSEQ_GLOBAL CT* __restrict__ dst, bool vec, long long i, long long end,
                                                   const int (&v)[EVPREP_PER]) {
    if (vec && i + EVPREP_PER <= end) {
        constexpr int PER = 16 / (int)sizeof(CT);
        typedef CT vec_t __attribute__((ext_vector_type(PER)));
#pragma unroll
        for (int k = 0; k < EVPREP_PER / PER; k++) {
            vec_t q;
#pragma unroll
            for (int j = 0; j < PER; j++) q[j] = (CT)v[k * PER + j];
            *reinterpret_cast<EVSEQ_GLOBAL vec_t*>(dst + i + k * PER) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EVPREP_PER; j++)
            if (i + j < end) dst[i + j] = (CT)v[j];
    }
}

// grid (K, B).  repair == 0 (decode entry only): the timestamps go out as decoded, ws and carry are not touched.
template <int MODE, class CT> __global__ void __launch_bounds__(EVPREP_THREADS)
evprep_scan_kernel(EvStream* __restrict__ table, const void* const* __restrict__ records, const long long* __restrict__ n_records,
                   long long capacity, int repair, long long* __restrict__ carry, long long* __restrict__ repaired,
                   const long long* __restrict__ ws) {
    __shared__ long long totals[2][EVPREP_WAVES];
    const int b = blockIdx.y, k = blockIdx.x, K = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const EvStream s = table[b];
    const long long n = evprep_count<MODE>(s, n_records, capacity, b);
    const void* base = MODE == EVPREP_DECODE ? records[b] : (const void*)s.t;
    const bool vin = ((uintptr_t)base & 15) == 0;
    const bool vout = ((((uintptr_t)s.x) | ((uintptr_t)s.y) | ((uintptr_t)s.p) | ((uintptr_t)s.t)) & 15) == 0;
    const EVSEQ_GLOBAL void* src = (const EVSEQ_GLOBAL void*)base;           // (the repair entry stores into what it loads from)
    EVSEQ_GLOBAL long long* tp = (EVSEQ_GLOBAL long long*)s.t;
    long long s0, e0;
    evprep_span(n, k, K, s0, e0);

    if (s0 >= e0 && k > 0 && k < K - 1) {                       // an empty span that owes neither n nor the carry (same for every thread)
        if (repaired && threadIdx.x == 0) repaired[(size_t)b * K + k] = 0;
        return;
    }

    long long run = EVPREP_LOWEST;                              // max(carry-in, everything in front of the tile), same in every thread
    if (repair) {
        const long long* __restrict__ row = ws + (size_t)b * (K + 1);
        long long m = EVPREP_LOWEST;
        for (int j = threadIdx.x; j < k; j += EVPREP_THREADS) m = evprep_max(m, row[j]);
        run = evprep_max(evprep_block_fold<false>(m), row[K]);
    }

    long long changed = 0;
    int par = 0;
    for (long long tile = s0; tile < e0; tile += EVPREP_TILE, par ^= 1) {
        const long long i = tile + (long long)threadIdx.x * EVPREP_PER;
        long long t[EVPREP_PER], o[EVPREP_PER];
        int w[EVPREP_PER];
        evprep_load<MODE>(src, vin, i, e0, t, w);
#pragma unroll
        for (int j = 0; j < EVPREP_PER; j++) o[j] = t[j];
        if (repair) {
#pragma unroll
            for (int j = 1; j < EVPREP_PER; j++) o[j] = evprep_max(o[j], o[j - 1]);
            long long inc = o[EVPREP_PER - 1];                  // inclusive over the lanes of the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long up = evprep_shfl(inc, (lane - d) & 63);
                if (lane >= d) inc = evprep_max(inc, up);
            }
            long long pre = evprep_shfl(inc, (lane - 1) & 63);  // exclusive
            if (lane == 0) pre = EVPREP_LOWEST;
            if (lane == 63) totals[par][wave] = inc;
            __syncthreads();                                    // (the other parity is free: its readers passed this barrier a tile ago)
            pre = evprep_max(pre, run);
#pragma unroll
            for (int v = 0; v < EVPREP_WAVES; v++) {
                const long long tv = totals[par][v];
                if (v < wave) pre = evprep_max(pre, tv);
                run = evprep_max(run, tv);
            }
#pragma unroll
            for (int j = 0; j < EVPREP_PER; j++) {
                o[j] = evprep_max(o[j], pre);
                changed += (i + j < e0 && o[j] != t[j]) ? 1 : 0;
            }
        }
        if constexpr (MODE == EVPREP_REPAIR) {
#pragma unroll
            for (int j = 0; j < EVPREP_PER; j++)
                if (i + j < e0 && o[j] != t[j]) tp[i + j] = o[j];
        } else {
            int xv[EVPREP_PER], yv[EVPREP_PER], pv[EVPREP_PER];
#pragma unroll
            for (int j = 0; j < EVPREP_PER; j++) {
                xv[j] = w[j] & 16383;
                yv[j] = (w[j] >> 14) & 16383;
                pv[j] = (w[j] >> 28) & 1;
            }
            evprep_store_coord<CT>((EVSEQ_GLOBAL CT*)s.x, vout, i, e0, xv);
            evprep_store_coord<CT>((EVSEQ_GLOBAL CT*)s.y, vout, i, e0, yv);
            evprep_store_coord<CT>((EVSEQ_GLOBAL CT*)s.p, vout, i, e0, pv);
            if (vout && i + EVPREP_PER <= e0) {
#pragma unroll
                for (int q = 0; q < EVPREP_PER / 2; q++)
                    *reinterpret_cast<EVSEQ_GLOBAL i64x2*>(tp + i + 2 * q) = i64x2{o[2 * q], o[2 * q + 1]};
            } else {
#pragma unroll
                for (int j = 0; j < EVPREP_PER; j++)
                    if (i + j < e0) tp[i + j] = o[j];
            }
        }
    }

    if (repaired) {                                             // this workgroup's own slot: written, never accumulated
        const long long c = evprep_block_fold<true>(changed);
        if (threadIdx.x == 0) repaired[(size_t)b * K + k] = c;
    }
    if (threadIdx.x == 0) {
        if (repair && carry && k == K - 1) carry[b] = run;      // max(carry-in, every timestamp of the stream)
        if (MODE == EVPREP_DECODE && k == 0) table[b].n = n;
    }
}

}  // namespace rvt
