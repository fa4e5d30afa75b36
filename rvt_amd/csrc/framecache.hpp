// Sparse frame cache: a lossless codec for byte planes that are mostly zero (event histograms, mixed-density stacks).  The device
// counterpart of the reference's compressed pre-processed store (data/genx_utils/sequence_base.py:92-102 reads blosc/zstd H5).
//
// Format, version 1 (include/rvt_hip.h restates it for a host).  A frame is E bytes; a group is 64 consecutive bytes of a frame,
// Gf = ceil(E / 64); a segment is 64 consecutive groups (4096 bytes), Sf = ceil(Gf / 64).
//   masks      uint64 [F][Gf]     bit i of group g set iff byte 64 g + i of the frame exists and is non-zero
//   seg_offset uint32 [F][Sf + 1] exclusive prefix sum of the segments' non-zero counts of the frame; the last entry is the frame's count
//   value_base int64  [F + 1]     exclusive prefix sum of the frames' counts; value_base[F] = nnz
//   values     uint8  [capacity]  the non-zero bytes, frame order then byte order, no padding
//   status     int32  [1]         bit 0: pack ran out of capacity (written by pack);  bit 1: unpack met an index outside [-1, F) (or-ed in);
//                                 bit 2: gather met a table row whose count is outside [0, E] (frames_gather.hpp, which writes bits 0 and 2)
//
// One wave owns one segment, in every kernel; a workgroup is four such waves that share nothing.  No workgroup waits for another:
// the launches of a pack follow each other on the stream, which is the only ordering used.
//   pack    launch 1 (mask):    the segment's 4096 bytes as four 16-byte lines per lane, lane-consecutive (one instruction = 1 KiB);
//                               the 16 non-zero bits of a line are one ushort of a 512-byte LDS image in which they fall into place
//                               (line (j, lane) -> ushort 64 j + lane), read back as one uint64 per lane = group `lane`: one
//                               coalesced 512-byte store.  The wave's count goes to the workspace.
//           launch 2 (segments): per frame, exclusive scan of the counts -> seg_offset, the frame's total to the workspace
//           launch 3 (frames):   exclusive scan of the totals -> value_base, and status
//           launch 4 (compact):  the segment again, the lines' counts scanned in byte order (two shuffle scans of packed 16-bit
//                               counts), the non-zero bytes into a 4-KiB LDS image that starts at the run's own alignment within a
//                               16-byte line, so that whole lines of the image are whole aligned lines of `values`.  Neighbouring
//                               runs meet at arbitrary byte addresses: the bytes of a line the run owns only in part leave by byte
//                               stores, never by read-modify-write.  Bytes at or behind `capacity` are not written.
//   unpack  one launch:         wave = (output frame, segment).  64 masks in one load, popcount, wave scan; masks and prefix counts
//                               parked in LDS with a zero group on either side; the value run staged through LDS by aligned lines
//                               (byte loads, clamped to values_len, where a line leaves the array).  Output lines are the 16-byte
//                               lines of the OUTPUT address: a lane takes line L, reads the 16 mask bits under it (they may straddle
//                               two groups when the frame does not start on a line), their prefix count, and rebuilds the line from
//                               the staged values; whole lines leave as one 16-byte store, the (at most two) lines a segment shares
//                               with its neighbours by byte stores.  A segment without values reads none and stores zeros.
// Format version 2 (capi_frames2.hip: a mask only for the non-empty groups) is these kernels with a second mask level; it calls the
// pieces below (fc_line_load / fc_line_store, the scans, fc_compact_lines, fc_unpack_parked).  The kernels are static: two parts of
// the library include this file.
// A frame of a pack's input that does not start on a 16-byte boundary (E % 16 != 0) is read byte by byte; every shape the package
// builds (20 x 360 x 640, 20 x 240 x 304, 10 x 240 x 304) is a multiple of 16.
#pragma once
#include "common.hpp"

namespace rvt {

constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / 64;                      // segments per workgroup
constexpr int FC_GROUP = 64;                                   // bytes under one mask word
constexpr int FC_SEG = 64 * FC_GROUP;                          // bytes of one segment
constexpr int FC_STATUS_CAPACITY = RVT_FRAMES_STATUS_CAPACITY, FC_STATUS_INDEX = RVT_FRAMES_STATUS_INDEX,
              FC_STATUS_COUNT = RVT_FRAMES_STATUS_COUNT;     // the bits of status (include/rvt_hip.h)

__device__ __forceinline__ void fc_status_or(int* status, int bits) {
#ifdef RVT_EMU
    *status |= bits;
#else
    atomicOr(status, bits);
#endif
}

// inclusive sum over the lanes of the wave
__device__ __forceinline__ int fc_wave_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl(v, (lane - d) & 63);
        if (lane >= d) v += up;
    }
    return v;
}
__device__ __forceinline__ long long fc_wave_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned lo = (unsigned)__shfl((int)(unsigned)((unsigned long long)v & 0xffffffffULL), (lane - d) & 63);
        const unsigned hi = (unsigned)__shfl((int)(unsigned)((unsigned long long)v >> 32), (lane - d) & 63);
        if (lane >= d) v += (long long)(((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// bit k set iff byte k of the line is non-zero
__device__ __forceinline__ unsigned fc_nonzero16(const u32x4& v) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) m |= ((v[k >> 2] >> (8 * (k & 3))) & 0xffu) ? 1u << k : 0u;
    return m;
}
// byte k (0..15, not known at compile time) of the line: selects, no indexed register array
__device__ __forceinline__ unsigned fc_byte_of(const u32x4& v, int k) {
    const unsigned w = k < 8 ? (k < 4 ? v[0] : v[1]) : (k < 12 ? v[2] : v[3]);
    return (w >> (8 * (k & 3))) & 0xffu;
}

// The 16-byte line [lo, lo + 16) behind `base` (base + lo is 16-byte aligned) of a run that owns the bytes [b, e) behind `base`: a
// line inside the run is one 16-byte access, the run's first and last line move byte by byte inside the run, and nothing outside
// the run is touched (bytes not loaded read as zero; edges are stored by byte stores, never by read-modify-write).  aligned = false:
// base + lo is not aligned (a frame of a pack's input with E % 16 != 0), and every line moves byte by byte.
template <typename I>
__device__ __forceinline__ u32x4 fc_line_load(const unsigned char* __restrict__ base, I lo, I b, I e, bool aligned = true) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (aligned && lo >= b && lo + 16 <= e) {
        v = *reinterpret_cast<const u32x4*>(base + lo);
    } else if (lo + 16 > b && lo < e) {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (lo + k >= b && lo + k < e) v[k >> 2] |= (unsigned)base[lo + k] << (8 * (k & 3));
    }
    return v;
}
template <typename I>
__device__ __forceinline__ void fc_line_store(unsigned char* __restrict__ base, I lo, I b, I e, const u32x4& v) {
    if (lo >= b && lo + 16 <= e) {
        *reinterpret_cast<u32x4*>(base + lo) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (lo + k >= b && lo + k < e) base[lo + k] = (unsigned char)((v[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
}

// Exclusive sum over the workgroup of one tile of a longer sequence (a value per thread, int or long long): returns what lies in
// front of this thread's value, `run` = the total of the tiles in front, advanced by this tile's.  part: LDS, one row per parity of
// the tile number (the other parity is free: its readers passed this tile's barrier a tile ago).  Every thread calls it.
template <typename V>
__device__ __forceinline__ V fc_block_scan(V v, V& run, V (*part)[FC_WAVES], int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const V inc = fc_wave_scan(v, lane);
    if (lane == 63) part[par][wave] = inc;
    __syncthreads();
    V pre = run + inc - v;
#pragma unroll
    for (int q = 0; q < FC_WAVES; q++) {
        const V t = part[par][q];
        if (q < wave) pre += t;
        run += t;
    }
    return pre;
}

// Parks segment s of a frame for a wave's decode: the 64 masks (fmask = the frame's Gf masks; the bits behind the frame's end E
// cleared, groups behind it zero) to mg[0..63] and the count of values in front of each group within the segment to pg[0..63],
// both in LDS.  Returns the segment's count.  The caller keeps the wave's earlier readers of mg / pg away and calls
// wave_rendezvous() before the first read.
__device__ __forceinline__ int fc_park_segment(const unsigned long long* __restrict__ fmask, long long s, long long E, long long Gf,
                                               unsigned long long* mg, int* pg, int lane) {
    const long long g = s * 64 + lane;
    unsigned long long m = 0;
    if (g < Gf) {
        m = fmask[g];
        const long long nb = E - 64 * g;                        // bytes of the group that exist
        if (nb < 64) m &= (1ULL << nb) - 1;
    }
    const int c = __builtin_popcountll(m);
    const int inc = fc_wave_scan(c, lane);
    mg[lane] = m;
    pg[lane] = inc - c;
    return __shfl(inc, 63);
}

// -------------------------------------------------------------------------------------------------- pack, launch 1: masks + counts
static __global__ void __launch_bounds__(FC_THREADS)
frames_mask_kernel(const unsigned char* __restrict__ frames, long long F, long long E, long long Gf, long long Sf,
                   unsigned long long* __restrict__ masks, unsigned* __restrict__ seg_count) {
    __shared__ __attribute__((aligned(16))) unsigned short bits[FC_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * FC_WAVES + wave;
    if (w >= F * Sf) return;                                    // (the whole wave)
    const long long f = w / Sf, s = w - f * Sf;
    const unsigned char* __restrict__ frame = frames + f * E;
    const bool aligned = ((uintptr_t)frame & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32x4 v = fc_line_load(frame, (unsigned long long)(s * FC_SEG + j * 1024 + lane * 16), 0ULL, (unsigned long long)E, aligned);
        bits[wave][j * 64 + lane] = (unsigned short)fc_nonzero16(v);
    }
    wave_rendezvous();
    const unsigned long long m = *reinterpret_cast<const unsigned long long*>(&bits[wave][lane * 4]);
    const long long g = s * 64 + lane;
    if (g < Gf) masks[f * Gf + g] = m;
    int c = __builtin_popcountll(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) seg_count[w] = (unsigned)c;
}

// ------------------------------------------------------------------------------------------ pack, launch 2: seg_offset of each frame
// grid F: seg_offset[f][0..Sf] = exclusive scan of seg_count[f][0..Sf), frame_count[f] = the total
static __global__ void __launch_bounds__(FC_THREADS)
frames_seg_scan_kernel(const unsigned* __restrict__ seg_count, long long Sf, unsigned* __restrict__ seg_offset,
                       unsigned* __restrict__ frame_count) {
    __shared__ int part[2][FC_WAVES];
    const long long f = blockIdx.x;
    const unsigned* __restrict__ src = seg_count + f * Sf;
    unsigned* __restrict__ dst = seg_offset + f * (Sf + 1);
    int run = 0, par = 0;                                       // (a frame holds fewer than 2^31 bytes)
    for (long long base = 0; base < Sf; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        const int pre = fc_block_scan(i < Sf ? (int)src[i] : 0, run, part, par);
        if (i < Sf) dst[i] = (unsigned)pre;
    }
    if (threadIdx.x == 0) {
        dst[Sf] = (unsigned)run;
        frame_count[f] = (unsigned)run;
    }
}

// --------------------------------------------------------------------------------------------- pack, launch 3: value_base and status
// one workgroup: value_base[0..F] = exclusive scan of frame_count[0..F); status = nnz > capacity
static __global__ void __launch_bounds__(FC_THREADS)
frames_base_scan_kernel(const unsigned* __restrict__ frame_count, long long F, long long capacity, long long* __restrict__ value_base,
                        int* __restrict__ status) {
    __shared__ long long part[2][FC_WAVES];
    long long run = 0;
    int par = 0;
    for (long long base = 0; base < F; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        const long long pre = fc_block_scan(i < F ? (long long)frame_count[i] : 0LL, run, part, par);
        if (i < F) value_base[i] = pre;
    }
    if (threadIdx.x == 0) {
        value_base[F] = run;
        *status = run > capacity ? FC_STATUS_CAPACITY : 0;
    }
}

// The non-zero bytes of a segment held as four lines per lane, lane-consecutive (v, and m = fc_nonzero16 of each), to the n_fit
// bytes behind dst, through the wave's LDS image img (FC_SEG + 16 bytes): the image starts at the run's own alignment within a
// 16-byte line, whole lines leave as aligned 16-byte stores and the run's edges by byte stores.  Every lane of the wave calls it.
__device__ __forceinline__ void fc_compact_lines(const u32x4 (&v)[4], const unsigned (&m)[4], unsigned char* __restrict__ dst, int n_fit,
                                                 unsigned char* img, int lane) {
    // where each line's bytes go: byte order is (j, lane), so four exclusive scans over the lanes, two 16-bit counts per scan
    // (a wave's sum of one j is at most 1024: the low half never carries into the high one)
    const int p0 = __builtin_popcount(m[0]) | (__builtin_popcount(m[1]) << 16);
    const int p1 = __builtin_popcount(m[2]) | (__builtin_popcount(m[3]) << 16);
    const int i0 = fc_wave_scan(p0, lane), i1 = fc_wave_scan(p1, lane);
    const int t0 = __shfl(i0, 63), t1 = __shfl(i1, 63);
    const int e0 = i0 - p0, e1 = i1 - p1;
    int pos[4];
    pos[0] = e0 & 0xffff;
    pos[1] = (t0 & 0xffff) + (e0 >> 16);
    pos[2] = (t0 & 0xffff) + (t0 >> 16) + (e1 & 0xffff);
    pos[3] = (t0 & 0xffff) + (t0 >> 16) + (t1 & 0xffff) + (e1 >> 16);

    const int a = (int)((uintptr_t)dst & 15);                   // the image starts where the run starts within its line
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int q = a + pos[j];
        unsigned mm = m[j];
        while (mm) {
            const int k = __builtin_ctz(mm);
            mm &= mm - 1;
            img[q++] = (unsigned char)fc_byte_of(v[j], k);
        }
    }
    wave_rendezvous();
    unsigned char* line0 = dst - a;
    const int end = a + n_fit, nlines = (end + 15) >> 4;
    for (int L = lane; L < nlines; L += 64) fc_line_store(line0, 16 * L, a, end, *reinterpret_cast<const u32x4*>(img + 16 * L));
}

// Decode of a parked segment (fc_park_segment's 64 masks and prefix counts at mg[1..64] / pg[1..64], a zero group on either side,
// pg[65] = total): the run of `total` values of segment s of packed frame idx staged through img (FC_SEG + 32 bytes of LDS) by
// aligned lines, reads clamped to [0, values_len), then the len bytes at o rebuilt line by line of the OUTPUT address: whole
// lines by one 16-byte store, the segment's edges by byte stores.  total == 0: nothing is read (idx may name no frame) and zeros
// are stored.  Every lane of the wave calls it.
__device__ __forceinline__ void fc_unpack_parked(int total, const long long* __restrict__ value_base, const unsigned* __restrict__ seg_offset,
                                                 long long idx, long long Sf, long long s, const unsigned char* __restrict__ values,
                                                 long long values_len, unsigned char* img, const unsigned long long* mg, const int* pg,
                                                 unsigned char* __restrict__ o, int len, int lane) {
    int av = 0;
    if (total > 0) {                                            // (the same in every lane)
        const long long start = value_base[idx] + (long long)seg_offset[idx * (Sf + 1) + s];
        av = (int)(((uintptr_t)values + (uintptr_t)start) & 15);
        const long long first = start - av;                     // index into values of the image's byte 0
        const int nl = (av + total + 15) >> 4;
        for (int L = lane; L < nl; L += 64)                     // (lines of the ADDRESS values + first; the array is the run [0, values_len))
            *reinterpret_cast<u32x4*>(img + 16 * L) = fc_line_load(values, first + 16 * L, 0LL, values_len);
    }
    wave_rendezvous();

    const int a = (int)((uintptr_t)o & 15);
    unsigned char* line0 = o - a;
    const int nlines = (a + len + 15) >> 4;
    for (int L = lane; L < nlines; L += 64) {
        const int r0 = 16 * L - a;                              // segment byte under the line's byte 0 (negative: the neighbour's)
        const int bit = r0 + 64, gi = bit >> 6, bo = bit & 63;
        const unsigned long long lo = mg[gi], hi = mg[gi + 1];
        unsigned mm = (unsigned)((bo ? (lo >> bo) | (hi << (64 - bo)) : lo) & 0xffffULL);
        int off = av + pg[gi] + __builtin_popcountll(lo & ((1ULL << bo) - 1));
        unsigned q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        while (mm) {
            const int k = __builtin_ctz(mm);
            mm &= mm - 1;
            const unsigned b = (unsigned)img[off++] << (8 * (k & 3));
            const int wd = k >> 2;
            q0 |= wd == 0 ? b : 0u; q1 |= wd == 1 ? b : 0u; q2 |= wd == 2 ? b : 0u; q3 |= wd == 3 ? b : 0u;
        }
        const u32x4 q = {q0, q1, q2, q3};
        fc_line_store(line0, 16 * L, a, a + len, q);
    }
}

// ------------------------------------------------------------------------------------------------ pack, launch 4: value compaction
static __global__ void __launch_bounds__(FC_THREADS)
frames_compact_kernel(const unsigned char* __restrict__ frames, long long F, long long E, long long Sf,
                      const unsigned* __restrict__ seg_offset, const long long* __restrict__ value_base,
                      unsigned char* __restrict__ values, long long capacity) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[FC_WAVES][FC_SEG + 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * FC_WAVES + wave;
    if (w >= F * Sf) return;
    const long long f = w / Sf, s = w - f * Sf;
    const long long start = value_base[f] + (long long)seg_offset[f * (Sf + 1) + s];
    const int n = (int)(seg_offset[f * (Sf + 1) + s + 1] - seg_offset[f * (Sf + 1) + s]);
    const long long room = capacity - start;
    const int n_fit = room <= 0 ? 0 : (room < n ? (int)room : n);   // bytes of the run that `values` has room for
    if (n_fit == 0) return;                                     // (the same in every lane)

    const unsigned char* __restrict__ frame = frames + f * E;
    const bool aligned = ((uintptr_t)frame & 15) == 0;
    u32x4 v[4];
    unsigned m[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = fc_line_load(frame, (unsigned long long)(s * FC_SEG + j * 1024 + lane * 16), 0ULL, (unsigned long long)E, aligned);
        m[j] = fc_nonzero16(v[j]);
    }
    fc_compact_lines(v, m, values + start, n_fit, stage[wave], lane);
}

// -------------------------------------------------------------------------------------------------------------------------- unpack
static __global__ void __launch_bounds__(FC_THREADS)
frames_unpack_kernel(const unsigned long long* __restrict__ masks, const unsigned* __restrict__ seg_offset,
                     const long long* __restrict__ value_base, const unsigned char* __restrict__ values, long long values_len,
                     long long F, long long E, long long Gf, long long Sf, const long long* __restrict__ index, long long Fout,
                     unsigned char* __restrict__ out, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) unsigned char vstage[FC_WAVES][FC_SEG + 32];
    __shared__ unsigned long long mgrp[FC_WAVES][66];           // [0] and [65]: a zero group on either side
    __shared__ int pgrp[FC_WAVES][66];                          // values in front of group g - 1 within the segment
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * FC_WAVES + wave;
    if (w >= Fout * Sf) return;
    const long long fo = w / Sf, s = w - fo * Sf;
    const long long idx = index ? index[fo] : fo;
    const bool present = idx >= 0 && idx < F;
    if (!present && idx != -1 && s == 0 && lane == 0) fc_status_or(status, FC_STATUS_INDEX);
    const long long left = E - s * FC_SEG;
    const int len = left < FC_SEG ? (int)left : FC_SEG;         // bytes of this segment

    // (a frame that is not there has no groups: all masks zero)
    const int total = fc_park_segment(masks + (present ? idx : 0) * Gf, s, E, present ? Gf : 0, &mgrp[wave][1], &pgrp[wave][1], lane);
    if (lane == 0) {
        mgrp[wave][0] = 0; pgrp[wave][0] = 0;
        mgrp[wave][65] = 0; pgrp[wave][65] = total;
    }

    fc_unpack_parked(total, value_base, seg_offset, idx, Sf, s, values, values_len, vstage[wave], mgrp[wave], pgrp[wave],
                     out + fo * E + s * FC_SEG, len, lane);
}

}  // namespace rvt
