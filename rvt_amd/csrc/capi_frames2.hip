// extern "C" entry points, part 18: the sparse frame cache, format version 2 (include/rvt_hip.h): a mask word is kept only for the
// 64-byte groups that hold a non-zero byte.  The kernels live in this file (they are version 1's with a second mask level) and
// reuse framecache.hpp's pieces (fc_line_load / fc_line_store, the wave and block scans, fc_compact_lines, fc_unpack_parked) and
// frames_gather.hpp's copies (ga_copy_items, ga_copy_bytes).  Integer work: bit-exact.
//
// Format, version 2.  Geometry as in version 1: a frame is E bytes; a group is 64 consecutive bytes of a frame, Gf = ceil(E / 64); a
// segment is 64 consecutive groups (4096 bytes), Sf = ceil(Gf / 64).
//   group_mask uint64 [F][Sf]         bit g of segment s set iff group 64 s + g exists and holds a non-zero byte
//   seg_offset uint32 [F][Sf + 1]     unchanged: exclusive prefix sum of the segments' non-zero byte counts; last entry = the frame's count
//   grp_offset uint32 [F][Sf + 1]     exclusive prefix sum of popcount(group_mask[f][s]); last entry = the frame's count of non-empty groups
//   value_base int64  [F + 1]         unchanged
//   mask_base  int64  [F + 1]         exclusive prefix sum of the frames' non-empty group counts; mask_base[F] = ngroups
//   masks      uint64 [mask_capacity] version 1's mask of each NON-EMPTY group, frame order then group order, no padding; bits behind E
//                                     are zero; no stored word is zero
//   values     uint8  [capacity]      unchanged
//   status     int32  [1]             the version-1 bits; bit 0: nnz > capacity or ngroups > mask_capacity
// The mask of group g (segment s, bit j): masks[mask_base[f] + grp_offset[f][s] + popcount(group_mask[f][s] & ((1 << j) - 1))] when
// bit j of group_mask[f][s] is set, else 0.
//
// One wave owns one segment, so lane = group: the second level is one ballot (pack) or one popcount under the lane (unpack).
//   pack    launch 1 (mask):     version 1's mask launch; instead of the 64 masks the wave stores their ballot `mask != 0`, and leaves
//                                the segment's byte count and group count in the workspace
//           launch 2 (segments): per frame, both exclusive scans -> seg_offset, grp_offset, the frame's two totals to the workspace
//           launch 3 (frames):   both exclusive scans of the totals -> value_base, mask_base, and status
//           launch 4 (compact):  the segment again; the group masks are RECOMPUTED from the bytes this launch reloads anyway (one more
//                                trip through the 512-byte LDS bit image) instead of being kept in a workspace of 8 Gf F bytes, which
//                                would write and read back exactly the traffic the format removes.  A non-empty group's mask goes to
//                                its slot by one aligned 8-byte store, nothing at or behind mask_capacity; the values as in version 1.
//   unpack  one launch:          wave = (output frame, segment).  Lane j reads its mask through the rule above (index clamped to
//                                [0, masks_len)) or takes 0; everything behind is version 1's (fc_unpack_parked).  A segment whose
//                                group_mask word is 0 loads no mask and no value and stores zeros.
//   gather  scan + copy:         the scan makes value_base and mask_base; the copy walks, wave-stride, the three fixed-size rows of
//                                every frame (aligned item copies), then the value pieces and the mask pieces: both are pieces of
//                                the DESTINATION found by a binary search of their base array; the masks ride the byte-run path as
//                                8 x count bytes.
#include <stdint.h>

#include "host.hpp"
#include "framecache.hpp"
#include "frames_gather.hpp"

namespace rvt {

constexpr int GA2_COLS = RVT_FRAMES_GATHER2_COLS;              // int64 columns of a row of rvt_frames_gather2's table

__device__ __forceinline__ unsigned long long fc_ballot(bool p) {
#ifndef RVT_EMU
    return __ballot(p ? 1 : 0);
#else
    unsigned long long m = p ? 1ull << (threadIdx.x & 63) : 0ull;
    for (int s = 1; s < 64; s <<= 1) m |= __shfl_xor(m, s);
    return m;
#endif
}

// Segment s of a frame as four 16-byte lines per lane, lane-consecutive (v, and nz = their non-zero bits), and, through the wave's
// 512-byte LDS bit image, the mask of group `lane` (zero for a group behind the frame's end).  The caller keeps earlier readers of
// `bits` away.
__device__ __forceinline__ unsigned long long fc2_load_segment(const unsigned char* __restrict__ frame, long long s, long long E,
                                                               unsigned short* bits, int lane, u32x4 (&v)[4], unsigned (&nz)[4]) {
    const bool aligned = ((uintptr_t)frame & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = fc_line_load(frame, (unsigned long long)(s * FC_SEG + j * 1024 + lane * 16), 0ULL, (unsigned long long)E, aligned);
        nz[j] = fc_nonzero16(v[j]);
        bits[j * 64 + lane] = (unsigned short)nz[j];
    }
    wave_rendezvous();
    return *reinterpret_cast<const unsigned long long*>(&bits[lane * 4]);
}

// ------------------------------------------------------------------------------------ pack, launch 1: group_mask + the two counts
__global__ void __launch_bounds__(FC_THREADS)
frames_mask2_kernel(const unsigned char* __restrict__ frames, long long F, long long E, long long Sf,
                    unsigned long long* __restrict__ group_mask, unsigned* __restrict__ seg_count, unsigned* __restrict__ grp_count) {
    __shared__ __attribute__((aligned(16))) unsigned short bits[FC_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * FC_WAVES + wave;
    if (w >= F * Sf) return;                                    // (the whole wave)
    const long long f = w / Sf, s = w - f * Sf;
    u32x4 v[4];
    unsigned nz[4];
    const unsigned long long m = fc2_load_segment(frames + f * E, s, E, bits[wave], lane, v, nz);
    const unsigned long long live = fc_ballot(m != 0);
    int c = __builtin_popcountll(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) {
        group_mask[w] = live;                                   // ([F][Sf]: entry f Sf + s)
        seg_count[w] = (unsigned)c;
        grp_count[w] = (unsigned)__builtin_popcountll(live);
    }
}

// ------------------------------------------------------------------------- pack, launch 2: seg_offset and grp_offset of each frame
// grid F: the two exclusive scans over the frame's segments, the two totals to frame_count[f], frame_groups[f]
__global__ void __launch_bounds__(FC_THREADS)
frames_seg_scan2_kernel(const unsigned* __restrict__ seg_count, const unsigned* __restrict__ grp_count, long long Sf,
                        unsigned* __restrict__ seg_offset, unsigned* __restrict__ grp_offset, unsigned* __restrict__ frame_count,
                        unsigned* __restrict__ frame_groups) {
    __shared__ int part[2][2][FC_WAVES];
    const long long f = blockIdx.x;
    const unsigned* __restrict__ sc = seg_count + f * Sf;
    const unsigned* __restrict__ gc = grp_count + f * Sf;
    unsigned* __restrict__ so = seg_offset + f * (Sf + 1);
    unsigned* __restrict__ go = grp_offset + f * (Sf + 1);
    int run_v = 0, run_g = 0, par = 0;
    for (long long base = 0; base < Sf; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        const int pv = fc_block_scan(i < Sf ? (int)sc[i] : 0, run_v, part[0], par);
        const int pg = fc_block_scan(i < Sf ? (int)gc[i] : 0, run_g, part[1], par);
        if (i < Sf) {
            so[i] = (unsigned)pv;
            go[i] = (unsigned)pg;
        }
    }
    if (threadIdx.x == 0) {
        so[Sf] = (unsigned)run_v;
        go[Sf] = (unsigned)run_g;
        frame_count[f] = (unsigned)run_v;
        frame_groups[f] = (unsigned)run_g;
    }
}

// -------------------------------------------------------------------------- pack, launch 3: value_base, mask_base and status
__global__ void __launch_bounds__(FC_THREADS)
frames_base_scan2_kernel(const unsigned* __restrict__ frame_count, const unsigned* __restrict__ frame_groups, long long F,
                         long long capacity, long long mask_capacity, long long* __restrict__ value_base,
                         long long* __restrict__ mask_base, int* __restrict__ status) {
    __shared__ long long part[2][2][FC_WAVES];
    long long run_v = 0, run_g = 0;
    int par = 0;
    for (long long base = 0; base < F; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        const long long pv = fc_block_scan(i < F ? (long long)frame_count[i] : 0LL, run_v, part[0], par);
        const long long pg = fc_block_scan(i < F ? (long long)frame_groups[i] : 0LL, run_g, part[1], par);
        if (i < F) {
            value_base[i] = pv;
            mask_base[i] = pg;
        }
    }
    if (threadIdx.x == 0) {
        value_base[F] = run_v;
        mask_base[F] = run_g;
        *status = (run_v > capacity || run_g > mask_capacity) ? FC_STATUS_CAPACITY : 0;
    }
}

// ---------------------------------------------------------------------- pack, launch 4: mask compaction and value compaction
__global__ void __launch_bounds__(FC_THREADS)
frames_compact2_kernel(const unsigned char* __restrict__ frames, long long F, long long E, long long Sf,
                       const unsigned* __restrict__ seg_offset, const unsigned* __restrict__ grp_offset,
                       const long long* __restrict__ value_base, const long long* __restrict__ mask_base,
                       unsigned long long* __restrict__ masks, long long mask_capacity, unsigned char* __restrict__ values,
                       long long capacity) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[FC_WAVES][FC_SEG + 16];
    __shared__ __attribute__((aligned(16))) unsigned short bits[FC_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * FC_WAVES + wave;
    if (w >= F * Sf) return;
    const long long f = w / Sf, s = w - f * Sf, row = f * (Sf + 1) + s;
    if (grp_offset[row + 1] == grp_offset[row]) return;         // an empty segment: no mask, no value (the same in every lane)
    const long long start = value_base[f] + (long long)seg_offset[row];
    const int n = (int)(seg_offset[row + 1] - seg_offset[row]);
    const long long room = capacity - start;
    const int n_fit = room <= 0 ? 0 : (room < n ? (int)room : n);   // bytes of the run that `values` has room for
    const long long mstart = mask_base[f] + (long long)grp_offset[row];
    if (n_fit == 0 && mstart >= mask_capacity) return;          // room for neither (the same in every lane)

    u32x4 v[4];
    unsigned nz[4];
    const unsigned long long m = fc2_load_segment(frames + f * E, s, E, bits[wave], lane, v, nz);
    const unsigned long long live = fc_ballot(m != 0);
    if (m != 0) {
        const long long slot = mstart + __builtin_popcountll(live & ((1ULL << lane) - 1));
        if (slot < mask_capacity) masks[slot] = m;
    }
    if (n_fit == 0) return;                                     // (the same in every lane)
    fc_compact_lines(v, nz, values + start, n_fit, stage[wave], lane);
}

// -------------------------------------------------------------------------------------------------------------------------- unpack
// fc_park_segment for version 2: lane j takes the mask of group 64 s + j from its slot behind `first` (the index into masks of the
// segment's first stored mask) when bit j of `live` is set and the slot lies inside [0, masks_len), else 0.
__device__ __forceinline__ int fc_park_segment2(unsigned long long live, const unsigned long long* __restrict__ masks, long long masks_len,
                                                long long first, long long s, long long E, long long Gf, unsigned long long* mg, int* pg,
                                                int lane) {
    const long long g = s * 64 + lane;
    unsigned long long m = 0;
    if (((live >> lane) & 1ULL) && g < Gf) {
        const long long k = first + __builtin_popcountll(live & ((1ULL << lane) - 1));
        if (k >= 0 && k < masks_len) m = masks[k];
        const long long nb = E - 64 * g;                        // bytes of the group that exist
        if (nb < 64) m &= (1ULL << nb) - 1;
    }
    const int c = __builtin_popcountll(m);
    const int inc = fc_wave_scan(c, lane);
    mg[lane] = m;
    pg[lane] = inc - c;
    return __shfl(inc, 63);
}

__global__ void __launch_bounds__(FC_THREADS)
frames_unpack2_kernel(const unsigned long long* __restrict__ group_mask, const unsigned* __restrict__ seg_offset,
                      const unsigned* __restrict__ grp_offset, const long long* __restrict__ value_base,
                      const long long* __restrict__ mask_base, const unsigned long long* __restrict__ masks, long long masks_len,
                      const unsigned char* __restrict__ values, long long values_len, long long F, long long E, long long Gf, long long Sf,
                      const long long* __restrict__ index, long long Fout, unsigned char* __restrict__ out, int* __restrict__ status) {
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

    // (a frame that is not there has no groups; a segment without a live group loads no mask)
    const unsigned long long live = present ? group_mask[idx * Sf + s] : 0ULL;
    int total = 0;
    if (live != 0) {                                            // (the same in every lane)
        const long long first = mask_base[idx] + (long long)grp_offset[idx * (Sf + 1) + s];
        total = fc_park_segment2(live, masks, masks_len, first, s, E, Gf, &mgrp[wave][1], &pgrp[wave][1], lane);
    } else {
        mgrp[wave][1 + lane] = 0;
        pgrp[wave][1 + lane] = 0;
    }
    if (lane == 0) {
        mgrp[wave][0] = 0; pgrp[wave][0] = 0;
        mgrp[wave][65] = 0; pgrp[wave][65] = total;
    }
    fc_unpack_parked(total, value_base, seg_offset, idx, Sf, s, values, values_len, vstage[wave], mgrp[wave], pgrp[wave],
                     out + fo * E + s * FC_SEG, len, lane);
}

// ----------------------------------------------------------------------------- gather, launch 1: value_base, mask_base and status
__global__ void __launch_bounds__(FC_THREADS)
frames_gather2_scan_kernel(const long long* __restrict__ table, long long n, long long E, long long Gf, long long capacity,
                           long long mask_capacity, long long* __restrict__ value_base, long long* __restrict__ mask_base,
                           int* __restrict__ status) {
    __shared__ long long part[2][2][FC_WAVES];
    __shared__ int badw[FC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long run_v = 0, run_g = 0;
    int par = 0, bad = 0;
    for (long long base = 0; base < n; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        long long cv = 0, cg = 0;
        if (i < n) {
            cv = table[i * GA2_COLS + 5];
            cg = table[i * GA2_COLS + 6];
            if (cv < 0 || cv > E) { cv = 0; bad = 1; }
            if (cg < 0 || cg > Gf) { cg = 0; bad = 1; }
        }
        const long long pv = fc_block_scan(cv, run_v, part[0], par);
        const long long pg = fc_block_scan(cg, run_g, part[1], par);
        if (i < n) {
            value_base[i] = pv;
            mask_base[i] = pg;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad |= __shfl_xor(bad, d);
    if (lane == 0) badw[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any = 0;
#pragma unroll
        for (int q = 0; q < FC_WAVES; q++) any |= badw[q];
        value_base[n] = run_v;
        mask_base[n] = run_g;
        *status = ((run_v > capacity || run_g > mask_capacity) ? FC_STATUS_CAPACITY : 0) | (any ? FC_STATUS_COUNT : 0);
    }
}

// ------------------------------------------------------------------------------------------------------------ gather, launch 2: copy
// Piece v of a variable-length run of the destination: the bytes [lo, hi) under the v-th GA_PIECE of aligned lines behind dst (av =
// dst & 15, `fit` bytes are written in all).  Frame f owns the bytes [unit base[f], unit base[f + 1]) and its source address is
// column col of its table row.  The wave finds the first frame under the piece by a binary search of base and walks the frames the
// piece spans (fit > 0, so base[0] = 0 <= lo < fit <= unit base[n]).
__device__ __forceinline__ void ga2_copy_piece(const long long* __restrict__ table, long long n, int col, const long long* __restrict__ base,
                                               long long unit, unsigned char* __restrict__ dst, int av, long long fit, long long v, int lane) {
    const long long lo = v == 0 ? 0 : v * GA_PIECE - av;
    const long long hi = (v + 1) * GA_PIECE - av < fit ? (v + 1) * GA_PIECE - av : fit;
    long long f = 0, top = n;
    while (top - f > 1) {
        const long long mid = f + ((top - f) >> 1);
        if (unit * base[mid] <= lo) f = mid; else top = mid;
    }
    long long at = lo;
    while (at < hi) {                                           // (empty frames under `at` have base[f + 1] == base[f]: skipped)
        const long long b0 = unit * base[f], b1 = unit * base[f + 1];
        const long long end = b1 < hi ? b1 : hi;
        if (end > at) {
            const unsigned char* src = reinterpret_cast<const unsigned char*>((uintptr_t)table[f * GA2_COLS + col]);
            ga_copy_bytes(src + (at - b0), dst + at, end - at, lane);
            at = end;
        }
        f++;
    }
}

__global__ void __launch_bounds__(FC_THREADS)
frames_gather2_copy_kernel(const long long* __restrict__ table, long long n, long long Sf, unsigned long long* __restrict__ group_mask,
                           unsigned* __restrict__ seg_offset, unsigned* __restrict__ grp_offset, const long long* __restrict__ value_base,
                           const long long* __restrict__ mask_base, unsigned long long* __restrict__ masks, long long mask_capacity,
                           unsigned char* __restrict__ values, long long capacity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long nwaves = (long long)gridDim.x * FC_WAVES;
    const long long MP = GA_PIECE / 8, SP = GA_PIECE / 4;       // group_mask / offset entries of one piece
    const long long GU = (Sf + MP - 1) / MP, SU = (Sf + 1 + SP - 1) / SP;
    const long long vtotal = value_base[n], gtotal = mask_base[n];
    const long long vfit = vtotal < capacity ? vtotal : capacity;                       // value bytes that are written
    const long long mfit = 8 * (gtotal < mask_capacity ? gtotal : mask_capacity);       // mask bytes that are written: whole words
    unsigned char* mbytes = reinterpret_cast<unsigned char*>(masks);
    const int av = (int)((uintptr_t)values & 15), am = (int)((uintptr_t)mbytes & 15);
    const long long VU = vfit > 0 ? (av + vfit + GA_PIECE - 1) / GA_PIECE : 0;
    const long long KU = mfit > 0 ? (am + mfit + GA_PIECE - 1) / GA_PIECE : 0;
    const long long rows = n * (GU + 2 * SU);
    const long long units = rows + VU + KU;
    for (long long u = (long long)blockIdx.x * FC_WAVES + wave; u < units; u += nwaves) {
        if (u < n * GU) {
            const long long f = u / GU, c = u - f * GU;
            const long long cnt = Sf - c * MP < MP ? Sf - c * MP : MP;
            const unsigned long long* src = reinterpret_cast<const unsigned long long*>((uintptr_t)table[f * GA2_COLS + 0]);
            ga_copy_items<unsigned long long, u32x4>(src + c * MP, group_mask + f * Sf + c * MP, cnt, lane);
        } else if (u < rows) {
            const long long r = u - n * GU, which = r >= n * SU ? 1 : 0, q = r - which * n * SU, f = q / SU, c = q - f * SU;
            const long long cnt = Sf + 1 - c * SP < SP ? Sf + 1 - c * SP : SP;
            const unsigned* src = reinterpret_cast<const unsigned*>((uintptr_t)table[f * GA2_COLS + 1 + which]);
            unsigned* dst = (which ? grp_offset : seg_offset) + f * (Sf + 1) + c * SP;
            ga_copy_items<unsigned, unsigned long long>(src + c * SP, dst, cnt, lane);
        } else if (u < rows + VU) {
            ga2_copy_piece(table, n, 4, value_base, 1, values, av, vfit, u - rows, lane);
        } else {
            ga2_copy_piece(table, n, 3, mask_base, 8, mbytes, am, mfit, u - rows - VU, lane);
        }
    }
}

}  // namespace rvt

using namespace rvt;

namespace {
struct FrameGeom2 { long long Gf, Sf; };
static inline FrameGeom2 frame_geom2(long long E) {
    const long long Gf = (E + FC_GROUP - 1) / FC_GROUP;
    return FrameGeom2{Gf, (Gf + 63) / 64};
}
static inline bool frames2_shape_ok(long long F, long long E) { return F >= 1 && F <= 0x7fffffffLL && E >= 1 && E < (1LL << 31); }
// one wave per segment, FC_WAVES of them per workgroup
static inline bool frames2_grid(long long waves, dim3& grid) {
    const long long blocks = (waves + FC_WAVES - 1) / FC_WAVES;
    if (blocks > 0x7fffffffLL) return false;
    grid = dim3((unsigned)blocks);
    return true;
}
static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
}  // namespace

extern "C" {

size_t rvt_frames_pack2_ws_bytes(long long F, long long E) {
    if (!frames2_shape_ok(F, E)) return 0;
    const FrameGeom2 g = frame_geom2(E);
    // the segments' byte counts and group counts, then the frames'
    return ((2 * (size_t)F * (size_t)g.Sf + 2 * (size_t)F) * 4 + 15) & ~(size_t)15;
}

int rvt_frames_pack2(const void* frames, long long F, long long E, void* group_mask, void* seg_offset, void* grp_offset, void* value_base,
                     void* mask_base, void* masks, long long mask_capacity, void* values, long long capacity, void* status, void* ws,
                     size_t ws_bytes, void* stream) {
    RVT_CHECK(frames && group_mask && seg_offset && grp_offset && value_base && mask_base && status && ws, "frames_pack2: null argument");
    RVT_CHECK(frames2_shape_ok(F, E), "frames_pack2: F=%lld frames of E=%lld bytes outside the supported range (F >= 1, 1 <= E < 2^31)", F, E);
    RVT_CHECK(capacity >= 0 && (values || capacity == 0), "frames_pack2: capacity=%lld without a values array", capacity);
    RVT_CHECK(mask_capacity >= 0 && (masks || mask_capacity == 0), "frames_pack2: mask_capacity=%lld without a masks array", mask_capacity);
    RVT_CHECK(ws_bytes >= rvt_frames_pack2_ws_bytes(F, E), "frames_pack2: workspace of %zu bytes, rvt_frames_pack2_ws_bytes says %zu", ws_bytes,
              rvt_frames_pack2_ws_bytes(F, E));
    RVT_CHECK(aligned_to(group_mask, 8) && aligned_to(value_base, 8) && aligned_to(mask_base, 8) && aligned_to(masks, 8) &&
              aligned_to(seg_offset, 4) && aligned_to(grp_offset, 4) && aligned_to(status, 4) && aligned_to(ws, 4),
              "frames_pack2: group_mask / value_base / mask_base / masks need 8-byte, seg_offset / grp_offset / status / ws 4-byte alignment");
    const FrameGeom2 g = frame_geom2(E);
    dim3 grid;
    RVT_CHECK(frames2_grid(F * g.Sf, grid), "frames_pack2: F=%lld frames of %lld segments exceed the grid", F, g.Sf);
    const size_t FS = (size_t)F * (size_t)g.Sf;
    unsigned* seg_count = (unsigned*)ws;
    unsigned* grp_count = seg_count + FS;
    unsigned* frame_count = grp_count + FS;
    unsigned* frame_groups = frame_count + (size_t)F;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frames_mask2_kernel, grid, dim3(FC_THREADS), 0, st, (const unsigned char*)frames, F, E, g.Sf,
                       (unsigned long long*)group_mask, seg_count, grp_count);
    hipLaunchKernelGGL(frames_seg_scan2_kernel, dim3((unsigned)F), dim3(FC_THREADS), 0, st, (const unsigned*)seg_count,
                       (const unsigned*)grp_count, g.Sf, (unsigned*)seg_offset, (unsigned*)grp_offset, frame_count, frame_groups);
    hipLaunchKernelGGL(frames_base_scan2_kernel, dim3(1), dim3(FC_THREADS), 0, st, (const unsigned*)frame_count,
                       (const unsigned*)frame_groups, F, capacity, mask_capacity, (long long*)value_base, (long long*)mask_base, (int*)status);
    if (capacity > 0 || mask_capacity > 0)
        hipLaunchKernelGGL(frames_compact2_kernel, grid, dim3(FC_THREADS), 0, st, (const unsigned char*)frames, F, E, g.Sf,
                           (const unsigned*)seg_offset, (const unsigned*)grp_offset, (const long long*)value_base,
                           (const long long*)mask_base, (unsigned long long*)masks, mask_capacity, (unsigned char*)values, capacity);
    return check_launch("frames_pack2");
}

int rvt_frames_unpack2(const void* group_mask, const void* seg_offset, const void* grp_offset, const void* value_base, const void* mask_base,
                       const void* masks, long long masks_len, const void* values, long long values_len, long long F, long long E,
                       const long long* index, long long Fout, void* out, void* status, void* stream) {
    RVT_CHECK(group_mask && seg_offset && grp_offset && value_base && mask_base && out && status, "frames_unpack2: null argument");
    RVT_CHECK(frames2_shape_ok(F, E) && Fout >= 1, "frames_unpack2: F=%lld, Fout=%lld frames of E=%lld bytes outside the supported range", F, Fout, E);
    RVT_CHECK(values_len >= 0 && (values || values_len == 0), "frames_unpack2: values_len=%lld without a values array", values_len);
    RVT_CHECK(masks_len >= 0 && (masks || masks_len == 0), "frames_unpack2: masks_len=%lld without a masks array", masks_len);
    RVT_CHECK(index || Fout <= F, "frames_unpack2: without an index Fout=%lld must not exceed F=%lld", Fout, F);
    RVT_CHECK(aligned_to(group_mask, 8) && aligned_to(value_base, 8) && aligned_to(mask_base, 8) && aligned_to(masks, 8) &&
              aligned_to(index, 8) && aligned_to(seg_offset, 4) && aligned_to(grp_offset, 4) && aligned_to(status, 4),
              "frames_unpack2: group_mask / value_base / mask_base / masks / index need 8-byte, seg_offset / grp_offset / status 4-byte alignment");
    const FrameGeom2 g = frame_geom2(E);
    dim3 grid;
    RVT_CHECK(Fout <= 0x7fffffffLL && frames2_grid(Fout * g.Sf, grid), "frames_unpack2: Fout=%lld frames of %lld segments exceed the grid", Fout, g.Sf);
    hipLaunchKernelGGL(frames_unpack2_kernel, grid, dim3(FC_THREADS), 0, (hipStream_t)stream, (const unsigned long long*)group_mask,
                       (const unsigned*)seg_offset, (const unsigned*)grp_offset, (const long long*)value_base, (const long long*)mask_base,
                       (const unsigned long long*)masks, masks_len, (const unsigned char*)values, values_len, F, E, g.Gf, g.Sf, index, Fout,
                       (unsigned char*)out, (int*)status);
    return check_launch("frames_unpack2");
}

int rvt_frames_gather2(const long long* table, long long n, long long E, void* group_mask, void* seg_offset, void* grp_offset, void* value_base,
                       void* mask_base, void* masks, long long mask_capacity, void* values, long long capacity, void* status, int max_blocks,
                       void* stream) {
    RVT_CHECK(n >= 0 && n <= 0x7fffffffLL && E >= 1 && E < (1LL << 31), "frames_gather2: n=%lld frames of E=%lld bytes outside the supported range (n >= 0, 1 <= E < 2^31)", n, E);
    if (n == 0) return 0;
    RVT_CHECK(table && group_mask && seg_offset && grp_offset && value_base && mask_base && status, "frames_gather2: null argument");
    RVT_CHECK(capacity >= 0 && (values || capacity == 0), "frames_gather2: capacity=%lld without a values array", capacity);
    RVT_CHECK(mask_capacity >= 0 && (masks || mask_capacity == 0), "frames_gather2: mask_capacity=%lld without a masks array", mask_capacity);
    RVT_CHECK(max_blocks >= 0, "frames_gather2: max_blocks=%d is negative (0 = the default)", max_blocks);
    RVT_CHECK(aligned_to(table, 8) && aligned_to(group_mask, 8) && aligned_to(value_base, 8) && aligned_to(mask_base, 8) && aligned_to(masks, 8) &&
              aligned_to(seg_offset, 4) && aligned_to(grp_offset, 4) && aligned_to(status, 4),
              "frames_gather2: table / group_mask / value_base / mask_base / masks need 8-byte, seg_offset / grp_offset / status 4-byte alignment");
    const FrameGeom2 g = frame_geom2(E);
    // pieces of the copy: the three rows of every frame, and the value bytes and mask words the destination has room for
    const long long GU = (g.Sf * 8 + GA_PIECE - 1) / GA_PIECE, SU = ((g.Sf + 1) * 4 + GA_PIECE - 1) / GA_PIECE;
    const long long vroom = capacity < n * E ? capacity : n * E;
    const long long mroom = 8 * (mask_capacity < n * g.Gf ? mask_capacity : n * g.Gf);
    const long long units = n * (GU + 2 * SU) + (vroom > 0 ? (15 + vroom + GA_PIECE - 1) / GA_PIECE : 0) +
                            (mroom > 0 ? (15 + mroom + GA_PIECE - 1) / GA_PIECE : 0);
    long long blocks = (units + FC_WAVES - 1) / FC_WAVES;
    const long long cap_blocks = max_blocks > 0 ? max_blocks : GA_DEFAULT_BLOCKS;
    if (blocks > cap_blocks) blocks = cap_blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frames_gather2_scan_kernel, dim3(1), dim3(FC_THREADS), 0, st, table, n, E, g.Gf, capacity, mask_capacity,
                       (long long*)value_base, (long long*)mask_base, (int*)status);
    hipLaunchKernelGGL(frames_gather2_copy_kernel, dim3((unsigned)blocks), dim3(FC_THREADS), 0, st, table, n, g.Sf,
                       (unsigned long long*)group_mask, (unsigned*)seg_offset, (unsigned*)grp_offset, (const long long*)value_base,
                       (const long long*)mask_base, (unsigned long long*)masks, mask_capacity, (unsigned char*)values, capacity);
    return check_launch("frames_gather2");
}

}  // extern "C"
