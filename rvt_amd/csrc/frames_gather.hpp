// Gather of packed frames by address: the frames a batch names, out of any number of packed stores (framecache.hpp, format
// version 1) in device memory or in pinned host memory, into one packed set on the device.  The kernel side of the loader's
// staging='gather' route: the host writes one int64 [n][4] row per frame and the device fetches the bytes itself, so no packed
// byte crosses host memory on its way to the link.
//
//   row f of the table: {address of the frame's Gf masks, address of its Sf + 1 seg_offset entries, address of its first value
//   byte (0 allowed when the count is 0), its count of non-zero bytes}.  A count outside [0, E] is taken as 0 and reported.
//
// Two launches that follow each other on the stream, which is the only ordering used (no workgroup waits for another):
//   scan  one workgroup: value_base[0..n] = exclusive scan of the rows' counts; status WRITTEN: bit 0 total > capacity,
//         bit 2 a row's count was outside [0, E].
//   copy  a grid capped by the caller and walked wave-stride over fixed-size pieces of at most GA_PIECE bytes:
//         n * MU mask pieces, n * SU seg_offset pieces (rows are aligned on both sides: 16-byte accesses for masks and 8-byte
//         ones for seg_offset when source and destination agree modulo that width, 8- / 4-byte ones otherwise), then the value
//         pieces.  A value piece is GA_PIECE bytes of the DESTINATION, cut at the destination's aligned 16-byte lines, so the
//         work is even whatever the frames' fill: the wave finds the first frame under its piece by a binary search of the
//         value_base the scan left, and walks the frames the piece spans.
// Values: a frame's source offset and destination offset have any relative alignment.  Destination lines are whole aligned 16-byte
// stores; the source is read as whole ALIGNED 16-byte lines, one per lane, a lane takes its neighbour's line by shuffle and shifts
// the pair by the byte difference: every source line crosses the link once, in requests that never straddle a 64-byte block,
// which unaligned 16-byte loads would do in every fourth lane.  The first and last line of a run, on either side, move by byte
// accesses inside the run only: no byte outside a frame's values is read, none outside values[0, min(total, capacity)) written.
#pragma once
#include "framecache.hpp"

namespace rvt {

constexpr int GA_PIECE = 16384;                                // bytes of one piece of work (a wave: 16 instructions of 1 KiB)
constexpr int GA_COLS = RVT_FRAMES_GATHER_COLS;                // int64 columns of a table row
constexpr int GA_DEFAULT_BLOCKS = 64;

// --------------------------------------------------------------------------------------------- launch 1: value_base and status
static __global__ void __launch_bounds__(FC_THREADS)
frames_gather_scan_kernel(const long long* __restrict__ table, long long n, long long E, long long capacity,
                          long long* __restrict__ value_base, int* __restrict__ status) {
    __shared__ long long part[2][FC_WAVES];
    __shared__ int badw[FC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long run = 0;
    int par = 0, bad = 0;
    for (long long base = 0; base < n; base += FC_THREADS, par ^= 1) {
        const long long i = base + threadIdx.x;
        long long v = 0;
        if (i < n) {
            v = table[i * GA_COLS + 3];
            if (v < 0 || v > E) { v = 0; bad = 1; }
        }
        const long long pre = fc_block_scan(v, run, part, par);
        if (i < n) value_base[i] = pre;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad |= __shfl_xor(bad, d);
    if (lane == 0) badw[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any = 0;
#pragma unroll
        for (int q = 0; q < FC_WAVES; q++) any |= badw[q];
        value_base[n] = run;
        *status = (run > capacity ? FC_STATUS_CAPACITY : 0) | (any ? FC_STATUS_COUNT : 0);
    }
}

// ------------------------------------------------------------------------------------------------------------------ launch 2: copy
// n items of T, aligned to T on both sides, by one wave: pairs (T2 = two T) where source and destination agree modulo the pair
template <typename T, typename T2>
__device__ __forceinline__ void ga_copy_items(const T* __restrict__ s, T* __restrict__ d, long long n, int lane) {
    static_assert(sizeof(T2) == 2 * sizeof(T), "a pair of items");
    if ((((uintptr_t)s ^ (uintptr_t)d) & sizeof(T)) == 0) {
        const long long head = (n > 0 && ((uintptr_t)d & sizeof(T))) ? 1 : 0;
        const long long pairs = (n - head) >> 1;
        if (head && lane == 0) d[0] = s[0];
        const T2* __restrict__ s2 = reinterpret_cast<const T2*>(s + head);
        T2* __restrict__ d2 = reinterpret_cast<T2*>(d + head);
        for (long long i = lane; i < pairs; i += 64) d2[i] = s2[i];
        if (((n - head) & 1) && lane == 0) d[n - 1] = s[n - 1];
    } else {
        for (long long i = lane; i < n; i += 64) d[i] = s[i];
    }
}

// bytes [sh, sh + 16) of the 32 bytes lo, hi (sh in 0..15, the same in every lane): selects and funnel shifts, no indexed registers
__device__ __forceinline__ u32x4 ga_shift_bytes(const u32x4& lo, const u32x4& hi, int sh) {
    const int ws = sh >> 2, bs = 8 * (sh & 3);
    const unsigned x0 = ws == 0 ? lo[0] : ws == 1 ? lo[1] : ws == 2 ? lo[2] : lo[3];
    const unsigned x1 = ws == 0 ? lo[1] : ws == 1 ? lo[2] : ws == 2 ? lo[3] : hi[0];
    const unsigned x2 = ws == 0 ? lo[2] : ws == 1 ? lo[3] : ws == 2 ? hi[0] : hi[1];
    const unsigned x3 = ws == 0 ? lo[3] : ws == 1 ? hi[0] : ws == 2 ? hi[1] : hi[2];
    const unsigned x4 = ws == 0 ? hi[0] : ws == 1 ? hi[1] : ws == 2 ? hi[2] : hi[3];
    u32x4 r;
    r[0] = (unsigned)(((unsigned long long)x1 << 32 | x0) >> bs);
    r[1] = (unsigned)(((unsigned long long)x2 << 32 | x1) >> bs);
    r[2] = (unsigned)(((unsigned long long)x3 << 32 | x2) >> bs);
    r[3] = (unsigned)(((unsigned long long)x4 << 32 | x3) >> bs);
    return r;
}

// len > 0 bytes from s to d, any alignment on either side, by one wave (every lane calls it with the same arguments)
__device__ __forceinline__ void ga_copy_bytes(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, long long len, int lane) {
    const int a = (int)((uintptr_t)d & 15), b = (int)((uintptr_t)s & 15);
    unsigned char* __restrict__ dline0 = d - a;
    const unsigned char* __restrict__ sline0 = s - b;
    const long long dend = a + len, send = b + len;
    // destination line k = bytes [sh, sh + 16) of the source lines k + off, k + off + 1
    const int off = b < a ? -1 : 0, sh = b < a ? b - a + 16 : b - a;
    const long long nlines = (dend + 15) >> 4;
    // source lines (fc_line_load): whole ones are one 16-byte load, the run's first and last are read byte by byte inside the run
    u32x4 carry = fc_line_load(sline0, 16LL * off, (long long)b, send);    // the line in front of lane 0's (the same load in every lane)
    for (long long m = 0; m < nlines; m += 64) {                // (the same trip count in every lane: the shuffles below are wave-wide)
        const long long k = m + lane;
        const u32x4 hi = fc_line_load(sline0, 16 * (k + off + 1), (long long)b, send);
        u32x4 lo;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const unsigned up = (unsigned)__shfl((int)hi[w], (lane - 1) & 63);
            lo[w] = lane == 0 ? carry[w] : up;
            carry[w] = (unsigned)__shfl((int)hi[w], 63);
        }
        if (k < nlines) fc_line_store(dline0, 16 * k, (long long)a, dend, ga_shift_bytes(lo, hi, sh));
    }
}

static __global__ void __launch_bounds__(FC_THREADS)
frames_gather_copy_kernel(const long long* __restrict__ table, long long n, long long E, long long Gf, long long Sf,
                          unsigned long long* __restrict__ masks, unsigned* __restrict__ seg_offset,
                          const long long* __restrict__ value_base, unsigned char* __restrict__ values, long long capacity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long nwaves = (long long)gridDim.x * FC_WAVES;
    const long long MP = GA_PIECE / 8, SP = GA_PIECE / 4;       // masks / seg_offset entries of one piece
    const long long MU = (Gf + MP - 1) / MP, SU = (Sf + 1 + SP - 1) / SP;
    const long long total = value_base[n];
    const long long fit = total < capacity ? total : capacity;  // value bytes that are written
    const int av = (int)((uintptr_t)values & 15);
    const long long VU = fit > 0 ? (av + fit + GA_PIECE - 1) / GA_PIECE : 0;
    const long long units = n * (MU + SU) + VU;
    for (long long u = (long long)blockIdx.x * FC_WAVES + wave; u < units; u += nwaves) {
        if (u < n * MU) {
            const long long f = u / MU, c = u - f * MU;
            const long long cnt = Gf - c * MP < MP ? Gf - c * MP : MP;
            const unsigned long long* src = reinterpret_cast<const unsigned long long*>((uintptr_t)table[f * GA_COLS + 0]);
            ga_copy_items<unsigned long long, u32x4>(src + c * MP, masks + f * Gf + c * MP, cnt, lane);
        } else if (u < n * (MU + SU)) {
            const long long v = u - n * MU, f = v / SU, c = v - f * SU;
            const long long cnt = Sf + 1 - c * SP < SP ? Sf + 1 - c * SP : SP;
            const unsigned* src = reinterpret_cast<const unsigned*>((uintptr_t)table[f * GA_COLS + 1]);
            ga_copy_items<unsigned, unsigned long long>(src + c * SP, seg_offset + f * (Sf + 1) + c * SP, cnt, lane);
        } else {
            // destination value bytes [lo, hi): piece v of the aligned lines under values
            const long long v = u - n * (MU + SU);
            const long long lo = v == 0 ? 0 : v * GA_PIECE - av;
            const long long hi = (v + 1) * GA_PIECE - av < fit ? (v + 1) * GA_PIECE - av : fit;
            // the frame under byte lo: the largest f with value_base[f] <= lo (value_base[0] = 0 <= lo < fit <= value_base[n])
            long long f = 0, top = n;
            while (top - f > 1) {
                const long long mid = f + ((top - f) >> 1);
                if (value_base[mid] <= lo) f = mid; else top = mid;
            }
            long long at = lo;
            while (at < hi) {                                   // (empty frames under `at` have value_base[f + 1] == at: skipped)
                const long long b0 = value_base[f], b1 = value_base[f + 1];
                const long long end = b1 < hi ? b1 : hi;
                if (end > at) {
                    const unsigned char* src = reinterpret_cast<const unsigned char*>((uintptr_t)table[f * GA_COLS + 2]);
                    ga_copy_bytes(src + (at - b0), values + at, end - at, lane);
                    at = end;
                }
                f++;
            }
        }
    }
}

}  // namespace rvt
