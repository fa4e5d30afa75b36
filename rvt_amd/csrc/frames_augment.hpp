// Packed frames to augmented planes in one launch: rvt_frames_unpack followed by rvt_augment_planes without the dense tensor
// between them.  out[i] = augment(frame index[i] of the packed set, table row i % B), bit for bit what the two launches give.
//
// The kernel is augment_planes_kernel's body (augment_map.hpp: aug_planes_body) with another stage: a source row is not loaded, it
// is decoded from the packed set (framecache.hpp, format version 1).  One wave takes one source row.  The row's bytes [a, b) of
// the frame lie in at most two 4096-byte segments (W <= 2048); for each piece the wave parks the segment's masks and prefix counts
// in LDS (fc_park_segment; a wave's rows are neighbours, and a segment that is already parked is not loaded and scanned again); a
// lane then takes 4 bytes of the piece at a time (1 byte in the byte path): its mask bits, the rank of the first of them =
// seg prefix + popcount of the bits in front within the group, and the values behind
// value_base[src] + seg_offset[src][segment] + rank, which lie one behind the other: one 4-byte load at their byte address
// (byte loads where that would leave the array), then each value moves under its mask bit.  An item without a set bit costs no
// load.  For zoom-in only the columns [lo, hi] of the window are expanded; the count still starts at the segment.
// An output frame whose index is outside [0, F) is stored as zeros without touching the packed set.
// Reads of `values` are clamped to [0, values_len) and mask bits behind the frame's end are ignored, so any array contents
// terminate in bounds; the table is clamped into the frame as in augment_planes_kernel.
#pragma once
#include "augment_map.hpp"
#include "framecache.hpp"

namespace rvt {

constexpr int FA_WAVES = AUG_THREADS / 64;

// the packed stage of aug_planes_body: frame `idx` of the packed set, one wave per source row
struct AugPackedStage {
    const unsigned long long* __restrict__ fmask;     // the frame's Gf masks
    const unsigned* __restrict__ fseg;                // its Sf + 1 seg_offset entries
    const unsigned char* __restrict__ values;
    unsigned long long vbase, vlen;                   // value_base of the frame; values_len
    long long E, Gf;
    long long parked;                                 // the segment whose masks and prefix counts this wave has parked in LDS

    template <bool VEC>
    __device__ __forceinline__ void fill(unsigned char* srow, const int* src_rows, int nrows, int LW, int lo, int hi, int W) {
        __shared__ unsigned long long mgrp[FA_WAVES][64];       // the masks of the segment a wave is decoding from
        __shared__ int pgrp[FA_WAVES][64];                      // values of the segment in front of each group
        constexpr int V = VEC ? 16 : 1, U = VEC ? 4 : 1;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int j = 0; j < AUG_ROWS / FA_WAVES; j++) {         // one wave decodes one source row; its rows are neighbours, so that
            const int r = wave * (AUG_ROWS / FA_WAVES) + j;     // they mostly share a segment and with it the parked masks
            if (r >= nrows) break;
            const int src = src_rows[r];
            if (src < 0) continue;                    // (the whole wave)
            unsigned char* srw = &srow[r * LW];
            const long long rowb = (long long)src * W;
            long long a = rowb + (long long)lo * V;
            const long long b = rowb + (long long)(hi + 1) * V;
            while (a < b) {                           // the piece of [a, b) inside one segment
                const long long s = a / FC_SEG, sb0 = s * FC_SEG;
                const long long pb = b < sb0 + FC_SEG ? b : sb0 + FC_SEG;
                if (s != parked) {                    // (the whole wave: s follows from the row)
                    wave_rendezvous();                // the previous piece's readers are done with mgrp / pgrp
                    fc_park_segment(fmask, s, E, Gf, mgrp[wave], pgrp[wave], lane);
                    wave_rendezvous();
                    parked = s;
                }
                const unsigned long long start = vbase + (unsigned long long)fseg[s];
                const int n = (int)(pb - a) / U, rel = (int)(a - sb0), xf = (int)(a - rowb);
                for (int i = lane; i < n; i += 64) {
                    const int sb = rel + U * i, gi = sb >> 6, bo = sb & 63;
                    const unsigned long long mm = mgrp[wave][gi];
                    const unsigned bits = (unsigned)(mm >> bo) & (VEC ? 0xfu : 0x1u);
                    const unsigned long long pos = start + (unsigned long long)(pgrp[wave][gi] + __builtin_popcountll(mm & ((1ULL << bo) - 1)));
                    unsigned char* d = srw + aug_pos(xf + U * i);
                    if constexpr (VEC) {
                        // the (at most four) values of the item lie one behind the other: one 4-byte load at their byte address,
                        // byte loads only where it would leave the array; then each value moves under its mask bit
                        unsigned v = 0, w = 0;
                        if (bits && pos < vlen) {
                            const unsigned long long room = vlen - pos;        // (no sum that could wrap: pos may be anything)
                            if (room >= 4) {
                                __builtin_memcpy(&v, values + pos, 4);
                            } else {
#pragma unroll
                                for (int k = 0; k < 3; k++)
                                    if ((unsigned long long)k < room) v |= (unsigned)values[pos + k] << (8 * k);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if ((bits >> k) & 1u) {
                                w |= (v & 0xffu) << (8 * k);
                                v >>= 8;
                            }
                        }
                        *(unsigned*)d = w;            // (x is a multiple of 4: the skew keeps 4-byte alignment)
                    } else {
                        *d = (bits && pos < vlen) ? values[pos] : (unsigned char)0;
                    }
                }
                a = pb;
            }
        }
    }
};

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS)
frames_unpack_augment_kernel(const unsigned long long* __restrict__ masks, const unsigned* __restrict__ seg_offset,
                             const long long* __restrict__ value_base, const unsigned char* __restrict__ values, long long values_len,
                             long long F, long long E, long long Gf, long long Sf, const long long* __restrict__ index,
                             const int* __restrict__ table, int B, int C, int H, int W, int chunks, unsigned char* __restrict__ out,
                             int* __restrict__ status) {
    constexpr int V = VEC ? 16 : 1;
    const int tid = threadIdx.x;
    const int f = blockIdx.x / chunks, q0 = (blockIdx.x % chunks) * AUG_CHUNK, NR = C * H;
    unsigned char* fout = out + (size_t)f * NR * W;

    const long long idx = index ? index[f] : (long long)f;
    if (idx < 0 || idx >= F) {                        // (the whole workgroup) a zero frame: the rows of this chunk, nothing else
        if (idx != -1 && q0 == 0 && tid == 0) fc_status_or(status, FC_STATUS_INDEX);
        const int nr = aug_min(AUG_CHUNK, NR - q0);
        unsigned char* g = fout + (size_t)q0 * W;
        const int n = nr * W / V;
        for (int i = tid; i < n; i += AUG_THREADS) {
            if constexpr (VEC) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                *(u32x4*)(g + (size_t)i * 16) = z;
            } else {
                g[i] = 0;
            }
        }
        return;
    }
    AugPackedStage stage{masks + idx * Gf, seg_offset + idx * (Sf + 1), values, (unsigned long long)value_base[idx],
                         (unsigned long long)values_len, E, Gf, -1};
    aug_planes_body<VEC>(stage, table + (size_t)(f % B) * AUG_PT, fout, q0, C, H, W);
}

}  // namespace rvt
