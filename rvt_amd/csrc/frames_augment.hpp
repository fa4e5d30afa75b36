// Packed frames to augmented planes in one launch: rvt_frames_unpack followed by rvt_augment_planes without the dense tensor
// between them.  out[i] = augment(frame index[i] of the packed set, table row i % B), bit for bit what the two launches give.
//
// The skeleton is augment_planes_kernel's (augment.hpp): one workgroup takes 64 consecutive (plane, row) pairs of one output frame,
// the x map of the sample is built once in LDS, eight source rows at a time are staged in the same skewed LDS row image, and the
// gather and the 16-byte stores are the same code.  Only the staging differs: a source row is not loaded, it is decoded from the
// packed set (framecache.hpp, format version 1).  One wave takes one source row.  The row's bytes [a, b) of the frame lie in at
// most two 4096-byte segments (W <= 2048); for each piece the wave loads the segment's 64 masks (one per lane, tail bits cleared),
// scans their popcounts and parks masks and prefix counts in LDS (a wave's rows are neighbours, and a segment that is already
// parked is not loaded and scanned again); a lane then takes 4 bytes of the piece at a time (1 byte in the byte path): its mask
// bits, the rank of the first of them = seg prefix + popcount of the bits in front within the group, and the values behind
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

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS)
frames_unpack_augment_kernel(const unsigned long long* __restrict__ masks, const unsigned* __restrict__ seg_offset,
                             const long long* __restrict__ value_base, const unsigned char* __restrict__ values, long long values_len,
                             long long F, long long E, long long Gf, long long Sf, const long long* __restrict__ index,
                             const int* __restrict__ table, int B, int C, int H, int W, int chunks, unsigned char* __restrict__ out,
                             int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) unsigned short xmap[AUG_MAX_W];
    __shared__ __attribute__((aligned(16))) unsigned char srow[AUG_ROWS * AUG_LDS_ROW];
    __shared__ int s_src[AUG_CHUNK];                  // source row inside the frame (plane * H + y), -1 = a zero row
    __shared__ unsigned long long mgrp[FA_WAVES][64]; // the masks of the segment a wave is decoding from
    __shared__ int pgrp[FA_WAVES][64];                // values of the segment in front of each group
    constexpr int T = AUG_THREADS, V = VEC ? 16 : 1, U = VEC ? 4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.x / chunks, q0 = (blockIdx.x % chunks) * AUG_CHUNK, NR = C * H;
    unsigned char* fout = out + (size_t)f * NR * W;

    const long long idx = index ? index[f] : (long long)f;
    if (idx < 0 || idx >= F) {                        // (the whole workgroup) a zero frame: the rows of this chunk, nothing else
        if (idx != -1 && q0 == 0 && tid == 0) fc_status_or(status, FC_STATUS_INDEX);
        const int nr = aug_min(AUG_CHUNK, NR - q0);
        unsigned char* g = fout + (size_t)q0 * W;
        const int n = nr * W / V;
        for (int i = tid; i < n; i += T) {
            if constexpr (VEC) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                *(u32x4*)(g + (size_t)i * 16) = z;
            } else {
                g[i] = 0;
            }
        }
        return;
    }

    const int* tb = table + (size_t)(f % B) * AUG_PT;
    const bool flip = tb[0] != 0;
    const int mode = (tb[1] == 1 || tb[1] == 2) ? tb[1] : 0;
    const int zh = aug_min(aug_max(tb[4], 1), H), zw = aug_min(aug_max(tb[5], 1), W);
    const int x0 = aug_min(aug_max(tb[2], 0), W - zw), y0 = aug_min(aug_max(tb[3], 0), H - zh);
    const int LW = ((aug_pos(W - 1) + 4) & ~3) + 4, ZREL = LW - 4;      // LDS row pitch; its last dword stays zero

    for (int x = tid; x < W; x += T) {
        int sx = x;
        if (mode == 1) sx = x0 + aug_nearest(x, W, zw);
        else if (mode == 2) sx = (x >= x0 && x < x0 + zw) ? aug_nearest(x - x0, zw, W) : -1;
        if (sx >= 0 && flip) sx = W - 1 - sx;
        xmap[x] = (unsigned short)(sx < 0 ? ZREL : aug_pos(sx));
    }
    if (tid < AUG_CHUNK) {
        const int q = q0 + tid;
        int src = -1;
        if (q < NR) {
            const int c = q / H, y = q - c * H;
            int sy = y;
            if (mode == 1) sy = y0 + aug_nearest(y, H, zh);
            else if (mode == 2) sy = (y >= y0 && y < y0 + zh) ? aug_nearest(y - y0, zh, H) : -1;
            src = sy < 0 ? -1 : c * H + sy;
        }
        s_src[tid] = src;
    }
    if (tid < AUG_ROWS) *(unsigned*)&srow[tid * LW + ZREL] = 0u;
    // source columns a row needs, in units of V bytes
    const int lo = (mode == 1 ? (flip ? W - x0 - zw : x0) : 0) / V;
    const int hi = (mode == 1 ? (flip ? W - 1 - x0 : x0 + zw - 1) : W - 1) / V;
    const int ndst = W / V;
    const unsigned long long* __restrict__ fmask = masks + idx * Gf;
    const unsigned* __restrict__ fseg = seg_offset + idx * (Sf + 1);
    const unsigned long long vbase = (unsigned long long)value_base[idx];
    const unsigned long long vlen = (unsigned long long)values_len;
    long long parked = -1;                            // the segment whose masks and prefix counts this wave has parked in LDS

    for (int qb = q0; qb < q0 + AUG_CHUNK && qb < NR; qb += AUG_ROWS) {
        const int nrows = aug_min(AUG_ROWS, NR - qb);
        __syncthreads();                              // x map and row table written; the previous group's gather is done
        for (int j = 0; j < AUG_ROWS / FA_WAVES; j++) {         // one wave decodes one source row; its rows are neighbours, so that
            const int r = wave * (AUG_ROWS / FA_WAVES) + j;     // they mostly share a segment and with it the parked masks
            if (r >= nrows) break;
            const int src = s_src[qb - q0 + r];
            if (src < 0) continue;                    // (the whole wave)
            unsigned char* srw = &srow[r * LW];
            const long long rowb = (long long)src * W;
            long long a = rowb + (long long)lo * V;
            const long long b = rowb + (long long)(hi + 1) * V;
            while (a < b) {                           // the piece of [a, b) inside one segment
                const long long s = a / FC_SEG, sb0 = s * FC_SEG;
                const long long pb = b < sb0 + FC_SEG ? b : sb0 + FC_SEG;
                if (s != parked) {                    // (the whole wave: s follows from the row)
                    fc_wave_sync();                   // the previous piece's readers are done with mgrp / pgrp
                    const long long g = s * 64 + lane;
                    unsigned long long m = 0;
                    if (g < Gf) {
                        m = fmask[g];
                        const long long nb = E - 64 * g;        // bytes of the group that exist
                        if (nb < 64) m &= (1ULL << nb) - 1;
                    }
                    const int c = __builtin_popcountll(m);
                    const int inc = fc_wave_scan(c, lane);
                    mgrp[wave][lane] = m;
                    pgrp[wave][lane] = inc - c;
                    fc_wave_sync();
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
        __syncthreads();
        {
            int r = tid / ndst, p = tid - r * ndst;
            const int dr = T / ndst, dp = T - dr * ndst;
            while (r < nrows) {
                const bool zero = s_src[qb - q0 + r] < 0;
                const unsigned char* s = &srow[r * LW];
                unsigned char* g = fout + (size_t)(qb + r) * W + p * V;
                if constexpr (VEC) {
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (!zero) {
                        const u32x4 ma = *(const u32x4*)&xmap[p * 16], mb = *(const u32x4*)&xmap[p * 16 + 8];
                        const unsigned m[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
                        unsigned w[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const unsigned a = m[2 * k], b = m[2 * k + 1];
                            w[k] = (unsigned)s[a & 0xffffu] | ((unsigned)s[a >> 16] << 8) | ((unsigned)s[b & 0xffffu] << 16) |
                                   ((unsigned)s[b >> 16] << 24);
                        }
                        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
                    }
                    *(u32x4*)g = v;
                } else {
                    *g = zero ? (unsigned char)0 : s[xmap[p]];
                }
                r += dr; p += dp;
                if (p >= ndst) { p -= ndst; r++; }
            }
        }
    }
}

}  // namespace rvt
