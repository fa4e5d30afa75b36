// The plane augmentation that more than one kernel runs (augment.hpp: augment_planes_kernel; frames_augment.hpp:
// frames_unpack_augment_kernel): workgroup shape, the skewed LDS row image, PyTorch's nearest-exact source index, and the body of
// the kernels: table clamp, x map, row table, and the gather and store of the output rows.  The kernels differ in one step, how
// the source rows reach LDS, which each hands in as a stage policy.
#pragma once
#include "common.hpp"

namespace rvt {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_W = 2048;                       // x map: one ushort per column in LDS
constexpr int AUG_ROWS = 8;                           // source rows staged in LDS at once
constexpr int AUG_CHUNK = 64;                         // (plane, row) pairs per workgroup
constexpr int AUG_LDS_ROW = AUG_MAX_W + 4 * (AUG_MAX_W / 256) + 16;
constexpr int AUG_PT = RVT_AUGMENT_PLANES_COLS;       // planes table, int32 per sample: flip mode x0 y0 zh zw - -
constexpr int AUG_LT = RVT_AUGMENT_LABEL_COLS;        // label table, fp32 per sample: flip mode W-1 x0 y0 hx hy m capx capy - -

__device__ __forceinline__ int aug_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int aug_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int aug_pos(int x) { return x + ((x >> 8) << 2); }

__device__ __forceinline__ int aug_nearest(int i, int n_out, int n_in) {
    const float scale = (float)n_in / (float)n_out;
    const int s = (int)floorf(((float)i + 0.5f) * scale);
    return s < n_in - 1 ? s : n_in - 1;
}

// The rows [q0, q0 + AUG_CHUNK) of one output frame (fout: its C * H rows of W bytes) under the table row tb, by the whole
// workgroup.  VEC: 16-byte accesses (W % 16 == 0, aligned bases), else byte accesses.  Source byte x of a staged row sits at LDS
// position aug_pos(x) of its row image of pitch LW, whose last dword stays zero (columns outside a zoom-out window point there).
// stage.template fill<VEC>(srow, src, nrows, LW, lo, hi, W) is called by every thread between two __syncthreads(): it brings the
// columns [lo * V, (hi + 1) * V) (V = 16 or 1 bytes) of the source rows src[r] (row inside the frame, -1 = a zero row that is not
// staged), r < nrows, to srow[r * LW + aug_pos(x)], and nothing else.
template <bool VEC, class Stage>
__device__ __forceinline__ void aug_planes_body(Stage& stage, const int* __restrict__ tb, unsigned char* __restrict__ fout, int q0,
                                                int C, int H, int W) {
    __shared__ __attribute__((aligned(16))) unsigned short xmap[AUG_MAX_W];
    __shared__ __attribute__((aligned(16))) unsigned char srow[AUG_ROWS * AUG_LDS_ROW];
    __shared__ int s_src[AUG_CHUNK];                  // source row inside the frame (plane * H + y), -1 = a zero row
    constexpr int T = AUG_THREADS, V = VEC ? 16 : 1;
    const int tid = threadIdx.x, NR = C * H;
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

    for (int qb = q0; qb < q0 + AUG_CHUNK && qb < NR; qb += AUG_ROWS) {
        const int nrows = aug_min(AUG_ROWS, NR - qb);
        __syncthreads();                              // x map and row table written; the previous group's gather is done
        stage.template fill<VEC>(srow, &s_src[qb - q0], nrows, LW, lo, hi, W);
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
