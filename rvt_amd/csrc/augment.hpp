// Spatial training augmentation on the device: horizontal flip, zoom-in and zoom-out of the uint8 event planes and of the box
// labels of a whole batch of sequences, every per-sample parameter read from a small device table the host writes.
// Reference: data/utils/augmentor.py (RandomSpatialAugmentorGenX: th.flip, interpolate(mode='nearest-exact') on a crop / into a
// zero canvas) and data/genx_utils/labels.py (ObjectLabels.flip_lr_ / zoom_in_and_rescale_ / zoom_out_and_rescale_ / scale_).
//
// Planes (augment_planes_kernel): in / out uint8 [F][C][H][W], frame f of sample f % B.  The reference's order is flip, then zoom:
//     n(i; n_out, n_in) = min((int)floorf((i + 0.5f) * ((float)n_in / (float)n_out)), n_in - 1)         PyTorch's CPU nearest-exact
//     S[y][x] = flip ? in[y][W-1-x] : in[y][x]
//     mode 0: out = S      mode 1: out[y][x] = S[y0 + n(y; H, zh)][x0 + n(x; W, zw)]
//     mode 2: out[y][x] = S[n(y-y0; zh, H)][n(x-x0; zw, W)] inside the window [y0, y0+zh) x [x0, x0+zw), 0 outside
// A pure byte mover.  One workgroup takes 64 consecutive (plane, row) pairs of one frame.  All of them share one x map, built once
// per workgroup in LDS as the LDS position of the source byte of every output column (flip and window offset folded in; columns
// outside a zoom-out window point at a zero byte).  Eight source rows at a time are brought into LDS with 16-byte loads of the
// contiguous source segment ([x0, x0+zw) for zoom-in, the whole row otherwise), and every lane assembles 16 output pixels with
// byte reads from LDS and writes them with one 16-byte store.  Source byte x sits at LDS position x + 4 * (x / 256): a wave's 64
// lanes read dwords about 4 apart, and the skew spreads what would be a 4-way bank conflict over neighbouring banks.
// W % 16 != 0 or a base that is not 16-byte aligned takes the same kernel with byte-wide global accesses (VEC = false).
// The table is clamped into the frame on the device, so any table contents terminate in bounds.
//
// Labels (augment_labels_kernel): rows fp32 [F][G][7] (t x y w h class_id class_confidence), count int32 [F] (-1 = no labels).
// One thread per frame walks its rows in order, so survivors keep their order.  Every operation is one rounded fp32 operation in
// the reference's order (this translation unit is compiled with -ffp-contract=off: x1 - x*m rounds x*m first); the constants
// come from the host, computed in double and rounded once, which is what torch does with Python scalars on fp32 tensors.
#pragma once
#include "common.hpp"
#include "augment_map.hpp"                            // geometry and aug_planes_body: shared with frames_augment.hpp

namespace rvt {

// the dense stage of aug_planes_body: the cooperative (row, 16-byte piece) walk over the source rows of the frame `fin`
struct AugDenseStage {
    const unsigned char* __restrict__ fin;
    template <bool VEC>
    __device__ __forceinline__ void fill(unsigned char* srow, const int* src_rows, int nrows, int LW, int lo, int hi, int W) {
        constexpr int T = AUG_THREADS, V = VEC ? 16 : 1;
        const int tid = threadIdx.x, nsrc = hi - lo + 1;
        int r = tid / nsrc, p = tid - r * nsrc;
        const int dr = T / nsrc, dp = T - dr * nsrc;
        while (r < nrows) {
            const int src = src_rows[r];
            if (src >= 0) {
                const int x = (lo + p) * V;
                const unsigned char* g = fin + (size_t)src * W + x;
                unsigned char* s = &srow[r * LW + aug_pos(x)];
                if constexpr (VEC) {
                    const u32x4 v = *(const u32x4*)g;
                    unsigned* s4 = (unsigned*)s;      // the skew keeps 4-byte, not 16-byte, alignment
                    s4[0] = v.x; s4[1] = v.y; s4[2] = v.z; s4[3] = v.w;
                } else {
                    *s = *g;
                }
            }
            r += dr; p += dp;
            if (p >= nsrc) { p -= nsrc; r++; }
        }
    }
};

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS)
augment_planes_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, const int* __restrict__ table,
                      int B, int C, int H, int W, int chunks) {
    const int f = blockIdx.x / chunks, q0 = (blockIdx.x % chunks) * AUG_CHUNK;
    const size_t frame = (size_t)f * C * H * W;
    AugDenseStage stage{in + frame};
    aug_planes_body<VEC>(stage, table + (size_t)(f % B) * AUG_PT, out + frame, q0, C, H, W);
}

// scale_ of the reference: returns whether the row survives (w > 0 and h > 0)
__device__ __forceinline__ bool aug_scale(float& x, float& y, float& w, float& h, float m, float capx, float capy) {
    const float x1 = fminf((x + w) * m, capx), y1 = fminf((y + h) * m, capy);
    x = x * m;
    y = y * m;
    w = x1 - x;
    h = y1 - y;
    return w > 0.f && h > 0.f;
}

__global__ void __launch_bounds__(AUG_THREADS)
augment_labels_kernel(const float* __restrict__ rows, const int* __restrict__ count, const float* __restrict__ table, int F, int B,
                      int G, float* __restrict__ rows_out, int* __restrict__ count_out, float* __restrict__ yolox_out) {
    const int f = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (f >= F) return;
    const float* tb = table + (size_t)(f % B) * AUG_LT;
    const bool flip = tb[0] != 0.f;
    const int mode = tb[1] == 1.f ? 1 : (tb[1] == 2.f ? 2 : 0);
    const float wm1 = tb[2], zx0 = tb[3], zy0 = tb[4], hx = tb[5], hy = tb[6], m = tb[7], capx = tb[8], capy = tb[9];
    const int n_in = count[f], n = aug_min(aug_max(n_in, 0), G);
    const float* src = rows + (size_t)f * G * 7;
    float* dst = rows_out + (size_t)f * G * 7;
    float* yo = yolox_out ? yolox_out + (size_t)f * G * 5 : nullptr;
    int kept = 0;
    for (int i = 0; i < n; i++) {
        const float* r = src + i * 7;
        float x = r[1], y = r[2], w = r[3], h = r[4];
        bool keep = true;
        if (flip) x = (wm1 - x) - w;
        if (mode == 1) {
            const float cx0 = fminf(fmaxf(x, zx0), hx), cx1 = fminf(fmaxf(x + w, zx0), hx);
            const float cy0 = fminf(fmaxf(y, zy0), hy), cy1 = fminf(fmaxf(y + h, zy0), hy);
            x = cx0 - zx0;
            y = cy0 - zy0;
            w = cx1 - cx0;
            h = cy1 - cy0;
            keep = w > 0.f && h > 0.f;
            if (keep) keep = aug_scale(x, y, w, h, m, capx, capy);
        } else if (mode == 2) {
            keep = aug_scale(x, y, w, h, m, capx, capy);
            x = x + zx0;
            y = y + zy0;
        }
        if (!keep) continue;
        float* d = dst + kept * 7;
        d[0] = r[0]; d[1] = x; d[2] = y; d[3] = w; d[4] = h; d[5] = r[5]; d[6] = r[6];
        if (yo) {
            float* o = yo + kept * 5;
            o[0] = r[5]; o[1] = x + 0.5f * w; o[2] = y + 0.5f * h; o[3] = w; o[4] = h;
        }
        kept++;
    }
    for (int i = kept; i < G; i++) {
        for (int k = 0; k < 7; k++) dst[i * 7 + k] = 0.f;
        if (yo) for (int k = 0; k < 5; k++) yo[i * 5 + k] = 0.f;
    }
    count_out[f] = n_in < 0 ? -1 : kept;
}

}  // namespace rvt
