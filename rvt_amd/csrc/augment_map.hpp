// The geometry of the plane augmentation that more than one kernel shares (augment.hpp: augment_planes_kernel; frames_augment.hpp:
// frames_unpack_augment_kernel): workgroup shape, the skewed LDS row image and PyTorch's nearest-exact source index.
#pragma once
#include "common.hpp"

namespace rvt {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_W = 2048;                       // x map: one ushort per column in LDS
constexpr int AUG_ROWS = 8;                           // source rows staged in LDS at once
constexpr int AUG_CHUNK = 64;                         // (plane, row) pairs per workgroup
constexpr int AUG_LDS_ROW = AUG_MAX_W + 4 * (AUG_MAX_W / 256) + 16;
constexpr int AUG_PT = 8;                             // planes table, int32 per sample: flip mode x0 y0 zh zw - -
constexpr int AUG_LT = 12;                            // label table, fp32 per sample: flip mode W-1 x0 y0 hx hy m capx capy - -

__device__ __forceinline__ int aug_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int aug_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int aug_pos(int x) { return x + ((x >> 8) << 2); }

__device__ __forceinline__ int aug_nearest(int i, int n_out, int n_in) {
    const float scale = (float)n_in / (float)n_out;
    const int s = (int)floorf(((float)i + 0.5f) * scale);
    return s < n_in - 1 ? s : n_in - 1;
}

}  // namespace rvt
