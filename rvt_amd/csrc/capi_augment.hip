// extern "C" entry points, part 12: the spatial training augmentation of event planes and box labels (augment.hpp; reference
// data/utils/augmentor.py, data/genx_utils/labels.py).  Compiled without fused multiply-add contraction (Makefile).
#include <stdint.h>

#include "host.hpp"
#include "augment.hpp"

using namespace rvt;

extern "C" {

int rvt_augment_planes(const void* in, void* out, const int* table, int F, int B, int C, int H, int W, void* stream) {
    RVT_CHECK(in && out && table, "augment_planes: null argument");
    RVT_CHECK(F >= 1 && B >= 1 && C >= 1 && H >= 1 && W >= 1, "augment_planes: F=%d B=%d C=%d H=%d W=%d must be positive", F, B, C, H, W);
    RVT_CHECK(W <= AUG_MAX_W, "augment_planes: W=%d outside the supported range 1..%d", W, AUG_MAX_W);
    RVT_CHECK((long long)C * H <= (1 << 24), "augment_planes: C*H=%lld rows per frame outside the supported range", (long long)C * H);
    const size_t bytes = (size_t)F * C * H * W;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    RVT_CHECK(a + bytes <= b || b + bytes <= a, "augment_planes: in and out overlap (the call is not in-place)");
    const int chunks = (C * H + AUG_CHUNK - 1) / AUG_CHUNK;
    RVT_CHECK((long long)F * chunks <= 0x7fffffffLL, "augment_planes: F=%d frames of %d rows exceed the grid", F, C * H);
    const bool vec = W % 16 == 0 && a % 16 == 0 && b % 16 == 0;
    hipLaunchKernelGGL(vec ? augment_planes_kernel<true> : augment_planes_kernel<false>, dim3((unsigned)(F * chunks)), dim3(AUG_THREADS), 0,
                       (hipStream_t)stream, (const unsigned char*)in, (unsigned char*)out, table, B, C, H, W, chunks);
    return check_launch("augment_planes");
}

int rvt_augment_labels(const float* rows, const int* count, const float* table, int F, int B, int G, float* rows_out, int* count_out,
                       float* yolox_out, void* stream) {
    RVT_CHECK(rows && count && table && rows_out && count_out, "augment_labels: null argument");
    RVT_CHECK(F >= 1 && B >= 1 && G >= 1 && G <= 65535, "augment_labels: F=%d B=%d G=%d out of range", F, B, G);
    RVT_CHECK(rows != rows_out && count != count_out, "augment_labels: in and out alias (the call is not in-place)");
    hipLaunchKernelGGL(augment_labels_kernel, dim3((F + AUG_THREADS - 1) / AUG_THREADS), dim3(AUG_THREADS), 0, (hipStream_t)stream,
                       rows, count, table, F, B, G, rows_out, count_out, yolox_out);
    return check_launch("augment_labels");
}

}  // extern "C"
