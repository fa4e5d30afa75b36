// extern "C" entry points, part 13: Prophesee / COCO mAP evaluation of detections (cocoeval.hpp; reference
// utils/evaluation/prophesee/ and the COCOeval core behind it).  Compiled without fused multiply-add contraction (Makefile): the
// box filter is fp32 and the IoU double arithmetic in the reference's operation order.
#include <stdint.h>

#include "host.hpp"
#include "cocoeval.hpp"

using namespace rvt;

namespace {
struct EvalWs { unsigned long long *cnt, *bucket; };

int eval_chunks(long long n_slots) { return n_slots <= 0 ? 1 : (int)((n_slots + EVAL_CHUNK - 1) / EVAL_CHUNK); }

size_t carve_eval(char* base, long long n_slots, int K, EvalWs& w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    w.cnt = (unsigned long long*)take((size_t)K * eval_chunks(n_slots) * EVAL_LANES * 8);
    w.bucket = (unsigned long long*)take((size_t)K * EVAL_LANES * EVAL_R * 8);
    return off;
}

bool eval_accumulate_range_ok(long long n_slots, int K) {
    return K >= 1 && K <= EVAL_MAX_NC && n_slots >= 0 && n_slots <= (1LL << 40) &&
           (n_slots + EVAL_CHUNK - 1) / EVAL_CHUNK * K <= 0x7fffffffLL;
}
}  // namespace

extern "C" {

int rvt_coco_match(const float* det, const int* count, const float* labels, const int* label_count, const long long* t_us, int F,
                   int max_det, int G, int num_classes, int det_xywh, float min_diag, float min_side, const double* iou_thrs,
                   long long* rec_key, long long* rec_matched, long long* rec_ignored, int rec_stride, int* counters, void* stream) {
    RVT_CHECK(max_det >= 1 && max_det <= EVAL_MAX_DET, "coco_match: max_det=%d outside the supported range 1..%d", max_det, EVAL_MAX_DET);
    RVT_CHECK(G >= 1 && G <= EVAL_MAX_G, "coco_match: G=%d label rows outside the supported range 1..%d", G, EVAL_MAX_G);
    RVT_CHECK(num_classes >= 1 && num_classes <= EVAL_MAX_NC, "coco_match: num_classes=%d outside the supported range 1..%d",
              num_classes, EVAL_MAX_NC);
    RVT_CHECK(F >= 1 && (long long)F * num_classes <= 0x7fffffffLL, "coco_match: F=%d frames of %d classes exceed the grid", F, num_classes);
    const int need = imin(max_det, EVAL_TOP * num_classes);
    RVT_CHECK(rec_stride >= need, "coco_match: rec_stride=%d smaller than min(max_det, 100 * num_classes) = %d", rec_stride, need);
    RVT_CHECK(min_diag >= 0.f && min_side >= 0.f, "coco_match: negative filter constant");
    RVT_CHECK(det && count && labels && label_count && t_us && iou_thrs && rec_key && rec_matched && rec_ignored && counters,
              "coco_match: null argument");
    const dim3 grid((unsigned)(F * num_classes));
    const float md2 = min_diag * min_diag;
    if (G <= 32)
        hipLaunchKernelGGL((coco_match_kernel<32>), grid, dim3(64), 0, (hipStream_t)stream, det, count, labels, label_count, t_us,
                           iou_thrs, max_det, G, num_classes, rec_stride, det_xywh != 0 ? 1 : 0, md2, min_side, rec_key, rec_matched,
                           rec_ignored, counters);
    else
        hipLaunchKernelGGL((coco_match_kernel<EVAL_MAX_G>), grid, dim3(64), 0, (hipStream_t)stream, det, count, labels, label_count,
                           t_us, iou_thrs, max_det, G, num_classes, rec_stride, det_xywh != 0 ? 1 : 0, md2, min_side, rec_key,
                           rec_matched, rec_ignored, counters);
    return check_launch("coco_match");
}

size_t rvt_coco_accumulate_ws_bytes(long long n_slots, int num_classes) {
    if (!eval_accumulate_range_ok(n_slots, num_classes)) return 0;
    EvalWs w;
    return carve_eval(nullptr, n_slots, num_classes, w);
}

int rvt_coco_accumulate(const long long* perm, const long long* rec_matched, const long long* rec_ignored, long long n_slots,
                        int num_classes, const int* counters, const double* rec_thrs, double* precision, void* ws, size_t ws_bytes,
                        void* stream) {
    RVT_CHECK(eval_accumulate_range_ok(n_slots, num_classes), "coco_accumulate: n_slots=%lld num_classes=%d out of range (1..%d classes)",
              n_slots, num_classes, EVAL_MAX_NC);
    RVT_CHECK(counters && rec_thrs && precision && ws && (n_slots == 0 || (perm && rec_matched && rec_ignored)),
              "coco_accumulate: null argument");
    EvalWs w;
    const size_t need = carve_eval((char*)ws, n_slots, num_classes, w);
    RVT_CHECK(ws_bytes >= need, "coco_accumulate: workspace %zu < %zu bytes", ws_bytes, need);
    const int nch = eval_chunks(n_slots), K = num_classes;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(coco_count_kernel, dim3((unsigned)(nch * K)), dim3(64), 0, st, perm, rec_matched, rec_ignored, n_slots, nch,
                       counters, w.cnt);
    RVT_TRY(check_launch("coco_accumulate (count)"));
    hipLaunchKernelGGL(coco_scan_kernel, dim3(K), dim3(1024), 0, st, n_slots, nch, counters, w.cnt, w.bucket);
    RVT_TRY(check_launch("coco_accumulate (scan)"));
    hipLaunchKernelGGL(coco_emit_kernel, dim3((unsigned)(nch * K)), dim3(64), 0, st, perm, rec_matched, rec_ignored, n_slots, nch,
                       counters, rec_thrs, w.cnt, w.bucket);
    RVT_TRY(check_launch("coco_accumulate (emit)"));
    hipLaunchKernelGGL(coco_finish_kernel, dim3(K), dim3(64), 0, st, K, counters, w.bucket, precision);
    return check_launch("coco_accumulate");
}

int rvt_coco_recall(const long long* rec_key, const long long* rec_matched, const long long* rec_ignored, int F, int rec_stride,
                    int num_classes, long long* tp, void* stream) {
    RVT_CHECK(rec_stride >= 1 && rec_stride <= EVAL_MAX_DET, "coco_recall: rec_stride=%d outside the supported range 1..%d", rec_stride,
              EVAL_MAX_DET);
    RVT_CHECK(num_classes >= 1 && num_classes <= EVAL_MAX_NC, "coco_recall: num_classes=%d outside the supported range 1..%d",
              num_classes, EVAL_MAX_NC);
    RVT_CHECK(F >= 1, "coco_recall: F=%d frames", F);
    RVT_CHECK(rec_key && rec_matched && rec_ignored && tp, "coco_recall: null argument");
    hipLaunchKernelGGL(coco_recall_kernel, dim3((unsigned)imin(F, EVAL_RECALL_GRID)), dim3(64), 0, (hipStream_t)stream, rec_key,
                       rec_matched, rec_ignored, F, rec_stride, num_classes, (unsigned long long*)tp);
    return check_launch("coco_recall");
}

}  // extern "C"
