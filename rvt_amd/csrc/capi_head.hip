// extern "C" entry points, part 10: the YOLOX head's tail — box decode, batched on-device SimOTA
// assignment and the detection losses with their gradient (simota.hpp; reference models/detection/yolox/models/yolo_head.py),
// the detection post-processing that follows the eval-mode decode (nms.hpp; reference models/detection/yolox/utils/boxes.py), and the
// two fused: head maps in, padded detections out (rvt_yolox_detect).  Decode and NMS share this translation unit and its flags, so
// expf, the divide and the multiplies of the fused kernel are the instructions of the two kernels it replaces.
#include "host.hpp"
#include "simota.hpp"
#include "nms.hpp"

using namespace rvt;

namespace {
static bool fill_levels(YoloLevels& lv, const int* level_hw, const int* level_stride, int L, int A) {
    if (L < 1 || L > 8) return false;
    lv.n = L;
    int a = 0;
    for (int l = 0; l < 8; l++) {
        lv.h[l] = l < L ? level_hw[2 * l] : 1;
        lv.w[l] = l < L ? level_hw[2 * l + 1] : 1;
        lv.stride[l] = l < L ? level_stride[l] : 1;
        lv.a0[l] = a;
        if (l < L) { if (lv.h[l] < 1 || lv.w[l] < 1 || lv.stride[l] < 1) return false; a += lv.h[l] * lv.w[l]; }
    }
    lv.a0[8] = a;
    for (int l = L; l < 8; l++) lv.a0[l] = a;
    return a == A;
}
struct SimotaWs {
    float *cost, *iou, *piou, *partial;
    int *nlabel, *meta, *count, *cand, *match;
    size_t bytes;
};
static SimotaWs carve_simota(char* base, int B, int G, int A) {
    SimotaWs w;
    size_t off = 0;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += (n + 255) & ~(size_t)255; return p; };
    const size_t bga = (size_t)B * imax(G, 1) * A, ba = (size_t)B * A;
    w.cost = (float*)take(bga * 4);
    w.iou = (float*)take(bga * 4);
    w.piou = (float*)take(ba * 4);
    w.partial = (float*)take((size_t)B * ((A + 255) / 256) * 3 * 4);
    w.nlabel = (int*)take((size_t)B * 4);
    w.meta = (int*)take(16);
    w.count = (int*)take(ba * 4);
    w.cand = (int*)take(ba * 4);
    w.match = (int*)take(ba * 4);
    w.bytes = off;
    return w;
}
static size_t carve_nms(char* base, int B, int A, NmsWs& w) {
    size_t off = 0;
    auto take = [&](size_t n) { char* p = base ? base + off : nullptr; off += (n + 255) & ~(size_t)255; return p; };
    const size_t ba = (size_t)B * A;
    w.keys = (unsigned long long*)take(ba * 8);
    w.sorted = (unsigned long long*)take(ba * 8);
    w.x1 = (float*)take(ba * 4);
    w.y1 = (float*)take(ba * 4);
    w.x2 = (float*)take(ba * 4);
    w.y2 = (float*)take(ba * 4);
    w.area = (float*)take(ba * 4);
    w.obj = (float*)take(ba * 4);
    w.conf = (float*)take(ba * 4);
    w.cls = (int*)take(ba * 4);
    w.acls = (int*)take(ba * 4);
    return off;
}
static bool nms_range_ok(int B, int A, int nc) {
    return B >= 1 && B <= 65535 && A >= 1 && A <= NMS_MAX_A && nc >= 1 && nc <= NMS_MAX_NC;
}
}  // namespace

extern "C" {

int rvt_yolox_decode(const void* reg_obj, const void* cls, int ld_ro, int ld_cls, int dtype, int B, int H, int W, int stride,
                     int num_classes, int anchor_offset, int A, float* pred_train, float* pred_infer, void* stream) {
    RVT_CHECK(reg_obj && cls && ld_ro >= 5 && ld_cls >= num_classes && num_classes >= 1, "yolox_decode: reg_obj needs >= 5 columns, cls >= %d", num_classes);
    RVT_CHECK(B >= 1 && H >= 1 && W >= 1 && stride >= 1 && anchor_offset >= 0 && anchor_offset + H * W <= A, "yolox_decode: level does not fit the anchor range");
    RVT_CHECK(pred_train || pred_infer, "yolox_decode: nothing to write");
    const int rows = B * H * W;
    DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((yolox_decode_kernel<T>), dim3(grid_for((size_t)rows, 4096)), dim3(256), 0, (hipStream_t)stream,
                                             (const T*)reg_obj, (const T*)cls, ld_ro, ld_cls, B, H, W, (float)stride, num_classes,
                                             anchor_offset, A, pred_train, pred_infer));
    return check_launch("yolox_decode");
}

int rvt_yolox_decode_bwd(const float* g_pred, const float* pred_train, const float* col_scale, void* d_reg_obj, void* d_cls, int ld_ro,
                         int ld_cls, int dtype, int B, int H, int W, int stride, int num_classes, int anchor_offset, int A, void* stream) {
    RVT_CHECK(g_pred && pred_train && col_scale && d_reg_obj && d_cls && ld_ro >= 5 && ld_cls >= num_classes, "yolox_decode_bwd: bad arguments");
    RVT_CHECK(B >= 1 && H >= 1 && W >= 1 && anchor_offset >= 0 && anchor_offset + H * W <= A, "yolox_decode_bwd: level does not fit the anchor range");
    const int rows = B * H * W;
    DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((yolox_decode_bwd_kernel<T>), dim3(grid_for((size_t)rows, 4096)), dim3(256), 0, (hipStream_t)stream,
                                             g_pred, pred_train, col_scale, (T*)d_reg_obj, (T*)d_cls, ld_ro, ld_cls, B, H, W, (float)stride,
                                             num_classes, anchor_offset, A));
    return check_launch("yolox_decode_bwd");
}

size_t rvt_simota_ws_bytes(int B, int G, int A) {
    if (B < 1 || G < 0 || A < 1) return 0;
    return carve_simota(nullptr, B, G, A).bytes;
}

int rvt_simota_loss(const float* pred_train, const float* labels, const int* level_hw, const int* level_stride, int L, int B, int G, int A,
                    int num_classes, float* losses, float* g_pred, int* match_out, float* piou_out, void* ws, size_t ws_bytes,
                    void* stream) {
    RVT_CHECK(pred_train && losses && ws && (labels || G == 0), "simota_loss: null argument");
    RVT_CHECK(B >= 1 && B <= 65535 && G >= 0 && G <= 65535 && A >= 1 && num_classes >= 1, "simota_loss: B=%d G=%d A=%d out of range", B, G, A);
    YoloLevels lv;
    RVT_CHECK(fill_levels(lv, level_hw, level_stride, L, A), "simota_loss: the %d levels do not add up to A=%d anchors", L, A);
    const SimotaWs w = carve_simota((char*)ws, B, G, A);
    RVT_CHECK(ws_bytes >= w.bytes, "simota_loss: workspace %zu < %zu bytes", ws_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 ga((A + 255) / 256, B);
    int* match = match_out ? match_out : w.match;
    float* piou = piou_out ? piou_out : w.piou;
    hipLaunchKernelGGL(simota_count_labels_kernel, dim3(1), dim3(256), 0, st, labels, B, G, w.nlabel, w.meta);
    hipLaunchKernelGGL(simota_cost_kernel, ga, dim3(256), 0, st, pred_train, labels, w.nlabel, lv, B, G, A, num_classes, w.cost, w.iou, w.count);
    if (G > 0) hipLaunchKernelGGL(simota_select_kernel, dim3(G, B), dim3(256), 0, st, w.cost, w.iou, w.nlabel, G, A, w.count, w.cand);
    hipLaunchKernelGGL(simota_resolve_kernel, ga, dim3(256), 0, st, w.cost, w.iou, w.nlabel, w.count, w.cand, G, A, match, piou, w.meta);
    hipLaunchKernelGGL(yolox_loss_kernel, ga, dim3(256), 0, st, pred_train, labels, match, piou, w.meta, G, A, num_classes, w.partial, g_pred);
    hipLaunchKernelGGL(yolox_loss_finalize_kernel, dim3(1), dim3(256), 0, st, w.partial, (int)(ga.x * ga.y), w.meta, losses);
    return check_launch("simota_loss");
}

size_t rvt_yolox_postprocess_ws_bytes(int B, int A, int num_classes) {
    if (!nms_range_ok(B, A, num_classes)) return 0;
    NmsWs w;
    return carve_nms(nullptr, B, A, w);
}

int rvt_yolox_postprocess(const float* pred, int B, int A, int num_classes, float conf_thre, float nms_thre, int class_agnostic,
                          int max_det, float* det, int* count, int* anchor_idx, void* ws, size_t ws_bytes, void* stream) {
    RVT_CHECK(A >= 1 && A <= NMS_MAX_A, "yolox_postprocess: A=%d anchors outside the supported range 1..%d", A, NMS_MAX_A);
    RVT_CHECK(num_classes >= 1 && num_classes <= NMS_MAX_NC, "yolox_postprocess: num_classes=%d outside the supported range 1..%d",
              num_classes, NMS_MAX_NC);
    RVT_CHECK(B >= 1 && B <= 65535 && max_det >= 1 && max_det <= (1 << 24), "yolox_postprocess: B=%d max_det=%d out of range", B, max_det);
    RVT_CHECK(pred && det && count && ws, "yolox_postprocess: null argument");
    NmsWs w;
    const size_t need = carve_nms((char*)ws, B, A, w);
    RVT_CHECK(ws_bytes >= need, "yolox_postprocess: workspace %zu < %zu bytes", ws_bytes, need);
    hipLaunchKernelGGL(yolox_postprocess_kernel, dim3(B), dim3(NMS_THREADS), 0, (hipStream_t)stream, pred, A, num_classes, conf_thre,
                       nms_thre, class_agnostic != 0 ? 1 : 0, max_det, det, count, anchor_idx, w);
    return check_launch("yolox_postprocess");
}

size_t rvt_yolox_detect_ws_bytes(int B, int A, int num_classes) { return rvt_yolox_postprocess_ws_bytes(B, A, num_classes); }

int rvt_yolox_detect(const void* const* reg_obj, const void* const* cls, int ld_ro, int ld_cls, int dtype, const int* level_hw,
                     const int* level_stride, int L, int B, int A, int num_classes, float conf_thre, float nms_thre, int class_agnostic,
                     int max_det, float* det, int* count, int* anchor_idx, void* ws, size_t ws_bytes, void* stream) {
    RVT_CHECK(L >= 1 && L <= 8, "yolox_detect: %d levels outside the supported range 1..8", L);
    RVT_CHECK(A >= 1 && A <= NMS_MAX_A, "yolox_detect: A=%d anchors outside the supported range 1..%d", A, NMS_MAX_A);
    RVT_CHECK(num_classes >= 1 && num_classes <= NMS_MAX_NC, "yolox_detect: num_classes=%d outside the supported range 1..%d", num_classes,
              NMS_MAX_NC);
    RVT_CHECK(B >= 1 && B <= 65535 && max_det >= 1 && max_det <= (1 << 24), "yolox_detect: B=%d max_det=%d out of range", B, max_det);
    RVT_CHECK(reg_obj && cls && level_hw && level_stride && det && count && ws, "yolox_detect: null argument");
    RVT_CHECK(ld_ro >= 5 && ld_cls >= num_classes, "yolox_detect: reg_obj needs >= 5 columns, cls >= %d", num_classes);
    YoloLevels lv;
    RVT_CHECK(fill_levels(lv, level_hw, level_stride, L, A), "yolox_detect: the %d levels do not add up to A=%d anchors", L, A);
    DetectMaps m;
    for (int l = 0; l < 8; l++) {
        m.ro[l] = l < L ? reg_obj[l] : nullptr;
        m.cl[l] = l < L ? cls[l] : nullptr;
        RVT_CHECK(l >= L || (m.ro[l] && m.cl[l]), "yolox_detect: level %d has a null map", l);
    }
    m.ld_ro = ld_ro;
    m.ld_cls = ld_cls;
    NmsWs w;
    const size_t need = carve_nms((char*)ws, B, A, w);
    RVT_CHECK(ws_bytes >= need, "yolox_detect: workspace %zu < %zu bytes", ws_bytes, need);
    DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((yolox_detect_kernel<T>), dim3(B), dim3(NMS_THREADS), 0, (hipStream_t)stream, m, lv, A, num_classes,
                                             conf_thre, nms_thre, class_agnostic != 0 ? 1 : 0, max_det, det, count, anchor_idx, w));
    return check_launch("yolox_detect");
}

}  // extern "C"
