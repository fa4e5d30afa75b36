"""Detection post-processing on the device: score filter + batched greedy NMS (csrc/nms.hpp, rvt_yolox_postprocess).

Mirror of the reference's `postprocess` (models/detection/yolox/utils/boxes.py:32-76), the step every consumer of the head's
eval-mode output runs first (modules/detection.py:175-178, :261-264): rows with obj * max class score >= conf_thre, per-class
(or class-agnostic) NMS, 7-column rows (x1, y1, x2, y2, obj_conf, class_conf, class_pred) in descending score order.

  * `postprocess(prediction, num_classes, conf_thre=0.7, nms_thre=0.45, class_agnostic=False)`: the reference's name, argument
    order, defaults and return value (a list with one [n][7] tensor per image, None for an image without detections).  One
    launch for the whole batch and ONE read-back of the per-image counts, the only host synchronisation.
  * `postprocess_padded(...) -> (det [B][max_det][7], count [B], anchor_idx [B][max_det])`: the sync-free form.  Workspace and
    outputs are cached per (B, A, num_classes, max_det, device) or passed in, so from the second call on nothing is allocated
    and the call can be captured in a torch.cuda.graph.  Rows from min(count, max_det) on are zero, their anchor_idx -1;
    count is the number kept BEFORE the max_det cap.

  * `detect_padded(maps, hws, strides, num_classes, ...)`: the same three tensors straight from the head's per-level prediction maps
    (rvt_yolox_detect: decode + score filter + NMS in ONE launch, the [B][A][5 + nc] tensor never written), bit-identical to
    `postprocess_padded(decode(maps, ...))`.  YOLOXHead.detect_padded and YoloXDetector.detect end in it.

Differences to the reference a caller can see: the input is NOT overwritten with corner boxes (the reference mutates
prediction[:, :, :4] in place); non-fp32 or non-contiguous input is converted first; exact score ties are ordered by anchor
index and exact class ties go to the lower class (the reference leaves both to the sort / max implementation).  There is no
PyTorch fallback: a missing kernel or an unsupported shape raises with the library's message.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L

Tensor = torch.Tensor

_cache: Dict[tuple, Tuple[Tensor, Tensor, Tensor, Tensor]] = {}


def _buffers(B: int, A: int, nc: int, max_det: int, dev: torch.device):
    key = (B, A, nc, max_det, dev.type, dev.index)
    hit = _cache.get(key)
    if hit is None:
        ws_bytes = int(L.get_lib().rvt_yolox_postprocess_ws_bytes(B, A, nc))
        hit = (torch.empty(B, max_det, 7, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, max_det, dtype=torch.int32, device=dev), torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev))
        _cache[key] = hit
    return hit


def postprocess_padded(prediction: Tensor, num_classes: int, conf_thre: float, nms_thre: float, class_agnostic: bool = False,
                       max_det: Optional[int] = None, out: Optional[Tuple[Tensor, Tensor, Tensor]] = None):
    """prediction [B][A][5 + num_classes] (cx cy w h obj cls...) -> (det, count, anchor_idx); no host synchronisation.

    max_det: rows per image (default A: never truncated).  out: (det, count, anchor_idx) to write into, float32 [B][max_det][7],
    int32 [B], int32 [B][max_det]; without it the tensors cached for this shape are returned, i.e. the NEXT call with the same
    shape overwrites them (clone what has to outlive it).  The workspace is cached per shape and device either way, not per stream:
    calls of one shape that may overlap on different streams are the caller's to order."""
    if prediction.dim() != 3 or prediction.shape[2] != 5 + num_classes:
        raise ValueError(f'prediction must be [B][A][5 + num_classes = {5 + num_classes}], got {tuple(prediction.shape)}')
    pred = prediction.detach()
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        pred = pred.float().contiguous()
    B, A, _ = pred.shape
    max_det = A if max_det is None else int(max_det)
    if B == 0:
        raise ValueError('prediction holds no image')
    det, count, aidx, ws = _buffers(B, A, num_classes, max_det, pred.device)
    if out is not None:
        det, count, aidx = out
        for t, shp, dt in ((det, (B, max_det, 7), torch.float32), (count, (B,), torch.int32), (aidx, (B, max_det), torch.int32)):
            if tuple(t.shape) != shp or t.dtype != dt or t.device != pred.device:
                raise ValueError(f'out tensor must be {dt} {shp} on {pred.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    L.call('rvt_yolox_postprocess', L.ptr(pred), B, A, num_classes, float(conf_thre), float(nms_thre), int(bool(class_agnostic)),
           max_det, L.ptr(det), L.ptr(count), L.ptr(aidx), L.ptr(ws), ws.numel(), L.stream_of(pred))
    return det, count, aidx


_detect_cache: Dict[tuple, tuple] = {}


def _check_out(out, B: int, max_det: int, dev: torch.device):
    det, count, aidx = out
    for t, shp, dt in ((det, (B, max_det, 7), torch.float32), (count, (B,), torch.int32), (aidx, (B, max_det), torch.int32)):
        if tuple(t.shape) != shp or t.dtype != dt or t.device != dev:
            raise ValueError(f'out tensor must be {dt} {shp} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    return det, count, aidx


def detect_padded(maps: Sequence[Tensor], hws, strides, num_classes: int, conf_thre: float, nms_thre: float,
                  class_agnostic: bool = False, max_det: Optional[int] = None, out: Optional[Tuple[Tensor, Tensor, Tensor]] = None):
    """The head's prediction maps -> (det, count, anchor_idx) in ONE launch, no host synchronisation (rvt_yolox_detect).

    maps: [reg_obj_0, cls_0, reg_obj_1, cls_1, ...] as YOLOXHead._pred_maps returns them, (B, H, W, ld) of one dtype (fp32 or bf16)
    with one ld_ro >= 5 and one ld_cls >= num_classes for all levels; hws[l] = (H, W), strides[l] the level's stride.  Everything
    else as postprocess_padded: max_det defaults to A, `out` or the tensors cached for this shape (overwritten by the next call of
    the same shape), workspace cached per shape and device.  Equal to postprocess_padded(decode(maps, ...)) bit for bit."""
    hws, strides = tuple((int(h), int(w)) for h, w in hws), tuple(int(s) for s in strides)
    nl = len(hws)
    if len(maps) != 2 * nl or len(strides) != nl or nl == 0:
        raise ValueError(f'{len(maps)} maps, {nl} level shapes and {len(strides)} strides do not describe the same levels')
    maps = [m.detach().contiguous() for m in maps]
    ro0, cl0 = maps[0], maps[1]
    B, dev = ro0.shape[0], ro0.device
    if B == 0:
        raise ValueError('the maps hold no image')
    for l in range(nl):
        ro, cl = maps[2 * l], maps[2 * l + 1]
        if ro.dtype != ro0.dtype or cl.dtype != ro0.dtype or ro.shape[-1] != ro0.shape[-1] or cl.shape[-1] != cl0.shape[-1]:
            raise ValueError('the maps of all levels must share one dtype and one row length each')
        if ro.numel() != B * hws[l][0] * hws[l][1] * ro.shape[-1] or cl.numel() != B * hws[l][0] * hws[l][1] * cl.shape[-1]:
            raise ValueError(f'level {l}: maps {tuple(ro.shape)} / {tuple(cl.shape)} are not B = {B} images of {hws[l]}')
    A = sum(h * w for h, w in hws)
    max_det = A if max_det is None else int(max_det)
    key = (B, hws, strides, num_classes, max_det, dev.type, dev.index)
    hit = _detect_cache.get(key)
    if hit is None:
        ws_bytes = int(L.get_lib().rvt_yolox_detect_ws_bytes(B, A, num_classes)) if nl <= 8 else 0
        hit = (torch.empty(B, max_det, 7, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, max_det, dtype=torch.int32, device=dev), torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev),
               (ctypes.c_int * (2 * nl))(*[v for hw in hws for v in hw]), (ctypes.c_int * nl)(*strides))
        _detect_cache[key] = hit
    det, count, aidx, ws, hw_arr, st_arr = hit
    if out is not None:
        det, count, aidx = _check_out(out, B, max_det, dev)
    ro_arr = (ctypes.c_void_p * nl)(*[L.ptr(maps[2 * l]) for l in range(nl)])
    cl_arr = (ctypes.c_void_p * nl)(*[L.ptr(maps[2 * l + 1]) for l in range(nl)])
    L.call('rvt_yolox_detect', ro_arr, cl_arr, ro0.shape[-1], cl0.shape[-1], L.dtype_code(ro0.dtype), hw_arr, st_arr, nl, B, A, num_classes,
           float(conf_thre), float(nms_thre), int(bool(class_agnostic)), max_det, L.ptr(det), L.ptr(count), L.ptr(aidx), L.ptr(ws),
           ws.numel(), L.stream_of(ro0))
    return det, count, aidx


def postprocess(prediction: Tensor, num_classes: int, conf_thre: float = 0.7, nms_thre: float = 0.45,
                class_agnostic: bool = False) -> List[Optional[Tensor]]:
    """The reference's postprocess: one [n][7] tensor per image (None where nothing is detected).  max_det = A, so nothing is
    ever truncated; one read-back of the counts for the whole batch."""
    det, count, _ = postprocess_padded(prediction, num_classes, conf_thre, nms_thre, class_agnostic)
    counts = count.tolist()
    return [det[b, :n].clone() if n > 0 else None for b, n in enumerate(counts)]
