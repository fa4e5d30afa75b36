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

Differences to the reference a caller can see: the input is NOT overwritten with corner boxes (the reference mutates
prediction[:, :, :4] in place); non-fp32 or non-contiguous input is converted first; exact score ties are ordered by anchor
index and exact class ties go to the lower class (the reference leaves both to the sort / max implementation).  There is no
PyTorch fallback: a missing kernel or an unsupported shape raises with the library's message.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

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


def postprocess(prediction: Tensor, num_classes: int, conf_thre: float = 0.7, nms_thre: float = 0.45,
                class_agnostic: bool = False) -> List[Optional[Tensor]]:
    """The reference's postprocess: one [n][7] tensor per image (None where nothing is detected).  max_det = A, so nothing is
    ever truncated; one read-back of the counts for the whole batch."""
    det, count, _ = postprocess_padded(prediction, num_classes, conf_thre, nms_thre, class_agnostic)
    counts = count.tolist()
    return [det[b, :n].clone() if n > 0 else None for b, n in enumerate(counts)]
