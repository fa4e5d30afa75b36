"""Plain-torch restatement of the detection post-processing semantics (include/rvt_hip.h, rvt_yolox_postprocess), with every
ordering rule explicit: stable descending sort (the lower anchor first on an exact score tie), the lowest class index on an exact
class tie, IoU = inter / (area_a + area_b - inter) in fp32 in this order, a pair whose union is not positive never suppresses.

TEST INFRASTRUCTURE: the property tests compare the kernels with it on shapes that have no recorded fixture, and
profiles/bench_postprocess.py times it as the baseline - a per-image loop with boolean-mask indexing, the all-pairs IoU matrix on
the tensors' device and the greedy pass over its rows on the host: what a user without torchvision can write today."""
from typing import List, Optional, Tuple

import numpy as np
import torch

Tensor = torch.Tensor


def class_max(cls: Tensor) -> Tuple[Tensor, Tensor]:
    """max over the class columns and the LOWEST index that attains it."""
    conf = cls.max(dim=1).values
    nc = cls.shape[1]
    idx = torch.where(cls == conf[:, None], torch.arange(nc, device=cls.device)[None, :], nc).min(dim=1).values
    return conf, idx


def suppression_matrix(boxes: Tensor, cls: Tensor, nms_thre: float, class_agnostic: bool) -> Tensor:
    """[n][n] bool: row i suppresses column j (boxes in sorted order; only j > i is meaningful)."""
    x1, y1, x2, y2 = boxes.unbind(1)
    area = (x2 - x1) * (y2 - y1)
    zero = torch.zeros((), dtype=boxes.dtype, device=boxes.device)
    rows = []
    for i0 in range(0, boxes.shape[0], 1024):
        s = slice(i0, i0 + 1024)
        iw = torch.maximum(zero, torch.minimum(x2[s, None], x2[None, :]) - torch.maximum(x1[s, None], x1[None, :]))
        ih = torch.maximum(zero, torch.minimum(y2[s, None], y2[None, :]) - torch.maximum(y1[s, None], y1[None, :]))
        inter = iw * ih
        union = area[s, None] + area[None, :] - inter
        m = (union > 0) & (inter / union > nms_thre)
        if not class_agnostic:
            m &= cls[s, None] == cls[None, :]
        rows.append(m)
    return torch.cat(rows)


def greedy_keep(sup: Tensor) -> np.ndarray:
    """Greedy pass in sorted order over the suppression matrix: indices kept."""
    s = sup.cpu().numpy()
    n = s.shape[0]
    alive = np.ones(n, dtype=bool)
    for i in range(n):
        if alive[i]:
            alive[i + 1:] &= ~s[i, i + 1:]
    return np.nonzero(alive)[0]


def postprocess_image(image_pred: Tensor, num_classes: int, conf_thre: float, nms_thre: float, class_agnostic: bool):
    """One image [A][5+nc] -> (rows [n][7], source anchors [n]) in descending score order."""
    p = image_pred.float()
    half_w, half_h = p[:, 2] / 2, p[:, 3] / 2
    boxes = torch.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h], dim=1)
    conf, cls = class_max(p[:, 5:5 + num_classes])
    score = p[:, 4] * conf
    cand = torch.nonzero(score >= conf_thre).squeeze(1)                     # ascending anchor index
    order = torch.sort(score[cand], descending=True, stable=True).indices    # stable: equal scores keep the anchor order
    cand = cand[order]
    if cand.numel():
        keep = torch.as_tensor(greedy_keep(suppression_matrix(boxes[cand], cls[cand], nms_thre, class_agnostic)), device=p.device)
        cand = cand[keep]
    rows = torch.cat([boxes[cand], p[cand, 4:5], conf[cand, None], cls[cand, None].float()], dim=1)
    return rows, cand


def postprocess_ref(prediction: Tensor, num_classes: int, conf_thre: float = 0.7, nms_thre: float = 0.45,
                    class_agnostic: bool = False, with_anchors: bool = False):
    """List of [n][7] rows per image, None for an image without detections (and the source anchors with with_anchors)."""
    out: List[Optional[Tensor]] = []
    anchors: List[Optional[Tensor]] = []
    for image_pred in prediction:
        rows, idx = postprocess_image(image_pred, num_classes, conf_thre, nms_thre, class_agnostic)
        out.append(rows if rows.shape[0] else None)
        anchors.append(idx if rows.shape[0] else None)
    return (out, anchors) if with_anchors else out
