"""YoloXDetector: recurrent backbone + YOLOX PAFPN + YOLOX head as one module - the object a user of the model starts from.

Mirror of the reference class (models/detection/yolox_extension/models/detector.py:18-72): the same constructor argument (the
`model` config tree with its `backbone`, `fpn` and `head` sections), the same sub-module names (`backbone`, `fpn`, `yolox_head`), so
`state_dict()` has the reference's names, shapes and order and a reference checkpoint loads with strict=True; the same
`forward_backbone`, `forward_detect` and `forward` with their return contracts.  The three parts are this package's own
(build_recurrent_backbone, build_yolox_fpn, build_yolox_head): HIP kernels end to end, no registry of the reference involved.

Beyond the reference:
  * `forward_sequence(xs, previous_states, token_masks)`: the backbone's whole-sequence form (rvt_amd/backbone.py);
  * `detect(x, previous_states, conf_thre, nms_thre, ...) -> ((det, count, anchor_idx), states)`: one streaming inference step from
    the event frame to the kept boxes under no_grad - backbone, PAFPN, the head's prediction maps, then decode + score filter + NMS
    as one launch (YOLOXHead.detect_padded) - with no host synchronisation; rvt_amd.graph.GraphedDetectorStream replays it as one
    hipGraph launch.
The config keys `impl` (which registry branch a reference-side maintainer routes to) and `compile` (torch.compile
settings of the reference; nothing is traced here) are accepted and ignored.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from .backbone import build_recurrent_backbone
from .config import AttrDict
from .fpn import build_yolox_fpn
from .head import build_yolox_head
from .types import BackboneFeatures, LstmStates

Tensor = torch.Tensor


def _section(cfg, name: str):
    """cfg.name of a dict / AttrDict / DictConfig / attribute object, as a plain dict without the keys nothing here reads."""
    sec = cfg[name] if isinstance(cfg, dict) or hasattr(cfg, '__getitem__') else getattr(cfg, name)
    items = sec.items() if hasattr(sec, 'items') else vars(sec).items()
    return {k: v for k, v in items if k not in ('impl', 'compile')}


class YoloXDetector(nn.Module):
    def __init__(self, model_cfg, compute_dtype: torch.dtype = torch.float32):
        super().__init__()
        backbone_cfg, fpn_cfg, head_cfg = (_section(model_cfg, k) for k in ('backbone', 'fpn', 'head'))
        self.compute_dtype = compute_dtype
        self.backbone = build_recurrent_backbone(AttrDict(backbone_cfg), compute_dtype=compute_dtype)
        in_stages = tuple(fpn_cfg['in_stages'])
        in_channels = self.backbone.get_stage_dims(in_stages)
        self.fpn = build_yolox_fpn(fpn_cfg, in_channels=in_channels, compute_dtype=compute_dtype)
        strides = self.backbone.get_strides(in_stages)
        self.yolox_head = build_yolox_head(head_cfg, in_channels=in_channels, strides=strides, compute_dtype=compute_dtype)

    def invalidate_weight_cache(self) -> None:
        """Force a rebuild of the kernel-side weight copies of all three parts on their next forward (call after writing parameters or
        buffers through ``.data`` in inference code)."""
        for part in (self.backbone, self.fpn, self.yolox_head):
            part.invalidate_weight_cache()

    def weight_caches(self) -> list:
        """The kernel-side buffers and tables the last forward used: a captured graph addresses them by raw pointer and keeps them."""
        return [c for part in (self.backbone, self.fpn, self.yolox_head) for c in part.weight_caches()]

    # ---- reference API ------------------------------------------------------------------------------
    def forward_backbone(self, x: Tensor, previous_states: Optional[LstmStates] = None, token_mask: Optional[Tensor] = None) \
            -> Tuple[BackboneFeatures, LstmStates]:
        return self.backbone(x, previous_states, token_mask)

    def forward_detect(self, backbone_features: BackboneFeatures, targets: Optional[Tensor] = None) \
            -> Tuple[Tensor, Union[Dict[str, Tensor], None]]:
        fpn_features = self.fpn(backbone_features)
        if self.training:
            assert targets is not None
            return self.yolox_head(fpn_features, targets)
        outputs, losses = self.yolox_head(fpn_features)
        assert losses is None
        return outputs, losses

    def forward(self, x: Tensor, previous_states: Optional[LstmStates] = None, retrieve_detections: bool = True,
                targets: Optional[Tensor] = None) -> Tuple[Union[Tensor, None], Union[Dict[str, Tensor], None], LstmStates]:
        backbone_features, states = self.forward_backbone(x, previous_states)
        outputs, losses = None, None
        if not retrieve_detections:
            assert targets is None
            return outputs, losses, states
        outputs, losses = self.forward_detect(backbone_features=backbone_features, targets=targets)
        return outputs, losses, states

    # ---- beyond the reference -----------------------------------------------------------------------
    def forward_sequence(self, xs, previous_states: Optional[LstmStates] = None, token_masks: Optional[Tensor] = None):
        """xs (T, B, Cin, h, w) or a list of T frames -> ({stage: (T, B, C, H, W)}, states): RNNDetector.forward_sequence."""
        return self.backbone.forward_sequence(xs, previous_states, token_masks)

    @torch.no_grad()
    def detect(self, x: Tensor, previous_states: Optional[LstmStates], conf_thre: float, nms_thre: float, class_agnostic: bool = False,
               max_det: Optional[int] = None, out=None):
        """One eval-mode step, frame to kept boxes: ((det [B][max_det][7], count [B], anchor_idx [B][max_det]), states), equal to
        postprocess_padded(self(x, previous_states)[0], ...) bit for bit, with no host synchronisation.  det / count / anchor_idx are
        `out` or the tensors cached for this shape (rvt_amd.postprocess.detect_padded: overwritten by the next call)."""
        assert not self.training, 'detect is the inference step: call .eval() first'
        backbone_features, states = self.backbone(x, previous_states)
        dets = self.yolox_head.detect_padded(self.fpn(backbone_features), conf_thre, nms_thre, class_agnostic, max_det, out)
        return dets, states
