"""Prophesee / COCO mAP evaluation of detections on the device (csrc/cocoeval.hpp, rvt_coco_match / rvt_coco_accumulate).

Mirror of the reference's validation metric (utils/evaluation/prophesee/: `PropheseeEvaluator`, the Prophesee box filter, and
the `pycocotools.COCOeval` core it hands the boxes to), the number its checkpoint callback monitors as val/AP.  The reference
copies every frame to the host, builds one Python dict per box and matches in a per-image, per-category, per-threshold Python
loop; here the output of `postprocess_padded` and the packed label rows of `augment.pack_labels` go in and nothing leaves the
device until the precision table is read back.

  * `DetectionEvaluator(dataset, downsample_by_2, num_classes=None)`: `add_frames(det, count, label_rows, label_count, t_us)`
    is ONE launch per batch of frames with no host synchronisation and appends one compact record per kept detection to device
    storage (padded per frame); `evaluate()` sorts the record keys (`torch.sort`), runs the accumulate kernels and does the ONE
    read-back of the evaluation, the table and the counters; `precision_table()`, `reset()`, `reserve()`.
  * `PropheseeEvaluator(dataset, downsample_by_2)`: the reference's surface (LABELS, PREDICTIONS, add_labels, add_predictions,
    reset_buffer, has_data, evaluate_buffer) over the same kernels, fed with the reference's BBOX_DTYPE structured arrays.

Semantics are the reference's, quirks included: the filter also drops detections, a frame that loses every label is not an
image (its detections are not false positives), the score is class_conf, every metric is 0.0 when no detection survives in any
image, and an area range or category without ground truth averages out as -1 cells do in COCOeval.summarize.  Metrics are per
rank, as in the reference.  There is no PyTorch fallback: a missing kernel or an unsupported shape raises with the library's
message.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional
from warnings import warn

import numpy as np
import torch

from . import _lib as L

Tensor = torch.Tensor

METRICS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # COCOeval Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
assert IOU_THRS[0] == 0.5 and IOU_THRS[5] == 0.75
DATASET_CLASSES = {'gen1': 2, 'gen4': 3}          # evaluation.py:15-18: (car, pedestrian) / (pedestrian, two-wheeler, car)
TOP = 100                                         # COCOeval maxDets[-1]
N_COUNTERS = 96                                   # include/rvt_hip.h: npig at 4k + a, records at 64 + k, images 80, with dets 81, truncated 82
NO_RECORD = 0x7fffffffffffffff

# the reference's box record (io/box_loading.py BBOX_DTYPE)
BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})


def filter_constants(dataset: str, downsample_by_2: bool):
    """(min_box_diag, min_box_side) of evaluation.py:22-31."""
    if dataset not in DATASET_CLASSES:
        raise ValueError(f"dataset must be 'gen1' or 'gen4', got {dataset!r}")
    diag, side = (60, 20) if dataset == 'gen4' else (30, 10)
    return (diag // 2, side // 2) if downsample_by_2 else (diag, side)


def summarize(precision: np.ndarray) -> Dict[str, float]:
    """COCOeval.summarize's first six numbers from precision [10][101][K][4]: the mean over the cells > -1, or -1."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    return {'AP': mean(precision[:, :, :, 0]), 'AP_50': mean(precision[0, :, :, 0]), 'AP_75': mean(precision[5, :, :, 0]),
            'AP_S': mean(precision[:, :, :, 1]), 'AP_M': mean(precision[:, :, :, 2]), 'AP_L': mean(precision[:, :, :, 3])}


class DetectionEvaluator:
    def __init__(self, dataset: str, downsample_by_2: bool, num_classes: Optional[int] = None):
        self.dataset, self.downsample_by_2 = dataset, bool(downsample_by_2)
        self.min_diag, self.min_side = filter_constants(dataset, downsample_by_2)
        self.num_classes = DATASET_CLASSES[dataset] if num_classes is None else int(num_classes)
        if self.num_classes < 1:
            raise ValueError(f'num_classes={self.num_classes} must be positive')
        self._dev: Optional[torch.device] = None
        self._planes: Optional[Tensor] = None        # int64 [3][capacity]: key, matched, ignored
        self._n = 0                                  # record slots in use
        self._frames = 0
        self._spans: List[tuple] = []                # (first slot, frames, slots per frame) of every add_frames call
        self._counters: Optional[Tensor] = None
        self._thr: Optional[Tensor] = None           # the two threshold tables, double [10 + 101]
        self._last: Optional[Dict[str, Any]] = None

    # ---- storage ------------------------------------------------------------------------------------------------------------
    def _bind(self, dev: torch.device) -> None:
        if self._dev is None:
            self._dev = dev
            self._counters = torch.zeros(N_COUNTERS, dtype=torch.int32, device=dev)
            self._thr = torch.from_numpy(np.concatenate([IOU_THRS, REC_THRS])).to(dev)
            self._planes = torch.empty(3, 0, dtype=torch.int64, device=dev)
        elif dev != self._dev:
            raise ValueError(f'this evaluator holds records on {self._dev}, got tensors on {dev}')

    def reserve(self, slots: int, device=None) -> None:
        """Make room for `slots` record slots (add_frames uses frames * min(max_det, 100 * num_classes) per call), so that later
        calls allocate nothing: needed before add_frames is captured in a torch.cuda.graph."""
        if device is not None:
            self._bind(torch.device(device))
        if self._planes is None:
            raise ValueError('reserve() before the first add_frames() needs the device')
        if slots > self._planes.shape[1]:
            grown = torch.empty(3, max(int(slots), 2 * self._planes.shape[1]), dtype=torch.int64, device=self._dev)
            if self._n:
                grown[:, :self._n].copy_(self._planes[:, :self._n])
            self._planes = grown

    def reset(self) -> None:
        """Forget every frame (the storage is kept).  No host synchronisation."""
        self._n, self._frames, self._last, self._spans = 0, 0, None, []
        if self._counters is not None:
            self._counters.zero_()

    def invalidate(self) -> None:
        """Drop the cached result of the last evaluation: call after replaying a graph that holds add_frames, which rewrites
        the store without the host's knowledge."""
        self._last = None

    @property
    def frames(self) -> int:
        return self._frames

    @property
    def slots(self) -> int:
        """Record slots in use (24 bytes each): frames * min(max_det, 100 * num_classes) summed over the add_frames calls."""
        return self._n

    # ---- per batch ----------------------------------------------------------------------------------------------------------
    def add_frames(self, det: Tensor, count: Tensor, label_rows: Tensor, label_count: Tensor, t_us: Tensor, det_xywh: bool = False) -> None:
        """det fp32 [F][max_det][7] and count int32 [F] as postprocess_padded returns them; label_rows fp32 [F][G][7]
        (t x y w h class_id class_confidence) and label_count int32 [F] (-1 or 0: no labels) as augment.pack_labels lays them
        out (leading [T][B] dimensions are flattened); t_us int64 [F], one timestamp per frame.  One launch, no host
        synchronisation.  det_xywh: columns 0..3 of det are x y w h instead of the corners."""
        if det.dim() != 3 or det.shape[2] != 7:
            raise ValueError(f'det must be [F][max_det][7], got {tuple(det.shape)}')
        F, max_det, _ = det.shape
        if label_rows.dim() >= 3 and label_rows.shape[-1] == 7:
            label_rows = label_rows.reshape(-1, label_rows.shape[-2], 7)
        if label_rows.dim() != 3 or label_rows.shape[0] != F or label_rows.shape[2] != 7:
            raise ValueError(f'label_rows must be [F = {F}][G][7], got {tuple(label_rows.shape)}')
        G = label_rows.shape[1]
        count, label_count, t_us = count.reshape(-1), label_count.reshape(-1), t_us.reshape(-1)
        for name, t, dt in (('count', count, torch.int32), ('label_count', label_count, torch.int32), ('t_us', t_us, torch.int64)):
            if t.numel() != F or t.dtype != dt:
                raise ValueError(f'{name} must be {dt} [F = {F}], got {t.dtype} {tuple(t.shape)}')
        if F == 0:
            raise ValueError('add_frames: no frame')
        if det.dtype != torch.float32 or label_rows.dtype != torch.float32:
            raise ValueError(f'det and label_rows must be float32, got {det.dtype} and {label_rows.dtype}')
        for t in (count, label_rows, label_count, t_us):
            if t.device != det.device:
                raise ValueError(f'every tensor must be on {det.device}, got one on {t.device}')
        self._bind(det.device)
        det, label_rows = det.detach().contiguous(), label_rows.contiguous()
        K = self.num_classes
        R = min(max_det, TOP * K)
        self.reserve(self._n + F * R)
        key, matched, ignored = (self._planes[i, self._n:self._n + F * R] for i in range(3))
        L.call('rvt_coco_match', L.ptr(det), L.ptr(count), L.ptr(label_rows), L.ptr(label_count), L.ptr(t_us), F, max_det, G, K,
               int(bool(det_xywh)), float(self.min_diag), float(self.min_side), L.ptr(self._thr), L.ptr(key), L.ptr(matched),
               L.ptr(ignored), R, L.ptr(self._counters), L.stream_of(det))
        self._spans.append((self._n, F, R))
        self._n += F * R
        self._frames += F
        self._last = None

    # ---- per evaluation -----------------------------------------------------------------------------------------------------
    def _run(self) -> Dict[str, Any]:
        if self._last is not None:
            return self._last
        if self._dev is None:
            raise RuntimeError('evaluate() before any add_frames(): the evaluator holds no frame')
        K, n = self.num_classes, self._n
        key, matched, ignored = (self._planes[i, :n] for i in range(3))
        perm = torch.sort(key, stable=True)[1]                           # (category, descending score, arrival order)
        ws = torch.empty(max(int(L.get_lib().rvt_coco_accumulate_ws_bytes(n, K)), 1), dtype=torch.uint8, device=self._dev)
        out = torch.empty(10 * 101 * K * 4 + N_COUNTERS, dtype=torch.float64, device=self._dev)
        L.call('rvt_coco_accumulate', L.ptr(perm), L.ptr(matched), L.ptr(ignored), n, K, L.ptr(self._counters),
               L.ptr(self._thr[10:]), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_of(out))
        out[10 * 101 * K * 4:].copy_(self._counters)
        host = out.cpu().numpy()                                         # the one read-back
        c = host[10 * 101 * K * 4:].astype(np.int64)
        self._last = {'precision': host[:10 * 101 * K * 4].reshape(10, 101, K, 4).copy(), 'npig': c[:4 * K].reshape(K, 4),
                      'records': c[64:64 + K], 'images': int(c[80]), 'images_with_detections': int(c[81]), 'truncated_frames': int(c[82])}
        return self._last

    def precision_table(self) -> np.ndarray:
        """COCOeval.eval['precision'] at maxDets = 100: double [10 IoU thresholds][101 recall levels][num_classes][4 area ranges]."""
        return self._run()['precision']

    def counts(self) -> Dict[str, Any]:
        """npig [K][4], records [K], images, images_with_detections, truncated_frames of the frames added so far."""
        return {k: v for k, v in self._run().items() if k != 'precision'}

    def records(self) -> Dict[str, np.ndarray]:
        """Inspection surface (copies the store to the host): per record, in storage order, the frame (in add_frames order),
        the category, the fp32 score, and the matched / ignored masks (bit 4 * threshold + area range)."""
        frame, f0 = [np.zeros(0, np.int64)], 0
        for _, F, R in self._spans:
            frame.append(f0 + np.repeat(np.arange(F), R))
            f0 += F
        frame = np.concatenate(frame)
        key, matched, ignored = self._planes[:, :self._n].cpu().numpy()
        used = key != NO_RECORD
        key = key[used]
        bits = (~key & 0xffffffff).astype(np.uint32)
        bits = np.where(bits & 0x80000000, bits & 0x7fffffff, ~bits).astype(np.uint32)
        return {'frame': frame[used], 'category': (key >> 32).astype(np.int64), 'score': bits.view(np.float32),
                'matched': matched[used], 'ignored': ignored[used]}

    def evaluate(self) -> Dict[str, float]:
        """The six numbers of the reference's evaluate_list plus truncated_frames (frames whose count exceeded max_det: their
        tail was not scored).  All six are 0.0 when no detection survives in any image (coco_eval.py:112-115)."""
        r = self._run()
        out = summarize(r['precision']) if r['images_with_detections'] > 0 else {k: 0.0 for k in METRICS}
        out['truncated_frames'] = r['truncated_frames']
        return out


class PropheseeEvaluator:
    """The reference's utils/evaluation/prophesee/evaluator.py surface over the device kernels.  Entry i of the labels pairs
    with entry i of the predictions; every entry is one frame (one distinct 't', as the reference's to_prophesee asserts)."""
    LABELS = 'lables'
    PREDICTIONS = 'predictions'
    BATCH = 256                                      # frames per launch

    def __init__(self, dataset: str, downsample_by_2: bool, device=None):
        assert dataset in {'gen1', 'gen4'}
        self.dataset = dataset
        self.downsample_by_2 = downsample_by_2
        self.device = device
        self._buffer = None
        self._buffer_empty = True
        self._reset_buffer()

    def _reset_buffer(self):
        self._buffer_empty = True
        self._buffer = {self.LABELS: list(), self.PREDICTIONS: list()}

    def _add_to_buffer(self, key: str, value: List[np.ndarray]):
        assert isinstance(value, list)
        for entry in value:
            assert isinstance(entry, np.ndarray)
        self._buffer_empty = False
        self._buffer[key].extend(value)

    def add_predictions(self, predictions: List[np.ndarray]):
        self._add_to_buffer(self.PREDICTIONS, predictions)

    def add_labels(self, labels: List[np.ndarray]):
        self._add_to_buffer(self.LABELS, labels)

    def reset_buffer(self) -> None:
        self._reset_buffer()

    def has_data(self):
        return not self._buffer_empty

    def evaluate_buffer(self, img_height: int, img_width: int) -> Optional[Dict[str, Any]]:
        if self._buffer_empty:
            warn("Attempt to use prophesee evaluation buffer, but it is empty", UserWarning, stacklevel=2)
            return
        labels, predictions = self._buffer[self.LABELS], self._buffer[self.PREDICTIONS]
        assert len(labels) == len(predictions)
        dev = torch.device(self.device) if self.device is not None else \
            (torch.device('cpu') if L.is_emulator() else torch.device('cuda', torch.cuda.current_device()))
        frames = []
        for lab, pred in zip(labels, predictions):
            ts = np.unique(np.concatenate([lab['t'], pred['t']]))
            if ts.size > 1:
                raise NotImplementedError(f'an entry with {ts.size} distinct timestamps: every entry must be one frame')
            if lab.size:                                                  # an entry without labels is never an image
                frames.append((lab, pred, int(ts[0])))
        ev = DetectionEvaluator(self.dataset, self.downsample_by_2)
        ev._bind(dev)
        for i in range(0, len(frames), self.BATCH):
            part = frames[i:i + self.BATCH]
            F, G, D = len(part), max(f[0].size for f in part), max(1, max(f[1].size for f in part))
            rows, det = np.zeros((F, G, 7), dtype=np.float32), np.zeros((F, D, 7), dtype=np.float32)
            lcount, count, t_us = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int64)
            for j, (lab, pred, t) in enumerate(part):
                for c, name in enumerate(('x', 'y', 'w', 'h', 'class_id', 'class_confidence')):
                    rows[j, :lab.size, 1 + c] = lab[name]
                for c, name in ((0, 'x'), (1, 'y'), (2, 'w'), (3, 'h'), (5, 'class_confidence'), (6, 'class_id')):
                    det[j, :pred.size, c] = pred[name]
                lcount[j], count[j], t_us[j] = lab.size, pred.size, t
            ev.add_frames(*(torch.from_numpy(a).to(dev) for a in (det, count, rows, lcount, t_us)), det_xywh=True)
        if not frames:
            return {k: 0.0 for k in METRICS}
        out = ev.evaluate()
        del out['truncated_frames']                   # D is the largest entry: nothing is ever truncated
        return out
