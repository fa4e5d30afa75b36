"""Prophesee / COCO mAP evaluation of detections on the device (csrc/cocoeval.hpp, rvt_coco_match / rvt_coco_accumulate).

Mirror of the reference's validation metric (utils/evaluation/prophesee/: `PropheseeEvaluator`, the Prophesee box filter, and
the `pycocotools.COCOeval` core it hands the boxes to), the number its checkpoint callback monitors as val/AP.  The reference
copies every frame to the host, builds one Python dict per box and matches in a per-image, per-category, per-threshold Python
loop; here the output of `postprocess_padded` and the packed label rows of `augment.pack_labels` go in and nothing leaves the
device until the precision table is read back.

  * `DetectionEvaluator(dataset, downsample_by_2, num_classes=None)`: `add_frames(det, count, label_rows, label_count, t_us)`
    is ONE launch per batch of frames with no host synchronisation and appends one compact record per kept detection to device
    storage (padded per frame); `evaluate()` sorts the record keys (`torch.sort`), runs the accumulate kernels and does the ONE
    read-back of the evaluation, the table and the counters; `precision_table()`, `reset()`, `reserve()`.  The same read-back
    carries the integer table of rvt_coco_recall: `recall_table()` is COCOeval.eval['recall'], `summary()` the twelve numbers of
    COCOeval.summarize with per-class AP / AP_50 / AR_100.  `merge(other)` appends another evaluator's store (the result has the
    bits of one evaluator fed both frame lists in order) and `all_gather(group)` makes every rank of a torch.distributed group
    hold the union of the ranks' stores in rank order, with fixed-size collectives only.
  * `PropheseeEvaluator(dataset, downsample_by_2)`: the reference's surface (LABELS, PREDICTIONS, add_labels, add_predictions,
    reset_buffer, has_data, evaluate_buffer) over the same kernels, fed with the reference's BBOX_DTYPE structured arrays.

Semantics are the reference's, quirks included: the filter also drops detections, a frame that loses every label is not an
image (its detections are not false positives), the score is class_conf, every metric is 0.0 when no detection survives in any
image, and an area range or category without ground truth averages out as -1 cells do in COCOeval.summarize.  Metrics are per
rank, as in the reference, until all_gather() is called.  There is no PyTorch fallback: a missing kernel or an unsupported
shape raises with the library's message.
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


RECALL_METRICS = ('AR_1', 'AR_10', 'AR_100', 'AR_S', 'AR_M', 'AR_L')
SUMMARY_KEYS = METRICS + RECALL_METRICS           # COCOeval.summarize's stats[0..11]


def _mean_cells(s: np.ndarray) -> float:
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def summarize_recall(recall: np.ndarray) -> Dict[str, float]:
    """COCOeval.summarize's numbers 7-12 from recall [10][K][4][3]: the mean over the cells > -1, or -1."""
    return {'AR_1': _mean_cells(recall[:, :, 0, 0]), 'AR_10': _mean_cells(recall[:, :, 0, 1]), 'AR_100': _mean_cells(recall[:, :, 0, 2]),
            'AR_S': _mean_cells(recall[:, :, 1, 2]), 'AR_M': _mean_cells(recall[:, :, 2, 2]), 'AR_L': _mean_cells(recall[:, :, 3, 2])}


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
        self._last_recall: Optional[Dict[str, np.ndarray]] = None    # read back with _last, valid while _last is

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
        out = torch.empty(10 * 101 * K * 4 + N_COUNTERS + 3 * K * 40, dtype=torch.float64, device=self._dev)
        L.call('rvt_coco_accumulate', L.ptr(perm), L.ptr(matched), L.ptr(ignored), n, K, L.ptr(self._counters),
               L.ptr(self._thr[10:]), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_of(out))
        out[10 * 101 * K * 4:10 * 101 * K * 4 + N_COUNTERS].copy_(self._counters)
        out[10 * 101 * K * 4 + N_COUNTERS:].copy_(self._recall_tp().reshape(-1))     # integers far below 2^53: exact as doubles
        host = out.cpu().numpy()                                         # the one read-back
        c = host[10 * 101 * K * 4:10 * 101 * K * 4 + N_COUNTERS].astype(np.int64)
        tp = host[10 * 101 * K * 4 + N_COUNTERS:].astype(np.int64).reshape(3, K, 10, 4)
        self._last = {'precision': host[:10 * 101 * K * 4].reshape(10, 101, K, 4).copy(), 'npig': c[:4 * K].reshape(K, 4),
                      'records': c[64:64 + K], 'images': int(c[80]), 'images_with_detections': int(c[81]), 'truncated_frames': int(c[82])}
        npig = self._last['npig'][None, :, None, :]                      # [1][K][1][4] against tp [3][K][10][4]
        recall = np.where(npig > 0, tp / np.maximum(npig, 1), -1.0)      # one double division per cell, as COCOeval's tp_sum[-1] / npig
        self._last_recall = {'tp': tp, 'recall': np.ascontiguousarray(recall.transpose(2, 1, 3, 0))}
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

    # ---- recall and the full summary ----------------------------------------------------------------------------------------
    def _recall_tp(self) -> Tensor:
        """int64 [3][num_classes][40] on the device: the true positives with rank < 1, 10, 100 inside their (frame, category)
        list, one rvt_coco_recall launch per run of add_frames calls with the same slots per frame.  No host synchronisation."""
        K = self.num_classes
        tp = torch.zeros(3, K, 40, dtype=torch.int64, device=self._dev)
        runs: List[List[int]] = []
        for first, F, R in self._spans:
            if runs and runs[-1][2] == R and runs[-1][0] + runs[-1][1] * R == first and runs[-1][1] + F <= 0x7fffffff:
                runs[-1][1] += F
            else:
                runs.append([first, F, R])
        for first, F, R in runs:
            key, matched, ignored = (self._planes[i, first:first + F * R] for i in range(3))
            L.call('rvt_coco_recall', L.ptr(key), L.ptr(matched), L.ptr(ignored), F, R, K, L.ptr(tp), L.stream_of(tp))
        return tp

    def recall_table(self) -> np.ndarray:
        """COCOeval.eval['recall']: double [10 IoU thresholds][num_classes][4 area ranges][3 maxDets = 1, 10, 100]; -1 where the
        cell has no non-ignored ground truth, else true positives / npig (one double division)."""
        self._run()
        return self._last_recall['recall']

    def recall_counts(self) -> np.ndarray:
        """The numerators of recall_table(): int64 [3 maxDets][num_classes][10][4], the table rvt_coco_recall filled."""
        self._run()
        return self._last_recall['tp']

    def summary(self) -> Dict[str, Any]:
        """The twelve numbers of COCOeval.summarize in its order (SUMMARY_KEYS), `per_class` (a list of {'AP', 'AP_50', 'AR_100'},
        one entry per class) and truncated_frames.  Each number is the mean over the cells > -1, or -1; all of them are 0.0 when
        no detection survives in any image, the rule of evaluate()."""
        r = self._run()
        K = self.num_classes
        if r['images_with_detections'] > 0:
            p, rc = r['precision'], self._last_recall['recall']
            out: Dict[str, Any] = dict(summarize(p), **summarize_recall(rc))
            out['per_class'] = [{'AP': _mean_cells(p[:, :, k, 0]), 'AP_50': _mean_cells(p[0, :, k, 0]), 'AR_100': _mean_cells(rc[:, k, 0, 2])}
                                for k in range(K)]
        else:
            out = {k: 0.0 for k in SUMMARY_KEYS}
            out['per_class'] = [{'AP': 0.0, 'AP_50': 0.0, 'AR_100': 0.0} for _ in range(K)]
        out['truncated_frames'] = r['truncated_frames']
        return out

    # ---- several evaluators, one result ------------------------------------------------------------------------------------
    def merge(self, other: 'DetectionEvaluator') -> None:
        """Append `other`'s store to this one: afterwards this evaluator answers as one that was given its own frames and then
        `other`'s, bit for bit (an exact score tie goes to the earlier arrival: this evaluator's records first).  `other` is left
        as it is.  Raises ValueError, before anything is touched, unless dataset, downsample_by_2, num_classes and device agree.
        No host synchronisation beyond what reserve() does."""
        if not isinstance(other, DetectionEvaluator):
            raise ValueError(f'merge() takes a DetectionEvaluator, got {type(other).__name__}')
        if other is self:
            raise ValueError('merge(): an evaluator cannot be merged into itself')
        for name in ('dataset', 'downsample_by_2', 'num_classes'):
            if getattr(self, name) != getattr(other, name):
                raise ValueError(f'merge(): {name} differs: {getattr(self, name)!r} here, {getattr(other, name)!r} there')
        if self._dev is not None and other._dev is not None and self._dev != other._dev:
            raise ValueError(f'merge(): this evaluator holds records on {self._dev}, the other on {other._dev}')
        if other._dev is None:                                           # never saw a tensor: holds nothing
            return
        self._bind(other._dev)
        n0, n1 = self._n, other._n
        self.reserve(n0 + n1)
        self._planes[:, n0:n0 + n1].copy_(other._planes[:, :n1])
        self._counters += other._counters
        self._spans += [(n0 + first, F, R) for first, F, R in other._spans]
        self._n += n1
        self._frames += other._frames
        self._last = None

    def all_gather(self, group=None) -> None:
        """Every rank of `group` ends up holding the union of the ranks' stores in rank order, as if rank 0's evaluator had
        merged rank 1's, then rank 2's, ...: by the contract of merge() every rank then returns identical results.  Collective:
        every rank of the group must call it, a rank that holds nothing included.  Fixed-size collectives only: an all_gather of
        five int64 sizes, all_gathers of the record planes and the span rows padded to the largest rank, an all_reduce of the
        counters.  Raises ValueError on every rank, before the store is touched, when the ranks' settings differ."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError('all_gather() needs an initialised torch.distributed process group')
        world = dist.get_world_size(group)
        if self._dev is None:                                            # this rank never saw a tensor: take the backend's device
            nccl = 'nccl' in str(dist.get_backend(group))
            self._bind(torch.device('cuda', torch.cuda.current_device()) if nccl else torch.device('cpu'))
        dev, n = self._dev, self._n
        sizes = torch.tensor([n, len(self._spans), self.num_classes, self.min_diag, self.min_side], dtype=torch.int64).to(dev)
        all_sizes = [torch.empty_like(sizes) for _ in range(world)]
        dist.all_gather(all_sizes, sizes, group=group)
        all_sizes = torch.stack(all_sizes).cpu().tolist()
        for r, s in enumerate(all_sizes):
            if s[2:] != all_sizes[0][2:]:
                raise ValueError(f'all_gather(): rank {r} evaluates (num_classes, min_diag, min_side) = {tuple(s[2:])}, '
                                 f'rank 0 {tuple(all_sizes[0][2:])}')
        max_n, max_s = max(1, max(s[0] for s in all_sizes)), max(1, max(s[1] for s in all_sizes))
        planes = torch.zeros(3, max_n, dtype=torch.int64, device=dev)
        planes[:, :n].copy_(self._planes[:, :n])
        spans = torch.zeros(max_s, 3, dtype=torch.int64)
        if self._spans:
            spans[:len(self._spans)] = torch.tensor(self._spans, dtype=torch.int64)
        spans = spans.to(dev)
        all_planes = [torch.empty_like(planes) for _ in range(world)]
        all_spans = [torch.empty_like(spans) for _ in range(world)]
        dist.all_gather(all_planes, planes, group=group)
        dist.all_gather(all_spans, spans, group=group)
        dist.all_reduce(self._counters, op=dist.ReduceOp.SUM, group=group)
        span_rows = torch.stack(all_spans).cpu().tolist()
        store = torch.empty(3, sum(s[0] for s in all_sizes), dtype=torch.int64, device=dev)
        at, merged, frames = 0, [], 0
        for r, s in enumerate(all_sizes):
            store[:, at:at + s[0]].copy_(all_planes[r][:, :s[0]])
            for first, F, R in span_rows[r][:s[1]]:
                merged.append((at + first, F, R))
                frames += F
            at += s[0]
        self._planes, self._n, self._spans, self._frames, self._last = store, at, merged, frames, None


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
