"""Epoch loader over the sparse frame cache: which T windows of which recording form sample b of the next batch, which samples
start a sequence, how a stream is carried across batches, padded and split over ranks -- and the batch itself, made on the device
from the packed store in one launch (framecache.unpack_augment) plus one for the labels (augment.augment_labels).

Host-side Python without per-pixel work and without worker processes.  It restates, on integer arrays, the index rules of the
reference's data/genx_utils/{sequence_rnd, sequence_for_streaming, dataset_rnd, dataset_streaming}.py,
data/utils/stream_{concat, sharded}_datapipe.py and modules/data/genx.py (which need h5py, torchdata and Lightning):

  * random access (sequence_rnd.py:24-50): `random_access_offset`, `random_access_item`;
  * streaming (sequence_for_streaming.py:25-54, 72-86, 141-185): `streaming_range`, `label_cluster_ranges`, `streaming_chunks`;
  * sharding of evaluation streams (stream_sharded_datapipe.py:19-67): `assign_to_worker`, `assign_to_slots`;
  * the mixed split (genx.py:116-129): `mixed_batch_split`; the weighted sampler (dataset_rnd.py:115-149): `sampler_weights`.

`SequenceStore` is one recording's built windows (a host `PackedFrames`) with its labelled frames; `BatchLoader` is iterable, one
iteration is an epoch.  A batch is {'data': {EV_REPR: (T,B,C,H,W) device tensor, OBJLABELS_SEQ: T `SparseLabels`, IS_FIRST_SAMPLE:
bool (B,), IS_PADDED_MASK: bool (T,B)}, 'worker_id': 0, 'device_labels': (rows_out, count_out, yolox, labelled)}: what
`step.BackboneSequenceModule` takes.  Under MIXED sampling the two part batches carry EV_REPR and IS_PADDED_MASK as lists over t
(views, no copy), which is the form `states.merge_mixed_batches` concatenates along the batch axis.

Out of scope: H5 / blosc reading, DataType.FLOW / IMAGE, rotation, worker processes, per-worker RNG seeds.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment as A
from . import framecache as fc
from .framecache import PackedFrames, PackedFrames2
from .types import DataType, DatasetSamplingMode, Mode

TOO_FEW_STREAMS_MSG = ("Each worker must at least get 'batch_size' number of datapipes. Otherwise, we would have to support dynamic "
                       "batch sizes. As a workaround, decrease the number of workers.")


# ---- index rules: plain functions on integer arrays ---------------------------------------------------------------------------------
def random_access_offset(objframe_idx_2_repr_idx: np.ndarray, T: int) -> int:
    """The first labelled frame whose window index is at least T - 1 (len(...) when there is none: an empty sequence)."""
    for i, r in enumerate(objframe_idx_2_repr_idx):
        if r - T + 1 >= 0:
            return i
    return len(objframe_idx_2_repr_idx)


def random_access_len(objframe_idx_2_repr_idx: np.ndarray, T: int) -> int:
    return len(objframe_idx_2_repr_idx) - random_access_offset(objframe_idx_2_repr_idx, T)


def random_access_item(objframe_idx_2_repr_idx: np.ndarray, T: int, i: int) -> Tuple[int, int]:
    """Windows [start, end) of item i: the T windows that end on labelled frame i + offset."""
    end = int(objframe_idx_2_repr_idx[i + random_access_offset(objframe_idx_2_repr_idx, T)]) + 1
    assert end - T >= 0
    return end - T, end


def streaming_range(objframe_idx_2_repr_idx: np.ndarray, N: int, T: int) -> Tuple[int, int]:
    """A whole recording as a stream: from T - 1 windows before the first label to the last window."""
    start = max(int(objframe_idx_2_repr_idx[0]) - T + 1, 0)
    assert 0 <= start < N
    return start, N


def label_cluster_ranges(objframe_idx_2_repr_idx: np.ndarray, T: int) -> List[Tuple[int, int]]:
    """_get_ev_repr_range_indices(indices, max_len=T): one range per run of labels no further than T windows apart."""
    idx = np.asarray(objframe_idx_2_repr_idx, dtype=np.int64)
    stops = np.flatnonzero(np.diff(idx) > T)
    starts = np.concatenate((np.atleast_1d(0), stops + 1))
    stops = np.concatenate((stops, np.atleast_1d(len(idx) - 1)))
    return [(max(int(idx[a]) - T + 1, 0), int(idx[b]) + 1) for a, b in zip(starts, stops)]


def streaming_chunks(start: int, stop: int, T: int) -> List[Tuple[int, int]]:
    """[start, stop) cut into chunks of T windows; the last may be shorter (it is padded)."""
    assert 0 <= start < stop
    s = list(range(start, stop, T))
    return list(zip(s, s[1:] + [stop]))


def _pyramid(n: int) -> Iterator[int]:
    while True:
        yield from range(n)
        yield from range(n - 1, -1, -1)


def assign_to_worker(lengths: Sequence[int], total_num_workers: int, global_worker_id: int) -> List[int]:
    """Positions (into `lengths`) of the streams of one worker: sorted long to short (stable), dealt out in pyramid order."""
    order = sorted(range(len(lengths)), key=lambda i: lengths[i], reverse=True)
    assert len(order) >= total_num_workers > global_worker_id, f'num_datapipes={len(order)}, {total_num_workers=}, {global_worker_id=}'
    gen = _pyramid(total_num_workers)
    return [i for i in order if next(gen) == global_worker_id]


def assign_to_slots(lengths: Sequence[int], batch_size: int) -> List[List[int]]:
    """Positions (into `lengths`) of the streams each batch slot concatenates: sorted long to short, pyramid order."""
    assert len(lengths) > 0 and batch_size > 0
    assert len(lengths) >= batch_size, TOO_FEW_STREAMS_MSG
    order = sorted(range(len(lengths)), key=lambda i: lengths[i], reverse=True)
    slots: List[List[int]] = [[] for _ in range(batch_size)]
    gen = _pyramid(batch_size)
    for i in order:
        slots[next(gen)].append(i)
    return slots


def mixed_batch_split(batch_size: int, w_random: float, w_stream: float) -> Tuple[int, int]:
    """(random, stream) batch sizes of MIXED sampling; Python's round (half to even)."""
    assert batch_size >= 2, 'Cannot use mixed mode with batch size smaller than 2'
    assert w_random > 0 and w_stream > 0
    bs_rnd = min(round(batch_size * w_random / (w_stream + w_random)), batch_size - 1)
    return bs_rnd, batch_size - bs_rnd


def sampler_weights(class_ids_per_item: Sequence[np.ndarray]) -> List[float]:
    """get_weighted_random_sampler: class weight = 1 / its count over all items; an item's weight = sum over its labels."""
    class2count: Dict[int, int] = {}
    per_item = []
    for ids in class_ids_per_item:
        c, n = np.unique(np.asarray(ids, dtype='int32'), return_counts=True)
        for k, v in zip(c, n):
            class2count[int(k)] = class2count.get(int(k), 0) + int(v)
        per_item.append((c, n))
    class2weight = {k: 1 / max(v, 1) for k, v in class2count.items()}
    return [float(sum(class2weight[int(k)] * int(v) for k, v in zip(c, n))) for c, n in per_item]


# ---- one recording ---------------------------------------------------------------------------------------------------------------------
def _validate_labels(N: int, o2r: np.ndarray, rows: np.ndarray, row_offset: np.ndarray) -> None:
    if o2r.dtype != np.int64 or o2r.ndim != 1:
        raise ValueError(f'objframe_idx_2_repr_idx must be an int64 vector, got {o2r.dtype} {o2r.shape}')
    if len(o2r) and (int(o2r.min()) < 0 or int(o2r.max()) >= N):
        raise ValueError(f'objframe_idx_2_repr_idx names a window outside [0, {N})')
    if np.any(np.diff(o2r) <= 0):
        raise ValueError('objframe_idx_2_repr_idx is not increasing')
    if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[1] != 7:
        raise ValueError(f'label rows must be float32 [n][7], got {rows.dtype} {rows.shape}')
    if (row_offset.dtype != np.int64 or row_offset.shape != (len(o2r) + 1,) or row_offset[0] != 0 or np.any(np.diff(row_offset) < 0)
            or int(row_offset[-1]) != rows.shape[0]):
        raise ValueError(f'row_offset must be a monotone int64 [{len(o2r) + 1}] from 0 to the {rows.shape[0]} rows')


class SequenceStore:
    """One recording's built windows: `frames` (host PackedFrames or PackedFrames2 of N windows), `objframe_idx_2_repr_idx` (int64, increasing: the
    window each labelled frame ends) and the labelled frames' fp32 [n][7] rows (t x y w h class_id class_confidence)."""

    def __init__(self, frames: PackedFrames, objframe_idx_2_repr_idx: np.ndarray, rows_per_frame: Sequence[np.ndarray]):
        if frames.device.type != 'cpu':
            raise ValueError('a SequenceStore keeps its frames on the host: call .to("cpu") first')
        o2r = np.ascontiguousarray(objframe_idx_2_repr_idx)
        rows_per_frame = [np.ascontiguousarray(r) for r in rows_per_frame]
        for r in rows_per_frame:
            if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != 7:
                raise ValueError(f'label rows must be float32 [n][7], got {r.dtype} {r.shape}')
        if len(rows_per_frame) != len(o2r):
            raise ValueError(f'{len(rows_per_frame)} label frames for {len(o2r)} entries of objframe_idx_2_repr_idx')
        rows = np.concatenate(rows_per_frame) if rows_per_frame else np.zeros((0, 7), dtype=np.float32)
        row_offset = np.zeros(len(o2r) + 1, dtype=np.int64)
        np.cumsum([r.shape[0] for r in rows_per_frame], out=row_offset[1:])
        _validate_labels(frames.num_frames, o2r, rows, row_offset)
        self.frames, self.objframe_idx_2_repr_idx, self.rows, self.row_offset = frames, o2r, rows, row_offset
        self._repr_2_objframe = {int(r): i for i, r in enumerate(o2r)}

    @property
    def num_windows(self) -> int:
        return self.frames.num_frames

    def __len__(self) -> int:
        return len(self.objframe_idx_2_repr_idx)

    def frame_rows(self, objframe_idx: int) -> np.ndarray:
        return self.rows[self.row_offset[objframe_idx]:self.row_offset[objframe_idx + 1]]

    def labels_at(self, repr_idx: int) -> Optional[np.ndarray]:
        """The rows of the labelled frame window `repr_idx` ends, None when it ends none (or an empty one, as the reference's
        SparselyBatchedObjectLabels turns an empty frame into None)."""
        f = self._repr_2_objframe.get(int(repr_idx))
        if f is None:
            return None
        r = self.frame_rows(f)
        return r if r.shape[0] > 0 else None

    @staticmethod
    def from_label_frames(frames: PackedFrames, label_frames, downsample_by_2: bool = False) -> 'SequenceStore':
        """From a recordings.LabelFrames: its frameidx_2_repridx and its per-frame rows."""
        o2r = np.asarray(label_frames.frameidx_2_repridx, dtype=np.int64)
        rows = [np.asarray(label_frames.rows(f, downsample_by_2), dtype=np.float32).reshape(-1, 7) for f in range(len(o2r))]
        return SequenceStore(frames, o2r, rows)

    def save(self, directory) -> None:
        os.makedirs(directory, exist_ok=True)
        self.frames.save(os.path.join(directory, 'frames.npz'))
        with open(os.path.join(directory, 'labels.npz'), 'wb') as f:
            np.savez(f, objframe_idx_2_repr_idx=self.objframe_idx_2_repr_idx, rows=self.rows, row_offset=self.row_offset)

    @staticmethod
    def load(directory) -> 'SequenceStore':
        """Read what `save` wrote and validate it before anything reaches a kernel."""
        frames = fc.load(os.path.join(directory, 'frames.npz'))
        with np.load(os.path.join(directory, 'labels.npz'), allow_pickle=False) as z:
            missing = [k for k in ('objframe_idx_2_repr_idx', 'rows', 'row_offset') if k not in z.files]
            if missing:
                raise ValueError(f'{directory}: not a sequence store, {missing} missing')
            o2r, rows, row_offset = z['objframe_idx_2_repr_idx'], z['rows'], z['row_offset']
        _validate_labels(frames.num_frames, o2r, rows, row_offset)
        return SequenceStore(frames, o2r, [rows[row_offset[i]:row_offset[i + 1]] for i in range(len(o2r))])


# ---- samples and label containers ------------------------------------------------------------------------------------------------------
@dataclass
class Sample:
    """One slot of a batch on the host: store (None = the fully padded filler), T window numbers (-1 = padding), the label rows of
    each window (None where it ends no labelled frame), and the two flags of the reference's item."""
    store: Optional[int]
    windows: np.ndarray
    labels: List[Optional[np.ndarray]]
    is_first_sample: bool
    new_sequence: bool = False                         # streaming: this chunk opens a sub-sequence (the augmentation is re-drawn)

    @property
    def is_padded_mask(self) -> np.ndarray:
        return self.windows < 0


def random_access_sample(store: SequenceStore, store_id: int, T: int, i: int, only_load_end_labels: bool = False) -> Sample:
    start, end = random_access_item(store.objframe_idx_2_repr_idx, T, i)
    labels = [None if (only_load_end_labels and r < end - 1) else store.labels_at(r) for r in range(start, end)]
    return Sample(store_id, np.arange(start, end, dtype=np.int64), labels, True)


def streaming_sample(store: SequenceStore, store_id: int, T: int, chunk: Tuple[int, int], chunk_idx: int) -> Sample:
    s, e = chunk
    assert T >= e - s > 0
    windows = np.full(T, -1, dtype=np.int64)
    windows[:e - s] = np.arange(s, e)
    labels = [store.labels_at(r) for r in range(s, e)] + [None] * (T - (e - s))
    return Sample(store_id, windows, labels, chunk_idx == 0, chunk_idx == 0)


def padded_sample(T: int) -> Sample:
    """get_fully_padded_sample: the filler of an exhausted evaluation slot."""
    return Sample(None, np.full(T, -1, dtype=np.int64), [None] * T, False)


class SparseLabels:
    """The labels of one time step of a batch: len() == B, entry b an fp32 [n][7] tensor or None (the surface of the reference's
    SparselyBatchedObjectLabels that the step uses)."""

    def __init__(self, labels: Sequence[Optional[torch.Tensor]]):
        self.labels = list(labels)

    def __len__(self) -> int:
        return len(self.labels)

    def __getitem__(self, b: int) -> Optional[torch.Tensor]:
        return self.labels[b]

    def __add__(self, other: 'SparseLabels') -> 'SparseLabels':
        return SparseLabels(self.labels + other.labels)

    def get_valid_labels_and_batch_indices(self) -> Tuple[List[torch.Tensor], List[int]]:
        idx = [b for b, lab in enumerate(self.labels) if lab is not None]
        return [self.labels[b] for b in idx], idx


# ---- the loader ----------------------------------------------------------------------------------------------------------------------------
class _Buffers:
    """One of the two sets of output buffers; the previous batch stays valid while the step uses it."""

    def __init__(self, T, B, G, frame_shape, dtype, dev):
        self.ev = torch.empty((T, B) + tuple(frame_shape), dtype=dtype, device=dev)
        self.rows_out = torch.empty(T, B, G, 7, dtype=torch.float32, device=dev)
        self.count_out = torch.empty(T, B, dtype=torch.int32, device=dev)
        self.yolox = torch.empty(T, B, G, 5, dtype=torch.float32, device=dev)


class _Staging:
    """Host residency: a packed set of T * B frames on the device, sized for the densest frames of the stores, and what fills it:
    staging='copy' a pinned twin of the set, staging='gather' a pinned int64 [T * B][4] table and its device twin."""

    def __init__(self, n_frames, frame_shape, dtype, cap, dev, pin, gather=False, version=1, mask_cap=0):
        def make(device, **kw):                                  # (format version 2: room for mask_cap mask words as well)
            if version == 2:
                return PackedFrames2.empty(frame_shape, dtype, n_frames, max(cap, 1), max(mask_cap, 1), device, zero=True, **kw)
            return PackedFrames.empty(frame_shape, dtype, n_frames, max(cap, 1), device, zero=True, **kw)
        self.dev = make(dev)
        self.host = self.table_host = self.table_dev = None
        if gather:
            cols = fc.GATHER2_COLS if version == 2 else fc.GATHER_COLS
            self.table_host = torch.zeros(n_frames * cols, dtype=torch.int64)
            if pin:
                self.table_host = self.table_host.pin_memory()
            self.table_rows = self.table_host.numpy().reshape(n_frames, cols)                  # the same memory, for numpy to fill
            self.table_dev = torch.zeros(n_frames * cols, dtype=torch.int64, device=dev)
        else:
            self.host = make('cpu', pin=pin)
        self.ready = torch.cuda.Event() if dev.type == 'cuda' else None


class BatchLoader:
    """Iterable; one iteration is an epoch.  The batch is described in the module docstring, the index rules are the functions above.
    resident: 'device' keeps the concatenated packed stores in device memory, 'host' keeps them pinned on the host and stages the
    frames of the next batch on a side stream: staging='copy' collects them on the host into a pinned set and copies that,
    staging='gather' writes one table row per frame and lets the device fetch them from the pinned stores (framecache.FrameGather);
    None = 'gather', the measured faster one; the batches are the same bit for bit.
    fused: None / False = unpack_frames + augment_planes (the measured faster route),
    True = unpack_augment (one launch, no dense intermediate).  seed: the epoch's random order comes from seed + epoch (the same on
    every rank); the streams' permutations and the augmentation draws use torch's global generator, seeded likewise when given.
    The stores' frames are PackedFrames or PackedFrames2 (format version 2), all of one version; version-2 stores take every route
    but fused=True, and give the batches of the converted version-1 stores bit for bit."""

    def __init__(self, stores: Sequence[SequenceStore], batch_size: int, sequence_length: int, mode: DatasetSamplingMode,
                 dataset_mode: Mode, augm_config: Any = None, dataset_hw: Optional[Tuple[int, int]] = None, device=None,
                 resident: str = 'device', weighted_sampling: bool = False, only_load_end_labels: bool = False, w_random: float = 1,
                 w_stream: float = 1, rank: int = 0, world_size: int = 1, seed: Optional[int] = None, fused: Optional[bool] = None,
                 staging: Optional[str] = None):
        self.stores = list(stores)
        if not self.stores:
            raise ValueError('no sequence stores')
        self.B, self.T = int(batch_size), int(sequence_length)
        assert self.B >= 1 and self.T >= 1
        self.mode, self.dataset_mode = DatasetSamplingMode(mode), dataset_mode
        self.train = dataset_mode == Mode.TRAIN
        if self.mode == DatasetSamplingMode.MIXED and not self.train:
            raise ValueError('MIXED sampling is a training mode')
        if resident not in ('device', 'host'):
            raise ValueError(f"resident must be 'device' or 'host', got {resident!r}")
        if staging not in (None, 'copy', 'gather'):
            raise ValueError(f"staging must be None, 'copy' or 'gather', got {staging!r}")
        if staging is not None and resident != 'host':
            raise ValueError(f"staging={staging!r} names how host-resident stores reach the device: it needs resident='host'")
        # the default is the measured one (profiles/frames_gather_bench.txt): at both shapes and all three fills the gather's host
        # time is lower (1 Mpx, 5 %: 1.7 ms against 55 ms) and its time until the set is ready is not higher (6.7 ms against 55 ms)
        self.staging = (staging or 'gather') if resident == 'host' else None
        assert world_size > rank >= 0
        self.rank, self.world_size, self.seed, self.epoch = rank, world_size, seed, 0
        self.weighted_sampling, self.only_load_end_labels = weighted_sampling, only_load_end_labels
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.resident = resident
        # the default route is the measured faster one: unpack_frames + augment_planes (profiles/loader_bench.txt: at 1 Mpx, 5 %
        # the one-launch kernel takes 1.96 ms against 1.49 ms); fused=True trades that for one (T, B, C, H, W) buffer less
        self.fused = False if fused is None else bool(fused)
        f0 = self.stores[0].frames
        self.version = 2 if isinstance(f0, PackedFrames2) else 1          # format version of the packed stores: all of one
        for s in self.stores:
            if s.frames.frame_shape != f0.frame_shape or s.frames.dtype != f0.dtype:
                raise ValueError(f'stores hold {s.frames.dtype} frames {s.frames.frame_shape} and {f0.dtype} frames {f0.frame_shape}')
            if isinstance(s.frames, PackedFrames2) != (self.version == 2):
                raise ValueError('stores hold packed frames of format versions 1 and 2: framecache.convert() them to one version')
        if self.fused and self.version == 2:
            raise ValueError('fused=True (unpack_augment) reads format version 1 only: version-2 stores take the two-launch route '
                             '(fused=None / False), or framecache.convert(frames, 1) them')
        if len(f0.frame_shape) != 3:
            raise ValueError(f'frames must be (C, H, W) planes, got {f0.frame_shape}')
        self.frame_shape, self.dtype = tuple(f0.frame_shape), f0.dtype
        self.hw = tuple(dataset_hw) if dataset_hw is not None else self.frame_shape[1:]
        if tuple(self.hw) != self.frame_shape[1:]:
            raise ValueError(f'frames are {self.frame_shape[1:]}, dataset_hw is {tuple(self.hw)}')
        self.base = np.concatenate(([0], np.cumsum([s.num_windows for s in self.stores]))).astype(np.int64)
        self.G = max([1] + [int(np.diff(s.row_offset).max()) for s in self.stores if len(s)])

        if self.mode == DatasetSamplingMode.MIXED:
            self.b_rnd, self.b_str = mixed_batch_split(self.B, w_random, w_stream)
        elif self.mode == DatasetSamplingMode.RANDOM:
            self.b_rnd, self.b_str = self.B, 0
        else:
            self.b_rnd, self.b_str = 0, self.B
        self.augm_rnd = self.augm_str = None
        if self.train and augm_config is not None:
            if self.b_rnd:
                self.augm_rnd = A.RandomSpatialAugmentorGenX(tuple(self.hw), True, A._cfg(augm_config, 'random'))
            if self.b_str:
                self.augm_str = [A.RandomSpatialAugmentorGenX(tuple(self.hw), False, A._cfg(augm_config, 'stream')) for _ in range(self.b_str)]

        # random access: the items of all stores, concatenated
        self.items = [(k, i) for k, s in enumerate(self.stores) for i in range(random_access_len(s.objframe_idx_2_repr_idx, self.T))]
        self.weights = None
        if self.b_rnd and self.train and weighted_sampling:
            ids = []
            for k, i in self.items:
                smp = random_access_sample(self.stores[k], k, self.T, i, only_load_end_labels)
                ids.append(np.concatenate([lab[:, 5] for lab in smp.labels if lab is not None]))
            self.weights = torch.tensor(sampler_weights(ids), dtype=torch.double)
        # streaming: (store, start, stop) per stream
        if self.train:
            self.streams = [(k, a, b) for k, s in enumerate(self.stores) if len(s)
                            for a, b in label_cluster_ranges(s.objframe_idx_2_repr_idx, self.T)]
        else:
            self.streams = [(k,) + streaming_range(s.objframe_idx_2_repr_idx, s.num_windows, self.T) for k, s in enumerate(self.stores) if len(s)]
        self.stream_chunks = [streaming_chunks(a, b, self.T) for _, a, b in self.streams]

        dev = self.device
        self.parts = {}
        for name, b in ((DatasetSamplingMode.RANDOM, self.b_rnd), (DatasetSamplingMode.STREAM, self.b_str)):
            if b:
                self.parts[name] = dict(B=b, bufs=[_Buffers(self.T, b, self.G, self.frame_shape, self.dtype, dev) for _ in range(2)], flip=0,
                                        index=torch.empty(self.T, b, dtype=torch.int64, device=dev),
                                        rows=torch.empty(self.T, b, self.G, 7, dtype=torch.float32, device=dev),
                                        count=torch.empty(self.T, b, dtype=torch.int32, device=dev),
                                        it=torch.zeros(b, A.PLANES_TABLE_COLS, dtype=torch.int32, device=dev),
                                        ft=torch.zeros(b, A.LABEL_TABLE_COLS, dtype=torch.float32, device=dev),
                                        dense=None if self.fused else torch.empty((self.T, b) + self.frame_shape, dtype=self.dtype, device=dev))
        if resident == 'device':
            self.packed = fc.concat([s.frames for s in self.stores]).to(dev)
        else:
            pin = dev.type == 'cuda'
            if pin:
                for s in self.stores:
                    s.frames = s.frames.pin_memory()
            cap = max(int(np.diff(s.frames.value_base.numpy()).max()) for s in self.stores)
            # (format version 2: the staging sets also hold the masks of the frames' non-empty groups, sized likewise)
            mcap = max(int(np.diff(s.frames.mask_base.numpy()).max()) for s in self.stores) if self.version == 2 else 0
            self.side = torch.cuda.Stream(device=dev) if pin else None
            gather = self.staging == 'gather'
            self.gatherer = fc.FrameGather([s.frames for s in self.stores], dev) if gather else None
            self.gather_blocks = 0                               # 0 = the library's default grid cap
            for p in self.parts.values():
                n = self.T * p['B']
                p['staging'] = [_Staging(n, self.frame_shape, self.dtype, n * cap, dev, pin, gather, self.version, n * mcap) for _ in range(2)]

    # ---- orders ----
    def _generator(self) -> Optional[torch.Generator]:
        if self.seed is None:
            return None
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        return g

    def random_order(self) -> List[int]:
        """This rank's item positions for the epoch: one order on every rank (seed + epoch), positions rank::world_size of it."""
        n = len(self.items)
        if not self.train:
            order = list(range(n))
        elif self.weights is not None:
            order = torch.multinomial(self.weights, n, replacement=True, generator=self._generator()).tolist()
        else:
            order = torch.randperm(n, generator=self._generator()).tolist()
        return order[self.rank::self.world_size]

    def _random_batches(self, B: int) -> Iterator[List[Sample]]:
        order = self.random_order()
        for at in range(0, len(order) - B + 1, B):                # drop_last
            yield [random_access_sample(self.stores[k], k, self.T, i, self.only_load_end_labels)
                   for k, i in (self.items[j] for j in order[at:at + B])]

    def _slot_stream(self, positions: Sequence[int]) -> Iterator[Sample]:
        for p in positions:
            k = self.streams[p][0]
            for ci, chunk in enumerate(self.stream_chunks[p]):
                yield streaming_sample(self.stores[k], k, self.T, chunk, ci)

    def stream_slot_orders(self, B: int) -> List[List[int]]:
        """Stream positions each batch slot walks this epoch."""
        if self.train:                                           # every slot its own permutation, drawn first, in slot order
            return [torch.randperm(len(self.streams)).tolist() for _ in range(B)]
        lengths = [len(c) for c in self.stream_chunks]
        mine = assign_to_worker(lengths, self.world_size, self.rank)
        return [[mine[i] for i in slot] for slot in assign_to_slots([lengths[p] for p in mine], B)]

    def _stream_batches(self, B: int) -> Iterator[List[Sample]]:
        slots = [self._slot_stream(o) for o in self.stream_slot_orders(B)]
        while True:
            batch, live = [], 0
            for s in slots:
                smp = next(s, None)
                if smp is None:
                    if self.train:                               # Zipper: the epoch ends with the first exhausted slot
                        return
                    smp = padded_sample(self.T)                  # ZipperLongest with the fully padded sample
                else:
                    live += 1
                batch.append(smp)
            if not live:
                return
            yield batch

    # ---- a batch ----
    def _states(self, part: DatasetSamplingMode, samples: List[Sample]) -> List[A.SpatialAugmentState]:
        if part == DatasetSamplingMode.RANDOM and self.augm_rnd is not None:
            return A.sample_states(self.augm_rnd, [s.labels for s in samples])
        if part == DatasetSamplingMode.STREAM and self.augm_str is not None:
            out = []
            for aug, s in zip(self.augm_str, samples):           # slot order: the reference's single-worker order of RNG calls
                if s.new_sequence:
                    aug.randomize_augmentation()
                out.append(aug.draw(s.labels))
            return out
        return [A.SpatialAugmentState() for _ in samples]

    def _global_index(self, samples: List[Sample]) -> np.ndarray:
        idx = np.full((self.T, len(samples)), -1, dtype=np.int64)
        for b, s in enumerate(samples):
            if s.store is not None:
                idx[:, b] = np.where(s.windows >= 0, s.windows + self.base[s.store], -1)
        return idx

    def _staging_set(self, p: dict, idx: np.ndarray):
        """(the staging set this batch fills, the global numbers of the frames it names, the index into them)."""
        need = np.unique(idx[idx >= 0])
        local = np.full_like(idx, -1)
        local[idx >= 0] = np.searchsorted(need, idx[idx >= 0])
        return p['staging'][p['flip']], need, local

    def _on_side_stream(self, st: '_Staging', fill) -> None:
        """fill(non_blocking) on the side stream, behind the set's previous reader on the current stream, and st.ready behind it;
        without a side stream (the CPU emulator) fill runs at once."""
        if self.side is None:
            fill(False)
            return
        self.side.wait_stream(torch.cuda.current_stream(self.device))            # the set's previous reader is done
        with torch.cuda.stream(self.side):
            fill(True)
            st.ready.record(self.side)

    def _stage(self, p: dict, idx: np.ndarray):
        """Host residency: gather the frames the batch names into the pinned staging set and start its copy on the side stream.
        Returns (staging set, local index)."""
        st, need, local = self._staging_set(p, idx)
        runs, at = [], 0
        while at < len(need):                                    # runs of consecutive frames of one store: one slice each
            k = int(np.searchsorted(self.base, need[at], side='right')) - 1
            end = at + 1
            while end < len(need) and need[end] == need[end - 1] + 1 and need[end] < self.base[k + 1]:
                end += 1
            runs.append(self.stores[k].frames.slice(int(need[at] - self.base[k]), int(need[end - 1] - self.base[k]) + 1))
            at = end
        h = st.host
        # the arrays with a row per frame, those with an entry per frame and one more, and the variable-length runs
        per_frame, bases, run_arrays = ((('group_mask', 'seg_offset', 'grp_offset'), ('value_base', 'mask_base'), ('masks', 'values'))
                                        if self.version == 2 else (('masks', 'seg_offset'), ('value_base',), ('values',)))
        if runs:
            g = fc.concat(runs)
            n = g.num_frames
            for k in per_frame:
                getattr(h, k)[:n].copy_(getattr(g, k))
            for k in bases:
                getattr(h, k)[:n + 1].copy_(getattr(g, k))
            for k in run_arrays:
                getattr(h, k)[:getattr(g, k).numel()].copy_(getattr(g, k))

        def fill(non_blocking):
            for k in per_frame + bases + run_arrays:
                getattr(st.dev, k).copy_(getattr(h, k), non_blocking=non_blocking)
        self._on_side_stream(st, fill)
        return st, local

    def _stage_gather(self, p: dict, idx: np.ndarray):
        """Host residency, staging='gather': one table row per frame the batch names, and one gather launch on the side stream that
        fetches them from the pinned stores into the device set.  Returns (staging set, local index)."""
        st, need, local = self._staging_set(p, idx)
        n = len(need)
        if st.ready is not None:
            st.ready.synchronize()                               # the table's previous copy has left the pinned buffer (long done: no wait)
        if n:
            self.gatherer.table(need, out=st.table_rows)

        def fill(non_blocking):
            if n:
                cols = self.gatherer.cols
                st.table_dev[:n * cols].copy_(st.table_host[:n * cols], non_blocking=non_blocking)
                self.gatherer.launch(st.table_dev, n, st.dev, self.gather_blocks)
        self._on_side_stream(st, fill)
        return st, local

    def _plan(self, part: DatasetSamplingMode, samples: List[Sample]) -> dict:
        """Steps 1-3 on the host: indices and label rows, the draw, and (host residency) the staging copy."""
        p = self.parts[part]
        idx = self._global_index(samples)
        states = self._states(part, samples)
        rows, count = A.pack_labels([[s.labels[t] for s in samples] for t in range(self.T)], G=self.G)
        plan = dict(part=part, samples=samples, states=states, rows=rows, count=count, index=idx, packed=None)
        if self.resident == 'host':
            st, plan['index'] = (self._stage_gather if self.staging == 'gather' else self._stage)(p, idx)
            plan['packed'] = st
        return plan

    def _launch(self, plan: dict, as_lists: bool) -> dict:
        """Steps 3-5: tables, one unpack_augment launch, one label launch, one read-back."""
        p = self.parts[plan['part']]
        samples, states = plan['samples'], plan['states']
        buf = p['bufs'][p['flip']]
        p['flip'] ^= 1
        if plan['packed'] is None:
            packed = self.packed
        else:
            if plan['packed'].ready is not None:
                torch.cuda.current_stream(self.device).wait_event(plan['packed'].ready)
            packed = plan['packed'].dev
        p['index'].copy_(torch.from_numpy(plan['index']))
        p['rows'].copy_(plan['rows'])
        p['count'].copy_(plan['count'])
        A.write_tables(states, self.hw, p['it'], p['ft'])
        if self.fused:
            fc.unpack_augment(packed, p['index'], p['it'], out=buf.ev)
        else:
            fc.unpack_frames(packed, p['index'], out=p['dense'])
            A.augment_planes(p['dense'].view(torch.uint8), p['it'], out=buf.ev.view(torch.uint8))
        A.augment_labels(p['rows'], p['count'], p['ft'], out=(buf.rows_out, buf.count_out, buf.yolox))
        labelled_dev = A.labelled_frames(buf.count_out, states)
        count_h, rows_h = buf.count_out.cpu(), buf.rows_out.cpu()                  # the one read-back: everything before is asynchronous
        zoom_out = np.array([s.mode == A.MODE_ZOOM_OUT for s in states])
        cnt = count_h.numpy()
        labelled = (cnt > 0) | ((cnt == 0) & zoom_out[None, :])
        labels_seq = [SparseLabels([rows_h[t, b, :cnt[t, b]].clone() if labelled[t, b] else None for b in range(len(samples))])
                      for t in range(self.T)]
        padded = torch.from_numpy(np.stack([s.is_padded_mask for s in samples], axis=1)).to(self.device)
        data = {DataType.EV_REPR: [buf.ev[t] for t in range(self.T)] if as_lists else buf.ev,
                DataType.OBJLABELS_SEQ: labels_seq,
                DataType.IS_FIRST_SAMPLE: torch.tensor([s.is_first_sample for s in samples], dtype=torch.bool).to(self.device),
                DataType.IS_PADDED_MASK: [padded[t] for t in range(self.T)] if as_lists else padded}
        return {'data': data, 'worker_id': 0, 'device_labels': (buf.rows_out, buf.count_out, buf.yolox, labelled_dev),
                'states': states, 'samples': samples}

    def __iter__(self):
        self.epoch += 1
        if self.seed is not None and self.train and self.b_str:
            torch.manual_seed(self.seed + self.epoch)             # the streams' permutations and draws use the global generator
        if self.mode == DatasetSamplingMode.MIXED:
            plans = (({DatasetSamplingMode.RANDOM: self._plan(DatasetSamplingMode.RANDOM, r),
                       DatasetSamplingMode.STREAM: self._plan(DatasetSamplingMode.STREAM, s)})
                     for r, s in zip(self._random_batches(self.b_rnd), self._stream_batches(self.b_str)))
        elif self.mode == DatasetSamplingMode.RANDOM:
            plans = ({DatasetSamplingMode.RANDOM: self._plan(DatasetSamplingMode.RANDOM, r)} for r in self._random_batches(self.B))
        else:
            plans = ({DatasetSamplingMode.STREAM: self._plan(DatasetSamplingMode.STREAM, s)} for s in self._stream_batches(self.B))
        mixed = self.mode == DatasetSamplingMode.MIXED
        cur = next(plans, None)
        while cur is not None:
            out = {part: self._launch(plan, mixed) for part, plan in cur.items()}
            cur = next(plans, None)                               # host residency: batch k + 1 is staged (into the other set) while batch k is consumed
            yield out if mixed else next(iter(out.values()))
