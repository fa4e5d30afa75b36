"""Raw Prophesee recordings: a ``*_td.dat`` event file plus its ``*_bbox.npy`` labels -> what the rest of this package takes.

The reference gets here through offline preprocessing into H5 files (scripts/genx/preprocess_dataset.py); this module does the same
work on the recording itself.  Events are per-event work and go to the device; labels are a few thousand rows per recording and
stay in numpy.

Events (rvt_event_decode_dat, rvt_amd/csrc/evprep.hpp):
  * ``read_dat_header(path) -> DatHeader(offset, ev_type, ev_size, height, width)``: the ``% `` comment lines, then one byte of
    event type and one of event size (utils/evaluation/prophesee/io/dat_events_tools.py:120-175, parse_header).  A file without
    comment lines is the legacy layout: type 0, size 8, records from byte 0.  Only Event2D records of 8 bytes are accepted.
  * ``DatDecoder(B, capacity, device, coord=torch.int16, repair=True)`` owns B stream buffers of ``capacity`` events, their
    device table, the repair carry and the workspace.  ``decode(records, counts=None)`` unpacks B device tensors of packed
    ``{uint32 t; int32 w}`` records (uint8 bytes or int64 words) into the compact 14 B/event form and returns the ``EventTable``
    for ``EventSequenceBuilder.build_from_table``; with ``repair`` the timestamps come out non-decreasing (the reader's
    ``_correct_time``), and the carry makes consecutive ``decode`` calls repair like one long stream until ``reset()``.
    Everything is read on the device: capture ``decode`` + ``build_from_table`` in a graph, rewrite ``records`` and
    ``decoder.n_records`` in place, replay.  ``load_dat(path)`` is the one-file convenience.

Labels, in the reference's order of operations (preprocess_dataset.py:195-432, data/genx_utils/labels.py:149-198):
  * ``filter_labels``: class filter of the 1 Mpx set, crop to the field of view, Prophesee or conservative size filter, and on
    the training split the filter for boxes as wide as the frame.  Returns a new array.
  * ``frame_labels`` -> ``LabelFrames``: the labelled frames on the base label period with 2 ms of jitter allowed, the window-end
    timestamps (back-filled before the first frame, evenly cut between frames) and the frame -> window index.
  * ``LabelFrames.rows`` / ``window_rows``: per-frame fp32 ``[n][7]`` rows ``t x y w h class_id class_confidence``, clamped to the
    frame and optionally at half scale, as ``augment.pack_labels``, the head and the evaluator take them.

``Recording`` joins the two sides for one recording.  Out of scope: H5 files.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from .evaluation import BBOX_DTYPE
from .representations import _COORD_BYTES, EventSequenceBuilder, EventTable, prep_blocks, prep_ws_elems

DATASETS = ('gen1', 'gen4')                          # the reference's names: Gen1 (304 x 240) and 1 Mpx (1280 x 720)
SENSOR_HW = {'gen1': (240, 304), 'gen4': (720, 1280)}
SPLITS = ('train', 'val', 'test')
LABEL_FRAME_STEP_MS = 100                            # labelled frames are looked for on a 100 ms grid (preprocess_dataset.py:348)
JITTER_US = 2000
MIN_FRAME_GAP_US = 98000
ROW_FIELDS = ('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')


class NoLabels(Exception):
    """No label of the recording survives the filters."""


def _check_dataset(dataset: str) -> None:
    if dataset not in DATASETS:
        raise ValueError(f'dataset={dataset!r} is not one of {DATASETS}')


# --------------------------------------------------------------------------------------------------------------- DAT files
class DatHeader(NamedTuple):
    offset: int                      # first byte of the records
    ev_type: int
    ev_size: int
    height: Optional[int]
    width: Optional[int]


def read_dat_header(path: Union[str, os.PathLike]) -> DatHeader:
    height = width = None
    with open(path, 'rb') as f:
        comment_lines = 0
        while True:
            start = f.tell()
            line = f.readline()
            if line[:2] != b'% ':
                break
            comment_lines += 1
            words = line.split()
            if len(words) > 2 and words[1] == b'Height':
                height = int(words[2])
            if len(words) > 2 and words[1] == b'Width':
                width = int(words[2])
        f.seek(start)
        if comment_lines:
            tb = f.read(2)
            if len(tb) != 2:
                raise ValueError(f'{path}: the file ends inside its header')
            ev_type, ev_size = tb[0], tb[1]
        else:
            ev_type, ev_size = 0, 8              # legacy file: records from the first byte
        offset = f.tell()
    if ev_type != 0 or ev_size != 8:
        raise ValueError(f'{path}: event type {ev_type} with {ev_size}-byte records; only Event2D (type 0, 8 bytes) is read')
    return DatHeader(offset, int(ev_type), int(ev_size), height, width)


class DatDecoder:
    def __init__(self, B: int, capacity: int, device, coord: torch.dtype = torch.int16, repair: bool = True, blocks_per_stream: int = 0):
        if B < 1 or capacity < 0:
            raise ValueError(f'B={B} must be positive and capacity={capacity} non-negative')
        if coord not in _COORD_BYTES:
            raise TypeError(f'coord={coord} is not one of int16 / int32 / int64')
        dev = torch.device(device)
        self.B, self.capacity, self.device, self.coord, self.repair = int(B), int(capacity), dev, coord, bool(repair)
        self.blocks_per_stream = int(blocks_per_stream)
        self.streams = [tuple(torch.zeros(self.capacity, dtype=dt, device=dev) for dt in (coord, coord, coord, torch.int64)) for _ in range(B)]
        self.ts_end = torch.zeros(1, dtype=torch.int64, device=dev)          # placeholder rows: write_table brings the real window ends
        self.table = EventSequenceBuilder(1, 1, 1, window_us=1).make_table(self.streams, self.ts_end, counts=[0] * B)
        self.carry = torch.zeros(B, dtype=torch.int64, device=dev)
        # (without the repair the decode is one launch and takes no workspace)
        self.ws = torch.empty(prep_ws_elems(B, self.blocks_per_stream), dtype=torch.int64, device=dev) if self.repair else None
        self.repaired = torch.zeros(B, prep_blocks(B, self.blocks_per_stream), dtype=torch.int64, device=dev)
        self.n_records = torch.zeros(B, dtype=torch.int64, device=dev)
        self.record_ptrs = torch.zeros(B, dtype=torch.int64, device=dev)
        self._records: List[torch.Tensor] = []

    def reset(self) -> None:
        """Forget the streams so far: the next decode repairs from 0 again."""
        self.carry.zero_()

    def set_window_ends(self, ts_end_us: torch.Tensor) -> EventTable:
        """Point the table's rows at the window ends (int64 [T] or [B][T]) the builder is to slice by."""
        ts_end = EventSequenceBuilder._check_ts_end(ts_end_us, self.B)
        rows = self.table.dev.cpu().numpy().view(L.row_dtype('RvtEventStream')).reshape(self.B)
        for b in range(self.B):
            rows[b]['ts_end'] = (ts_end if ts_end.dim() == 1 else ts_end[b]).data_ptr()
        self.table.dev.copy_(torch.from_numpy(rows.view(np.int64).reshape(self.B, -1)))
        self.table.ts_end, self.table.T = ts_end, int(ts_end.shape[-1])
        return self.table

    def decode(self, records: Sequence[torch.Tensor], counts: Optional[Sequence[int]] = None) -> EventTable:
        """records: B contiguous device tensors of packed records, uint8 (8 bytes each) or int64 (one each), 8-byte aligned.
        counts[b]: records of stream b in use (default: all of the tensor).  At most ``capacity`` are decoded per stream."""
        records = list(records)
        if len(records) != self.B:
            raise ValueError(f'{len(records)} record tensors for B={self.B} streams')
        ptrs, ns = [], []
        for b, r in enumerate(records):
            if not torch.is_tensor(r) or r.dtype not in (torch.uint8, torch.int64) or r.dim() != 1 or r.device != self.device:
                raise TypeError(f'records[{b}] must be a 1-D uint8 or int64 tensor on {self.device}')
            have = r.numel() // 8 if r.dtype == torch.uint8 else r.numel()
            if r.dtype == torch.uint8 and r.numel() % 8:
                raise ValueError(f'records[{b}]: {r.numel()} bytes are not a whole number of 8-byte records')
            p = L.ptr(r)
            if p % 8:
                raise ValueError(f'records[{b}] starts at an address that is not 8-byte aligned')
            n = have if counts is None else int(counts[b])
            if not 0 <= n <= have:
                raise ValueError(f'counts[{b}]={n} outside 0..{have}')
            ptrs.append(p)
            ns.append(n)
        if [r.data_ptr() for r in self._records] != ptrs:          # same buffers again (a replay loop): nothing to upload
            self.record_ptrs.copy_(torch.tensor(ptrs, dtype=torch.int64))
        self.n_records.copy_(torch.tensor(ns, dtype=torch.int64))
        self._records = records
        return self.decode_in_place()

    def decode_in_place(self) -> EventTable:
        """Decode what ``record_ptrs`` / ``n_records`` say on the device, without any host-to-device traffic: the capturable form.
        Nothing is checked here: that every address in ``record_ptrs`` is 8-byte aligned and holds at least
        ``min(n_records[b], capacity)`` records is the caller's to keep (``decode`` checks both for the tensors it is given)."""
        L.call('rvt_event_decode_dat', L.ptr(self.record_ptrs), L.ptr(self.n_records), self.capacity, L.ptr(self.table.dev), self.B,
               _COORD_BYTES[self.coord], int(self.repair), L.ptr(self.carry), L.ptr(self.repaired), L.ptr(self.ws), self.blocks_per_stream,
               L.stream_of(self.table.dev))
        return self.table

    def counts(self) -> List[int]:
        """Events per stream after the last decode (read back from the table: synchronises)."""
        rows = self.table.dev.cpu().numpy().view(L.row_dtype('RvtEventStream')).reshape(self.B)
        return [int(n) for n in rows['n']]

    @staticmethod
    def load_dat(path: Union[str, os.PathLike], device, coord: torch.dtype = torch.int16, repair: bool = True):
        """One file -> (decoder, table): the records behind the header are uploaded into a fresh allocation and decoded."""
        hdr = read_dat_header(path)
        raw = np.fromfile(path, dtype=np.uint8, offset=hdr.offset)
        raw = raw[:raw.size - raw.size % hdr.ev_size]
        dec = DatDecoder(1, raw.size // hdr.ev_size, device, coord, repair)
        return dec, dec.decode([torch.from_numpy(raw).to(device)])


# ------------------------------------------------------------------------------------------------------------------ labels
def as_box_records(labels: np.ndarray) -> np.ndarray:
    """A copy of box records in BBOX_DTYPE, fields taken by name (a ``_bbox.npy`` loads with an equivalent dtype of its own)."""
    names = getattr(labels.dtype, 'names', None)
    if not names or any(k not in names for k in BBOX_DTYPE.names):
        raise TypeError(f'labels must be box records with the fields {BBOX_DTYPE.names}, got {labels.dtype}')
    out = np.zeros(labels.shape, dtype=BBOX_DTYPE)
    for k in BBOX_DTYPE.names:
        out[k] = labels[k]
    return out


def filter_labels(labels: np.ndarray, dataset: str, split: str, apply_psee_bbox_filter: bool, apply_faulty_bbox_filter: bool) -> np.ndarray:
    _check_dataset(dataset)
    if split not in SPLITS:
        raise ValueError(f'split={split!r} is not one of {SPLITS}')
    lab = as_box_records(labels)
    H, W = SENSOR_HW[dataset]
    if dataset == 'gen4':                                 # pedestrian, two-wheeler, car stay; truck, bus, signs, lights go
        lab = lab[lab['class_id'] <= 2]
    # boxes hang out of the frame in both datasets: cut them to it and drop what is left without area
    left, top = lab['x'], lab['y']
    right, bottom = left + lab['w'], top + lab['h']
    left, right = np.clip(left, a_min=0, a_max=W - 1), np.clip(right, a_min=0, a_max=W - 1)
    top, bottom = np.clip(top, a_min=0, a_max=H - 1), np.clip(bottom, a_min=0, a_max=H - 1)
    bw, bh = right - left, bottom - top
    if np.any(bw < 0) or np.any(bh < 0):
        raise ValueError('a label has a negative width or height')
    lab['x'], lab['y'], lab['w'], lab['h'] = left, top, bw, bh
    lab = lab[(lab['w'] > 0) & (lab['h'] > 0)]
    if apply_psee_bbox_filter:
        diag, side = (60, 20) if dataset == 'gen4' else (30, 10)
        lab = lab[(lab['w'] ** 2 + lab['h'] ** 2 >= diag ** 2) & (lab['w'] >= side) & (lab['h'] >= side)]
    else:
        lab = lab[(lab['w'] >= 5) & (lab['h'] >= 5)]
    if split == 'train' and apply_faulty_bbox_filter:     # labels that span the frame without covering an object
        lab = lab[lab['w'] <= (9 * W) // 10]
    return lab


def _base_label_period_us(unique_ts_us: np.ndarray, dataset: str) -> int:
    if dataset == 'gen1':
        return 250000                                     # Gen1 is labelled at 4 Hz
    median = np.median(np.diff(unique_ts_us))
    hz = int(np.rint(10 ** 6 / median))
    if hz not in (30, 60):
        raise ValueError(f'1 Mpx labels come at 30 or 60 Hz, these at {hz} Hz')
    return int(6 * median if hz == 60 else 3 * median)    # about 10 Hz


class LabelFrames:
    """The labelled frames of one recording.  labels: the filtered box records of all frames, frame after frame;
    objframe_idx_2_label_idx[f]: first record of frame f; frame_ts_us[f]; ev_repr_ts_end_us: the window ends of the whole
    recording; frameidx_2_repridx[f]: the window that ends on frame f."""

    def __init__(self, labels: np.ndarray, objframe_idx_2_label_idx: np.ndarray, frame_ts_us: np.ndarray, ev_repr_ts_end_us: np.ndarray,
                 frameidx_2_repridx: np.ndarray, dataset: str):
        _check_dataset(dataset)
        self.labels, self.objframe_idx_2_label_idx, self.frame_ts_us = labels, objframe_idx_2_label_idx, frame_ts_us
        self.ev_repr_ts_end_us, self.frameidx_2_repridx, self.dataset = ev_repr_ts_end_us, frameidx_2_repridx, dataset
        self._clamped: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return len(self.frame_ts_us)

    def _all_rows(self) -> np.ndarray:
        """Every record as an fp32 row, clamped to the frame (done once for the recording, as the reference's label factory does)."""
        if self._clamped is None:
            H, W = SENSOR_HW[self.dataset]
            rows = np.stack([self.labels[k].astype(np.float32) for k in ROW_FIELDS], axis=1)
            x0, y0 = np.clip(rows[:, 1], 0, W - 1), np.clip(rows[:, 2], 0, H - 1)
            x1, y1 = np.clip(rows[:, 1] + rows[:, 3], 0, W - 1), np.clip(rows[:, 2] + rows[:, 4], 0, H - 1)
            w, h = x1 - x0, y1 - y0
            if not (np.all(w > 0) and np.all(h > 0)):
                raise ValueError('a label has no area inside the frame: filter the labels first')
            rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = x0, y0, w, h
            self._clamped = rows
        return self._clamped

    def rows(self, frame_idx: int, downsample_by_2: bool = False) -> np.ndarray:
        if not 0 <= frame_idx < len(self):
            raise IndexError(f'frame {frame_idx} outside 0..{len(self) - 1}')
        allr = self._all_rows()
        i0 = int(self.objframe_idx_2_label_idx[frame_idx])
        i1 = allr.shape[0] if frame_idx == len(self) - 1 else int(self.objframe_idx_2_label_idx[frame_idx + 1])
        if i1 <= i0:
            raise ValueError(f'frame {frame_idx} has no labels')
        r = allr[i0:i1].copy()
        if downsample_by_2:
            H, W = SENSOR_HW[self.dataset]
            half = np.float32(0.5)
            x1 = np.minimum((r[:, 1] + r[:, 3]) * half, np.float32(0.5 * W - 1))
            y1 = np.minimum((r[:, 2] + r[:, 4]) * half, np.float32(0.5 * H - 1))
            r[:, 1], r[:, 2] = r[:, 1] * half, r[:, 2] * half
            r[:, 3], r[:, 4] = x1 - r[:, 1], y1 - r[:, 2]
            r = r[(r[:, 3] > 0) & (r[:, 4] > 0)]
        return r

    def window_rows(self, first_repr_idx: int, T: int, downsample_by_2: bool = False) -> List[Optional[np.ndarray]]:
        """For the T windows from first_repr_idx on: the rows of the frame a window ends on, None where it ends on none
        (or where the half-scale step leaves no box)."""
        out: List[Optional[np.ndarray]] = [None] * T
        for f, ridx in enumerate(self.frameidx_2_repridx):
            k = int(ridx) - first_repr_idx
            if 0 <= k < T:
                r = self.rows(f, downsample_by_2)
                out[k] = r if r.shape[0] else None
        return out


def frame_labels(labels: np.ndarray, dataset: str, align_t_ms: int = 100, ts_step_ev_repr_ms: int = 50) -> LabelFrames:
    """labels: FILTERED box records, sorted by time.  align_t_ms: labels before it are skipped (the first one at or after it is the
    reference frame); ts_step_ev_repr_ms: the window period, a divisor of 100 ms."""
    _check_dataset(dataset)
    if ts_step_ev_repr_ms <= 0 or LABEL_FRAME_STEP_MS % ts_step_ev_repr_ms:
        raise ValueError(f'ts_step_ev_repr_ms={ts_step_ev_repr_ms} must be a positive divisor of {LABEL_FRAME_STEP_MS}')
    if labels.size == 0:
        raise NoLabels
    delta_us = ts_step_ev_repr_ms * 1000
    per_step = LABEL_FRAME_STEP_MS // ts_step_ev_repr_ms
    label_t = np.asarray(labels['t'], dtype=np.int64)
    unique_ts = np.unique(label_t)
    period = _base_label_period_us(unique_ts, dataset)
    first = int(np.searchsorted(unique_ts, align_t_ms * 1000, side='left'))
    if first >= unique_ts.size:
        raise ValueError(f'align_t_ms={align_t_ms} lies behind the last label')

    # a label time becomes a frame when it lies a whole number of base periods behind the last frame, 2 ms of jitter allowed
    frames, windows_between = [int(unique_ts[first])], []
    for ts in unique_ts[first + 1:]:
        diff = int(ts) - frames[-1]
        count = round(diff / period)
        if abs(diff - count * period) <= JITTER_US:
            if count <= 0:
                raise ValueError(f'label time {int(ts)} is less than a label period behind the frame at {frames[-1]}')
            frames.append(int(ts))
            windows_between.append(count * per_step)
    frame_ts = np.asarray(frames, dtype=np.int64)
    if frame_ts.size > 1 and int(np.diff(frame_ts).min()) <= MIN_FRAME_GAP_US:
        raise ValueError(f'frames {int(np.diff(frame_ts).min())} us apart: at least {MIN_FRAME_GAP_US} expected')

    i0 = np.searchsorted(label_t, frame_ts, side='left')
    i1 = np.searchsorted(label_t, frame_ts, side='right')
    per_frame = [labels[a:b] for a, b in zip(i0, i1)]
    for lab, ts in zip(per_frame, frame_ts):
        if lab.size == 0 or np.any(lab['t'] != ts):
            raise ValueError('the labels are not sorted by time')
    offsets = np.cumsum([0] + [len(lab) for lab in per_frame[:-1]]).astype(np.int64)

    # window ends: every delta_us down from the first frame while positive, without the earliest of them and without the frame
    # itself; then between two frames the edges of an even cut, each frame opening its interval and the last one closing the list
    ends = np.arange(frames[0] - delta_us, 0, -delta_us, dtype=np.int64)[::-1][1:].tolist()
    for k, (n_win, a, b) in enumerate(zip(windows_between, frame_ts[:-1], frame_ts[1:])):
        edges = np.linspace(a, b, n_win + 1).astype(np.int64).tolist()
        ends.extend(edges if k == len(windows_between) - 1 else edges[:-1])
    if frame_ts.size == 1:
        ends.append(frames[0])
    ends = np.asarray(ends, dtype=np.int64)
    f2r = np.searchsorted(ends, frame_ts, side='left')
    if np.any(f2r >= ends.size) or np.any(ends[f2r] != frame_ts):
        raise ValueError('a frame does not fall on a window end')
    return LabelFrames(as_box_records(np.concatenate(per_frame)), offsets, frame_ts, ends, f2r.astype(np.int64), dataset)


# --------------------------------------------------------------------------------------------------------------- recording
class Recording:
    """One recording: ``<name>_td.dat`` + ``<name>_bbox.npy``.  The labels are read and framed at construction (NoLabels when none
    survives); the events are read, uploaded and decoded on first use of ``table()``."""

    def __init__(self, dat_path: Union[str, os.PathLike], bbox_path: Union[str, os.PathLike], dataset: str, split: str,
                 apply_psee_bbox_filter: Optional[bool] = None, apply_faulty_bbox_filter: bool = True, align_t_ms: int = 100,
                 ts_step_ev_repr_ms: int = 50, device=None, coord: torch.dtype = torch.int16, repair: bool = True):
        _check_dataset(dataset)
        self.dat_path, self.bbox_path, self.dataset, self.split = dat_path, bbox_path, dataset, split
        self.device, self.coord, self.repair = device, coord, repair
        self.header = read_dat_header(dat_path)
        self.height, self.width = SENSOR_HW[dataset]
        if apply_psee_bbox_filter is None:                # the reference's shipped filter settings: Prophesee's sizes on Gen1 only
            apply_psee_bbox_filter = dataset == 'gen1'
        raw = np.load(bbox_path)
        if len(raw) == 0:
            raise NoLabels
        self.frames = frame_labels(filter_labels(raw, dataset, split, apply_psee_bbox_filter, apply_faulty_bbox_filter), dataset,
                                   align_t_ms, ts_step_ev_repr_ms)
        self._decoder: Optional[DatDecoder] = None

    def window_ends(self, first_repr_idx: int, T: int) -> torch.Tensor:
        """int64 [T] window-end timestamps from window first_repr_idx on, as EventSequenceBuilder takes them (a CPU tensor when
        the recording has no device yet)."""
        ends = self.frames.ev_repr_ts_end_us
        if first_repr_idx < 0 or T < 1 or first_repr_idx + T > ends.size:
            raise IndexError(f'windows {first_repr_idx}..{first_repr_idx + T - 1} outside 0..{ends.size - 1}')
        t = torch.from_numpy(ends[first_repr_idx:first_repr_idx + T].copy())
        return t if self.device is None else t.to(self.device)

    def window_rows(self, first_repr_idx: int, T: int, downsample_by_2: bool = False) -> List[Optional[np.ndarray]]:
        return self.frames.window_rows(first_repr_idx, T, downsample_by_2)

    def table(self, ts_end_us: Optional[torch.Tensor] = None) -> EventTable:
        """The decoded events as a stream table (uploaded and decoded once); with ts_end_us, pointing at those window ends."""
        if self.device is None:
            raise RuntimeError('Recording(device=...) is needed to decode the events')
        if self._decoder is None:
            self._decoder, _ = DatDecoder.load_dat(self.dat_path, self.device, self.coord, self.repair)
        return self._decoder.table if ts_end_us is None else self._decoder.set_window_ends(ts_end_us)
