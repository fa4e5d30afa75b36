"""Sparse frame cache: built event tensors kept as a bitmap plus their non-zero bytes, packed on the device and unpacked by
frame index (rvt_amd/csrc/framecache.hpp; format version 1 is stated in include/rvt_hip.h).

The device counterpart of the reference's compressed pre-processed store (uint8 histograms, blosc/zstd in H5, read by
data/genx_utils/sequence_base.py:92-102).  H5 and blosc stay out of scope; what this module keeps is the property that matters:
event tensors built once stay small, and a sampler fetches frames by index.

  * ``pack_frames(x)``: a uint8 / int8 tensor ``(..., C, H, W)`` -> ``PackedFrames`` (four launches, no host synchronisation).
  * ``unpack_frames(packed, index)``: frames by index -> ``index.shape + (C, H, W)``; ``-1`` is a zero frame.  One launch.
  * ``unpack_augment(packed, index, planes_table)``: the same followed by ``augment.augment_planes``, in one launch, bit for bit.
  * ``PackedFrames.slice`` / ``concat`` / ``save`` / ``load``: host side, plain numpy / CPU torch, no kernel.  ``load`` validates
    the arrays before anything reaches a kernel.
  * ``FrameGather(stores, device)`` / ``gather_frames(stores, global_index)``: frames of several packed sets, on the device or in
    pinned host memory, fetched by the device into one packed set (one call, no packed byte through host code).

Intended flow: ``load`` a recording's packed frames into pinned host memory, ``slice`` and ``concat`` the frames a batch needs,
one ``to(device)``, then one ``unpack_frames`` with an index laid out ``(T, B)``.

The arrays are torch tensors of the signed type of the same width (torch has no arithmetic on uint64 / uint32): ``masks`` int64
``[F][Gf]``, ``seg_offset`` int32 ``[F][Sf + 1]`` (a frame holds fewer than 2^31 bytes), ``value_base`` int64 ``[F + 1]``,
``values`` uint8 ``[capacity]``, ``status`` int32 ``[1]``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

VERSION = 1
GROUP_BYTES = 64
SEGMENT_BYTES = 64 * GROUP_BYTES
STATUS_CAPACITY, STATUS_INDEX, STATUS_COUNT = (L.ENUMS['RVT_FRAMES_STATUS_' + k] for k in ('CAPACITY', 'INDEX', 'COUNT'))
GATHER_COLS = L.ENUMS['RVT_FRAMES_GATHER_COLS']                  # int64 columns of a gather table row: masks, seg_offset, values, count
_DTYPES = {'uint8': torch.uint8, 'int8': torch.int8}


def geometry(E: int) -> Tuple[int, int]:
    """(Gf, Sf): groups and segments of a frame of E bytes."""
    Gf = (E + GROUP_BYTES - 1) // GROUP_BYTES
    return Gf, (Gf + 63) // 64


def packed_nbytes(F: int, E: int, nnz: int) -> int:
    """Bytes of a packed set, status excluded: 8 Gf F + 4 (Sf + 1) F + 8 (F + 1) + nnz."""
    Gf, Sf = geometry(E)
    return 8 * Gf * F + 4 * (Sf + 1) * F + 8 * (F + 1) + nnz


def _dtype_name(dt: torch.dtype) -> str:
    for k, v in _DTYPES.items():
        if v == dt:
            return k
    raise TypeError(f'frames are uint8 or int8 byte planes, got {dt}')


@dataclass(eq=False)
class PackedFrames:
    frame_shape: Tuple[int, ...]
    dtype: torch.dtype
    masks: Tensor
    seg_offset: Tensor
    value_base: Tensor
    values: Tensor
    status: Tensor

    @staticmethod
    def empty(frame_shape: Sequence[int], dtype: torch.dtype, num_frames: int, capacity: int, device, pin: bool = False,
              zero: bool = False) -> 'PackedFrames':
        """A packed set with rows for num_frames frames and room for `capacity` value bytes; zero: every array zeroed (else only
        allocated: status too); pin: in pinned host memory."""
        F, (Gf, Sf) = num_frames, geometry(math.prod(frame_shape))

        def make(*shape, dt):
            t = (torch.zeros if zero else torch.empty)(*shape, dtype=dt, device=device)
            return t.pin_memory() if pin else t
        return PackedFrames(tuple(frame_shape), dtype, make(F, Gf, dt=torch.int64), make(F, Sf + 1, dt=torch.int32),
                            make(F + 1, dt=torch.int64), make(capacity, dt=torch.uint8), make(1, dt=torch.int32))

    @property
    def num_frames(self) -> int:
        return self.masks.shape[0]

    @property
    def frame_bytes(self) -> int:
        return math.prod(self.frame_shape)

    @property
    def device(self) -> torch.device:
        return self.masks.device

    def nnz(self) -> int:
        """Non-zero bytes of all frames (reads value_base[F]: synchronises)."""
        return int(self.value_base[-1])

    @property
    def nbytes(self) -> int:
        return packed_nbytes(self.num_frames, self.frame_bytes, self.nnz())

    def check(self) -> 'PackedFrames':
        """Synchronise and raise on any status bit."""
        st = int(self.status[0])
        if st & STATUS_CAPACITY:
            raise RuntimeError(f'pack_frames ran out of capacity: {self.nnz()} non-zero bytes, room for {self.values.numel()}')
        if st & STATUS_INDEX:
            raise RuntimeError(f'unpack_frames met an index outside [-1, {self.num_frames})')
        if st & STATUS_COUNT:
            raise RuntimeError(f'gather_frames met a table row whose count is outside [0, {self.frame_bytes}] (taken as 0)')
        if st:
            raise RuntimeError(f'unknown frame-cache status {st}')
        return self

    def trim(self) -> 'PackedFrames':
        """Narrow `values` to the nnz bytes in use (a view; synchronises)."""
        self.check()
        self.values = self.values[:self.nnz()]
        return self

    def _map(self, fn) -> 'PackedFrames':
        return PackedFrames(self.frame_shape, self.dtype, fn(self.masks), fn(self.seg_offset), fn(self.value_base), fn(self.values),
                            fn(self.status))

    def to(self, device, non_blocking: bool = False) -> 'PackedFrames':
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> 'PackedFrames':
        return self._map(lambda t: t.pin_memory())

    # ---- host side: no kernel ----
    def _host(self, what: str) -> None:
        if self.device.type != 'cpu':
            raise RuntimeError(f'PackedFrames.{what} works on host arrays: call .to("cpu") first')

    def slice(self, start: int, stop: int) -> 'PackedFrames':
        """Frames [start, stop) as a packed set of their own: views of masks / seg_offset / values, value_base rebased."""
        self._host('slice')
        F = self.num_frames
        if not 0 <= start <= stop <= F:
            raise IndexError(f'slice [{start}, {stop}) outside the {F} frames')
        vb = self.value_base[start:stop + 1]
        lo, hi = int(vb[0]), int(vb[-1])
        if hi > self.values.numel():
            raise RuntimeError(f'values hold {self.values.numel()} bytes, frame {stop - 1} ends at {hi}: the pack ran out of capacity')
        return PackedFrames(self.frame_shape, self.dtype, self.masks[start:stop], self.seg_offset[start:stop], vb - lo,
                            self.values[lo:hi], torch.zeros(1, dtype=torch.int32))

    def save(self, path) -> None:
        """One uncompressed .npz: the arrays (values trimmed to nnz) plus version, frame_shape and dtype."""
        self._host('save')
        self.check()
        with open(path, 'wb') as f:
            np.savez(f, version=np.int64(VERSION), frame_shape=np.asarray(self.frame_shape, dtype=np.int64),
                     dtype=np.str_(_dtype_name(self.dtype)), masks=self.masks.numpy().view(np.uint64),
                     seg_offset=self.seg_offset.numpy().view(np.uint32), value_base=self.value_base.numpy(),
                     values=self.values[:self.nnz()].numpy())


def validate(frame_shape: Sequence[int], masks: np.ndarray, seg_offset: np.ndarray, value_base: np.ndarray, values: np.ndarray) -> None:
    """Raise ValueError naming the defect unless the arrays are a consistent version-1 packed set (numpy, host)."""
    E = math.prod(int(d) for d in frame_shape)
    if E < 1 or E >= 1 << 31:
        raise ValueError(f'frame_shape {tuple(frame_shape)}: a frame holds 1 .. 2^31 - 1 bytes')
    Gf, Sf = geometry(E)
    if masks.dtype != np.uint64 or masks.ndim != 2 or masks.shape[1] != Gf:
        raise ValueError(f'masks must be uint64 [F][{Gf}], got {masks.dtype} {masks.shape}')
    F = masks.shape[0]
    if seg_offset.dtype != np.uint32 or seg_offset.shape != (F, Sf + 1):
        raise ValueError(f'seg_offset must be uint32 [{F}][{Sf + 1}], got {seg_offset.dtype} {seg_offset.shape}')
    if value_base.dtype != np.int64 or value_base.shape != (F + 1,):
        raise ValueError(f'value_base must be int64 [{F + 1}], got {value_base.dtype} {value_base.shape}')
    if values.dtype != np.uint8 or values.ndim != 1:
        raise ValueError(f'values must be a uint8 vector, got {values.dtype} {values.shape}')
    if E % GROUP_BYTES and F and np.any(masks[:, -1] >> np.uint64(E % GROUP_BYTES)):
        raise ValueError(f'tail bits set in masks: the last group of a frame holds {E % GROUP_BYTES} bytes')
    if value_base[0] != 0 or np.any(np.diff(value_base) < 0):
        raise ValueError('value_base is not monotone from 0')
    if int(value_base[-1]) != values.shape[0]:
        raise ValueError(f'value_base[F] = {int(value_base[-1])} but values hold {values.shape[0]} bytes')
    pop = np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(F, Gf * 8), axis=1).reshape(F, Gf, 64).sum(axis=2, dtype=np.int64)
    seg = np.zeros((F, Sf * 64), dtype=np.int64)
    seg[:, :Gf] = pop
    want = np.zeros((F, Sf + 1), dtype=np.int64)
    np.cumsum(seg.reshape(F, Sf, 64).sum(axis=2), axis=1, out=want[:, 1:])
    if not np.array_equal(want, seg_offset.astype(np.int64)):
        f, s = np.argwhere(want != seg_offset.astype(np.int64))[0]
        raise ValueError(f'popcount of masks disagrees with seg_offset at frame {f}, entry {s}: {want[f, s]} against {seg_offset[f, s]}')
    if not np.array_equal(np.diff(value_base), want[:, -1]):
        raise ValueError('value_base disagrees with the frames\' non-zero counts in seg_offset')
    if np.any(values == 0):
        raise ValueError('values hold a zero byte')


def load(path) -> PackedFrames:
    """Read a file written by `save` and validate it before anything reaches a kernel."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ('version', 'frame_shape', 'dtype', 'masks', 'seg_offset', 'value_base', 'values') if k not in z.files]
        if missing:
            raise ValueError(f'{path}: not a packed-frames file, {missing} missing')
        if int(z['version']) != VERSION:
            raise ValueError(f'{path}: format version {int(z["version"])}, this reader knows version {VERSION}')
        name = str(z['dtype'])
        if name not in _DTYPES:
            raise ValueError(f'{path}: dtype {name!r} is neither uint8 nor int8')
        shape = tuple(int(d) for d in z['frame_shape'])
        arrs = [z[k] for k in ('masks', 'seg_offset', 'value_base', 'values')]
    validate(shape, *arrs)
    masks, seg_offset, value_base, values = arrs
    return PackedFrames(shape, _DTYPES[name], torch.from_numpy(masks.view(np.int64)), torch.from_numpy(seg_offset.view(np.int32)),
                        torch.from_numpy(value_base), torch.from_numpy(values), torch.zeros(1, dtype=torch.int32))


def concat(parts: Sequence[PackedFrames]) -> PackedFrames:
    """The frames of `parts` one behind the other (host side)."""
    parts = list(parts)
    if not parts:
        raise ValueError('concat of no packed sets')
    for p in parts:
        p._host('concat')
        if p.frame_shape != parts[0].frame_shape or p.dtype != parts[0].dtype:
            raise ValueError(f'concat of {p.dtype} frames {p.frame_shape} with {parts[0].dtype} frames {parts[0].frame_shape}')
    counts = [p.nnz() for p in parts]
    for p, n in zip(parts, counts):
        if n > p.values.numel():
            raise RuntimeError(f'values hold {p.values.numel()} bytes of {n}: the pack ran out of capacity')
    bases, at = [], 0
    for p, n in zip(parts, counts):
        bases.append(p.value_base[:-1] + at)
        at += n
    bases.append(torch.tensor([at], dtype=torch.int64))
    return PackedFrames(parts[0].frame_shape, parts[0].dtype, torch.cat([p.masks for p in parts]), torch.cat([p.seg_offset for p in parts]),
                        torch.cat(bases), torch.cat([p.values[:n] for p, n in zip(parts, counts)]), torch.zeros(1, dtype=torch.int32))


# ---- device side ----
def _bytes(t: Tensor) -> Tensor:
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


def _check_set(p: PackedFrames) -> Tuple[int, int]:
    F, E = p.num_frames, p.frame_bytes
    Gf, Sf = geometry(E)
    dev = p.device
    for name, t, dt, shape in (('masks', p.masks, torch.int64, (F, Gf)), ('seg_offset', p.seg_offset, torch.int32, (F, Sf + 1)),
                               ('value_base', p.value_base, torch.int64, (F + 1,)), ('status', p.status, torch.int32, (1,))):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous {dt} {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    if p.values.dtype != torch.uint8 or p.values.dim() != 1 or p.values.device != dev or not p.values.is_contiguous():
        raise ValueError(f'values must be a contiguous uint8 vector on {dev}')
    return F, E


def pack_frames(x: Tensor, capacity: Optional[int] = None, out: Optional[PackedFrames] = None) -> PackedFrames:
    """x: contiguous uint8 / int8 (..., C, H, W); the leading dimensions flatten to F frames.  capacity = room for non-zero bytes
    (None: the worst case F * E); out: a PackedFrames of the same F and frame shape whose arrays are overwritten (nothing is
    allocated then).  Does not synchronise: `check()` / `nnz()` do, and say whether the capacity sufficed."""
    name = _dtype_name(x.dtype)
    if x.dim() < 3:
        raise ValueError(f'frames are (..., C, H, W), got {tuple(x.shape)}')
    if not x.is_contiguous():
        raise ValueError('frames must be contiguous')
    frame_shape = tuple(x.shape[-3:])
    E, F = math.prod(frame_shape), math.prod(x.shape[:-3])
    if F < 1 or E < 1:
        raise ValueError(f'no bytes to pack in {tuple(x.shape)}')
    dev = x.device
    if out is None:
        cap = F * E if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError(f'capacity {cap} is negative')
        out = PackedFrames.empty(frame_shape, _DTYPES[name], F, cap, dev)
    else:
        if out.frame_shape != frame_shape or out.dtype != x.dtype or out.num_frames != F or out.device != dev:
            raise ValueError(f'out holds {out.num_frames} {out.dtype} frames {out.frame_shape} on {out.device}, x is {F} {x.dtype} frames '
                             f'{frame_shape} on {dev}')
        _check_set(out)
        cap = out.values.numel() if capacity is None else int(capacity)
        if not 0 <= cap <= out.values.numel():
            raise ValueError(f'capacity {cap} outside out.values ({out.values.numel()} bytes)')
    ws_bytes = int(L.get_lib().rvt_frames_pack_ws_bytes(F, E))
    if ws_bytes == 0:
        raise ValueError(f'{F} frames of {E} bytes are outside the supported range (E < 2^31)')
    st, ws = L.workspace('frames_pack', x, ws_bytes, torch.uint8)
    L.call('rvt_frames_pack', L.ptr(x), F, E, L.ptr(out.masks), L.ptr(out.seg_offset), L.ptr(out.value_base),
           L.ptr(out.values) if cap else None, cap, L.ptr(out.status), L.ptr(ws), ws_bytes, st)
    return out


def _check_index(index: Tensor, dev) -> None:
    if index.dtype != torch.int64 or index.device != dev or not index.is_contiguous():
        raise ValueError(f'index must be a contiguous int64 tensor on {dev}')


def _out_like(packed: PackedFrames, shape: Tuple[int, ...], out: Optional[Tensor]) -> Tensor:
    """`out` checked against the shape an unpack gives, or a new tensor of it."""
    dev = packed.device
    if out is None:
        return torch.empty(shape, dtype=packed.dtype, device=dev)
    if tuple(out.shape) != shape or out.dtype != packed.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be contiguous {packed.dtype} {shape} on {dev}')
    return out


def unpack_frames(packed: PackedFrames, index: Optional[Tensor] = None, out: Optional[Tensor] = None,
                  leading_shape: Optional[Sequence[int]] = None) -> Tensor:
    """Frames of `packed` by index -> a tensor of packed.dtype shaped leading_shape + frame_shape (leading_shape: index.shape, or
    (F,) without an index), e.g. an index laid out (T, B) gives the (T, B, C, H, W) that augment_planes / forward_sequence take.
    index: int64 on the device of `packed`; None = every frame in order; -1 = a zero frame; any other index outside [0, F) gives a
    zero frame and sets a status bit that `packed.check()` raises on.  With `out` given nothing is allocated."""
    F, E = _check_set(packed)
    dev = packed.device
    if index is None:
        Fout = F
    else:
        _check_index(index, dev)
        Fout = index.numel()
        if Fout < 1:
            raise ValueError('index is empty')
    lead = tuple(leading_shape) if leading_shape is not None else ((F,) if index is None else tuple(index.shape))
    if math.prod(lead) != Fout:
        raise ValueError(f'leading_shape {lead} does not hold the {Fout} frames asked for')
    out = _out_like(packed, lead + tuple(packed.frame_shape), out)
    n = packed.values.numel()
    L.call('rvt_frames_unpack', L.ptr(packed.masks), L.ptr(packed.seg_offset), L.ptr(packed.value_base),
           L.ptr(packed.values) if n else None, n, F, E, None if index is None else L.ptr(index), Fout, L.ptr(out), L.ptr(packed.status),
           L.stream_of(out))
    return out


def unpack_augment(packed: PackedFrames, index: Tensor, planes_table: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """`augment_planes(unpack_frames(packed, index), planes_table)` in one launch, bit for bit, without the dense tensor between
    the two (rvt_frames_unpack_augment).  index: int64 (T, B) on the device of `packed`, -1 = a zero frame whatever the table says,
    any other index outside [0, F) a zero frame and the status bit `packed.check()` raises on; planes_table: the int32 [B][8]
    table of `augment.make_tables` / `write_tables`, sample b = column b of the index.  Returns index.shape + frame_shape of
    packed.dtype (bytes are moved, never interpreted); with `out` given nothing is allocated."""
    F, E = _check_set(packed)
    dev = packed.device
    if len(packed.frame_shape) != 3:
        raise ValueError(f'frames must be (C, H, W) planes, the packed set holds {packed.frame_shape}')
    cols = L.ENUMS['RVT_AUGMENT_PLANES_COLS']
    if planes_table.dtype != torch.int32 or planes_table.dim() != 2 or planes_table.shape[1] != cols:
        raise ValueError(f'planes_table must be int32 [B][{cols}]')
    if planes_table.device != dev or not planes_table.is_contiguous():
        raise ValueError(f'planes_table must be contiguous on {dev}')
    B = planes_table.shape[0]
    _check_index(index, dev)
    if index.dim() != 2 or index.shape[1] != B or index.shape[0] < 1 or B < 1:
        raise ValueError(f'index must be (T, B={B}) like the rows of planes_table, got {tuple(index.shape)}')
    C, H, W = packed.frame_shape
    out = _out_like(packed, tuple(index.shape) + (C, H, W), out)
    n = packed.values.numel()
    L.call('rvt_frames_unpack_augment', L.ptr(packed.masks), L.ptr(packed.seg_offset), L.ptr(packed.value_base),
           L.ptr(packed.values) if n else None, n, F, E, L.ptr(index), index.numel(), L.ptr(planes_table), B, C, H, W, L.ptr(out),
           L.ptr(packed.status), L.stream_of(out))
    return out


# ---- gather: frames by address out of several stores, pinned host memory included ----
class FrameGather:
    """The frames of `stores` (PackedFrames of one frame shape and dtype, on `device` or in pinned host memory) under one global
    frame numbering, store after store, fetched by the device itself (rvt_frames_gather, rvt_amd/csrc/frames_gather.hpp): the
    host writes one int64 [4] row per frame (`table`), the launch copies masks, seg_offset rows and value bytes straight from
    where they lie into a packed set on the device and makes its value_base.  Keeps a reference to every source tensor: the
    kernel reads raw addresses, so the stores must neither be freed nor moved while a launch can still run."""

    def __init__(self, stores: Sequence[PackedFrames], device):
        stores = list(stores)
        if not stores:
            raise ValueError('no packed sets to gather from')
        self.device = dev = torch.device(device)
        if dev.type == 'cuda' and dev.index is None:
            self.device = dev = torch.device('cuda', torch.cuda.current_device())
        self.frame_shape, self.dtype = tuple(stores[0].frame_shape), stores[0].dtype
        E = self.frame_bytes = math.prod(self.frame_shape)
        Gf, Sf = geometry(E)
        self._keep, rows = [], []
        for k, s in enumerate(stores):
            if tuple(s.frame_shape) != self.frame_shape or s.dtype != self.dtype:
                raise ValueError(f'store {k} holds {s.dtype} frames {tuple(s.frame_shape)}, store 0 {self.dtype} frames {self.frame_shape}')
            _check_set(s)
            for name, t in (('masks', s.masks), ('seg_offset', s.seg_offset), ('values', s.values)):
                if t.device.type == 'cpu':
                    if dev.type != 'cpu' and t.numel() and not t.is_pinned():      # (an empty array is never read)
                        raise ValueError(f'store {k}: {name} lies in pageable host memory; the device reads pinned memory only (pin_memory())')
                elif t.device != dev:
                    raise ValueError(f'store {k}: {name} is on {t.device}, the gather runs on {dev}')
            vb = s.value_base.cpu().numpy()
            if int(vb[-1]) > s.values.numel():
                raise ValueError(f'store {k}: values hold {s.values.numel()} bytes of {int(vb[-1])}: the pack ran out of capacity')
            F = s.num_frames
            f = np.arange(F, dtype=np.int64)
            r = np.empty((F, GATHER_COLS), dtype=np.int64)
            r[:, 0] = s.masks.data_ptr() + 8 * Gf * f
            r[:, 1] = s.seg_offset.data_ptr() + 4 * (Sf + 1) * f
            r[:, 2] = s.values.data_ptr() + vb[:-1]
            r[:, 3] = np.diff(vb)
            rows.append(r)
            self._keep.append((s.masks, s.seg_offset, s.values))
        self.base = np.concatenate(([0], np.cumsum([r.shape[0] for r in rows]))).astype(np.int64)      # global number of each store's frame 0
        self._rows = np.concatenate(rows)
        self.value_base = np.concatenate(([0], np.cumsum(self._rows[:, 3]))).astype(np.int64)                # of the concatenated stores
        self.max_count = int(self._rows[:, 3].max()) if len(self._rows) else 0

    @property
    def num_frames(self) -> int:
        return int(self.base[-1])

    def table(self, global_index, out: Optional[np.ndarray] = None) -> np.ndarray:
        """int64 [n][4] rows of the frames `global_index` names, in its (flattened) order; into out[:n] when given."""
        idx = np.asarray(global_index, dtype=np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.num_frames):
            raise IndexError(f'frame index outside [0, {self.num_frames})')
        if out is None:
            return self._rows[idx]
        return np.take(self._rows, idx, axis=0, out=out[:idx.size])

    def _check_out(self, out: PackedFrames, n: int) -> None:
        if tuple(out.frame_shape) != self.frame_shape or out.dtype != self.dtype:
            raise ValueError(f'out holds {out.dtype} frames {tuple(out.frame_shape)}, the stores {self.dtype} frames {self.frame_shape}')
        _check_set(out)
        if out.device != self.device:
            raise ValueError(f'out is on {out.device}, the gather runs on {self.device}')
        if out.num_frames < n:
            raise ValueError(f'out has rows for {out.num_frames} frames, {n} are asked for')

    def launch(self, table_dev: Tensor, n: int, out: PackedFrames, max_blocks: int = 0) -> PackedFrames:
        """The launch alone, on the current stream: table_dev holds the n rows already (or will, by a copy enqueued before on the
        same stream).  Writes rows [0, n) of out.masks / seg_offset, out.value_base[0 .. n], the value bytes and out.status."""
        self._check_out(out, n)
        if table_dev.dtype != torch.int64 or table_dev.device != self.device or not table_dev.is_contiguous() or table_dev.numel() < GATHER_COLS * n:
            raise ValueError(f'table_dev must be a contiguous int64 tensor of at least {GATHER_COLS * n} entries on {self.device}')
        cap = out.values.numel()
        L.call('rvt_frames_gather', L.ptr(table_dev), n, self.frame_bytes, L.ptr(out.masks), L.ptr(out.seg_offset), L.ptr(out.value_base),
               L.ptr(out.values) if cap else None, cap, L.ptr(out.status), int(max_blocks), L.stream_of(out.masks))
        return out

    def gather(self, global_index, out: PackedFrames, table_dev: Optional[Tensor] = None, max_blocks: int = 0,
               rows: Optional[np.ndarray] = None) -> PackedFrames:
        """Frames `global_index` (any shape, flattened) into rows [0, n) of `out`, on the current stream; returns out.  rows: the
        int64 [n][4] table itself instead of an index (global_index None).  table_dev: a device int64 buffer the rows are copied to
        (none given: one is allocated).  Does not synchronise: out.check() says whether out.values had room."""
        if rows is None:
            rows = self.table(global_index)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.ndim != 2 or rows.shape[1] != GATHER_COLS:
                raise ValueError(f'rows must be int64 [n][{GATHER_COLS}], got {rows.shape}')
        n = rows.shape[0]
        self._check_out(out, n)
        if n == 0:
            return out
        host = torch.from_numpy(rows.reshape(-1))
        if table_dev is None:
            table_dev = host.to(self.device)
        else:
            if table_dev.dtype != torch.int64 or table_dev.device != self.device or table_dev.dim() != 1 or table_dev.numel() < host.numel():
                raise ValueError(f'table_dev must be a flat int64 tensor of at least {host.numel()} entries on {self.device}')
            table_dev[:host.numel()].copy_(host)
        return self.launch(table_dev, n, out, max_blocks)

    def empty(self, n: int, capacity: int) -> PackedFrames:
        """An uninitialised packed set on the device with rows for n frames and room for `capacity` value bytes."""
        out = PackedFrames.empty(self.frame_shape, self.dtype, n, capacity, self.device)
        out.status.zero_()
        return out


def gather_frames(stores: Sequence[PackedFrames], global_index, out: Optional[PackedFrames] = None) -> PackedFrames:
    """One-shot FrameGather: frames `global_index` of the concatenation of `stores` as a packed set on the device of `out`
    (none given: on the stores' device, the current GPU for host stores, sized exactly)."""
    stores = list(stores)
    if out is not None:
        dev = out.device
    elif stores and stores[0].device.type == 'cuda':
        dev = stores[0].device
    elif L.is_emulator():
        dev = torch.device('cpu')
    else:
        dev = torch.device('cuda', torch.cuda.current_device())
    g = FrameGather(stores, dev)
    rows = g.table(global_index)
    if out is None:
        out = g.empty(rows.shape[0], int(rows[:, 3].sum()))
    return g.gather(None, out, rows=rows)
