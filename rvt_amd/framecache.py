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
STATUS_CAPACITY, STATUS_INDEX = 1, 2
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
    Gf, Sf = geometry(E)
    dev = x.device
    if out is None:
        cap = F * E if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError(f'capacity {cap} is negative')
        out = PackedFrames(frame_shape, _DTYPES[name], torch.empty(F, Gf, dtype=torch.int64, device=dev),
                           torch.empty(F, Sf + 1, dtype=torch.int32, device=dev), torch.empty(F + 1, dtype=torch.int64, device=dev),
                           torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
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
        if index.dtype != torch.int64 or index.device != dev or not index.is_contiguous():
            raise ValueError(f'index must be a contiguous int64 tensor on {dev}')
        Fout = index.numel()
        if Fout < 1:
            raise ValueError('index is empty')
    lead = tuple(leading_shape) if leading_shape is not None else ((F,) if index is None else tuple(index.shape))
    if math.prod(lead) != Fout:
        raise ValueError(f'leading_shape {lead} does not hold the {Fout} frames asked for')
    shape = lead + tuple(packed.frame_shape)
    if out is None:
        out = torch.empty(shape, dtype=packed.dtype, device=dev)
    elif tuple(out.shape) != shape or out.dtype != packed.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be contiguous {packed.dtype} {shape} on {dev}')
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
    if planes_table.dtype != torch.int32 or planes_table.dim() != 2 or planes_table.shape[1] != 8:
        raise ValueError('planes_table must be int32 [B][8]')
    if planes_table.device != dev or not planes_table.is_contiguous():
        raise ValueError(f'planes_table must be contiguous on {dev}')
    B = planes_table.shape[0]
    if index.dtype != torch.int64 or index.device != dev or not index.is_contiguous():
        raise ValueError(f'index must be a contiguous int64 tensor on {dev}')
    if index.dim() != 2 or index.shape[1] != B or index.shape[0] < 1 or B < 1:
        raise ValueError(f'index must be (T, B={B}) like the rows of planes_table, got {tuple(index.shape)}')
    C, H, W = packed.frame_shape
    shape = tuple(index.shape) + (C, H, W)
    if out is None:
        out = torch.empty(shape, dtype=packed.dtype, device=dev)
    elif tuple(out.shape) != shape or out.dtype != packed.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out must be contiguous {packed.dtype} {shape} on {dev}')
    n = packed.values.numel()
    L.call('rvt_frames_unpack_augment', L.ptr(packed.masks), L.ptr(packed.seg_offset), L.ptr(packed.value_base),
           L.ptr(packed.values) if n else None, n, F, E, L.ptr(index), index.numel(), L.ptr(planes_table), B, C, H, W, L.ptr(out),
           L.ptr(packed.status), L.stream_of(out))
    return out
