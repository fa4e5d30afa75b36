"""Sparse frame cache: built event tensors kept as a bitmap plus their non-zero bytes, packed on the device and unpacked by
frame index (rvt_amd/csrc/framecache.hpp; format versions 1 and 2 are stated in include/rvt_hip.h).

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

Format version 2 (``PackedFrames2``, ``pack_frames(x, version=2)``, rvt_amd/csrc/capi_frames2.hip) keeps a 64-bit mask only for
the 64-byte groups that hold a non-zero byte: ``group_mask`` int64 ``[F][Sf]`` (one bit per group), ``grp_offset`` int32
``[F][Sf + 1]``, ``mask_base`` int64 ``[F + 1]`` and the compacted ``masks`` int64 ``[mask_capacity]`` beside version 1's ``seg_offset``,
``value_base`` and ``values``.  Every module function takes either class and dispatches on it; ``convert`` goes between the two on
the host; ``unpack_augment`` reads version 1 only.  Nothing defaults to version 2.

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
GATHER2_COLS = L.ENUMS['RVT_FRAMES_GATHER2_COLS']                # version 2: group_mask, seg_offset, grp_offset, masks, values, count, groups, 0
VALUE_BITS = 8                                                   # bits of a stored value: what a version-2 file says and this reader takes
_DTYPES = {'uint8': torch.uint8, 'int8': torch.int8}


def geometry(E: int) -> Tuple[int, int]:
    """(Gf, Sf): groups and segments of a frame of E bytes."""
    Gf = (E + GROUP_BYTES - 1) // GROUP_BYTES
    return Gf, (Gf + 63) // 64


def packed_nbytes(F: int, E: int, nnz: int) -> int:
    """Bytes of a packed set, status excluded: 8 Gf F + 4 (Sf + 1) F + 8 (F + 1) + nnz."""
    Gf, Sf = geometry(E)
    return 8 * Gf * F + 4 * (Sf + 1) * F + 8 * (F + 1) + nnz


def packed_nbytes2(F: int, E: int, ngroups: int, nnz: int) -> int:
    """Bytes of a version-2 packed set, status excluded: 16 Sf F + 8 F + 16 (F + 1) + 8 ngroups + nnz."""
    Sf = geometry(E)[1]
    return 16 * Sf * F + 8 * F + 16 * (F + 1) + 8 * ngroups + nnz


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


@dataclass(eq=False)
class PackedFrames2:
    """A packed set of format version 2: the surface of `PackedFrames`, with a mask only for the non-empty groups."""
    frame_shape: Tuple[int, ...]
    dtype: torch.dtype
    group_mask: Tensor
    seg_offset: Tensor
    grp_offset: Tensor
    value_base: Tensor
    mask_base: Tensor
    masks: Tensor
    values: Tensor
    status: Tensor

    @staticmethod
    def empty(frame_shape: Sequence[int], dtype: torch.dtype, num_frames: int, capacity: int, mask_capacity: int, device,
              pin: bool = False, zero: bool = False) -> 'PackedFrames2':
        """A packed set with rows for num_frames frames, room for `capacity` value bytes and `mask_capacity` mask words; zero: every
        array zeroed (else only allocated: status too); pin: in pinned host memory."""
        F, (_, Sf) = num_frames, geometry(math.prod(frame_shape))

        def make(*shape, dt):
            t = (torch.zeros if zero else torch.empty)(*shape, dtype=dt, device=device)
            return t.pin_memory() if pin else t
        return PackedFrames2(tuple(frame_shape), dtype, make(F, Sf, dt=torch.int64), make(F, Sf + 1, dt=torch.int32),
                             make(F, Sf + 1, dt=torch.int32), make(F + 1, dt=torch.int64), make(F + 1, dt=torch.int64),
                             make(mask_capacity, dt=torch.int64), make(capacity, dt=torch.uint8), make(1, dt=torch.int32))

    @property
    def num_frames(self) -> int:
        return self.group_mask.shape[0]

    @property
    def frame_bytes(self) -> int:
        return math.prod(self.frame_shape)

    @property
    def device(self) -> torch.device:
        return self.group_mask.device

    def nnz(self) -> int:
        """Non-zero bytes of all frames (reads value_base[F]: synchronises)."""
        return int(self.value_base[-1])

    def ngroups(self) -> int:
        """Non-empty groups of all frames (reads mask_base[F]: synchronises)."""
        return int(self.mask_base[-1])

    @property
    def nbytes(self) -> int:
        return packed_nbytes2(self.num_frames, self.frame_bytes, self.ngroups(), self.nnz())

    def check(self) -> 'PackedFrames2':
        """Synchronise and raise on any status bit."""
        st = int(self.status[0])
        if st & STATUS_CAPACITY:
            raise RuntimeError(f'pack_frames ran out of capacity: {self.nnz()} non-zero bytes, room for {self.values.numel()}; '
                               f'{self.ngroups()} non-empty groups, room for {self.masks.numel()}')
        if st & STATUS_INDEX:
            raise RuntimeError(f'unpack_frames met an index outside [-1, {self.num_frames})')
        if st & STATUS_COUNT:
            raise RuntimeError(f'gather_frames met a table row whose count is outside [0, {self.frame_bytes}] or whose group count is '
                               f'outside [0, {geometry(self.frame_bytes)[0]}] (taken as 0)')
        if st:
            raise RuntimeError(f'unknown frame-cache status {st}')
        return self

    def trim(self) -> 'PackedFrames2':
        """Narrow `values` to the nnz bytes and `masks` to the ngroups words in use (views; synchronises)."""
        self.check()
        self.values = self.values[:self.nnz()]
        self.masks = self.masks[:self.ngroups()]
        return self

    def _arrays(self) -> Tuple[Tensor, ...]:
        return (self.group_mask, self.seg_offset, self.grp_offset, self.value_base, self.mask_base, self.masks, self.values, self.status)

    def _map(self, fn) -> 'PackedFrames2':
        return PackedFrames2(self.frame_shape, self.dtype, *(fn(t) for t in self._arrays()))

    def to(self, device, non_blocking: bool = False) -> 'PackedFrames2':
        return self._map(lambda t: t.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> 'PackedFrames2':
        return self._map(lambda t: t.pin_memory())

    # ---- host side: no kernel ----
    def _host(self, what: str) -> None:
        if self.device.type != 'cpu':
            raise RuntimeError(f'PackedFrames2.{what} works on host arrays: call .to("cpu") first')

    def slice(self, start: int, stop: int) -> 'PackedFrames2':
        """Frames [start, stop) as a packed set of their own: views of the rows, the masks and the values, both bases rebased."""
        self._host('slice')
        F = self.num_frames
        if not 0 <= start <= stop <= F:
            raise IndexError(f'slice [{start}, {stop}) outside the {F} frames')
        vb, mb = self.value_base[start:stop + 1], self.mask_base[start:stop + 1]
        lo, hi, mlo, mhi = int(vb[0]), int(vb[-1]), int(mb[0]), int(mb[-1])
        if hi > self.values.numel() or mhi > self.masks.numel():
            raise RuntimeError(f'values hold {self.values.numel()} bytes and masks {self.masks.numel()} words, frame {stop - 1} ends at '
                               f'{hi} and {mhi}: the pack ran out of capacity')
        return PackedFrames2(self.frame_shape, self.dtype, self.group_mask[start:stop], self.seg_offset[start:stop],
                             self.grp_offset[start:stop], vb - lo, mb - mlo, self.masks[mlo:mhi], self.values[lo:hi],
                             torch.zeros(1, dtype=torch.int32))

    def save(self, path) -> None:
        """One uncompressed .npz: the seven arrays (masks and values trimmed) plus version, value_bits, frame_shape and dtype."""
        self._host('save')
        self.check()
        with open(path, 'wb') as f:
            np.savez(f, version=np.int64(2), value_bits=np.int64(VALUE_BITS), frame_shape=np.asarray(self.frame_shape, dtype=np.int64),
                     dtype=np.str_(_dtype_name(self.dtype)), group_mask=self.group_mask.numpy().view(np.uint64),
                     seg_offset=self.seg_offset.numpy().view(np.uint32), grp_offset=self.grp_offset.numpy().view(np.uint32),
                     value_base=self.value_base.numpy(), mask_base=self.mask_base.numpy(),
                     masks=self.masks[:self.ngroups()].numpy().view(np.uint64), values=self.values[:self.nnz()].numpy())


_ARRAYS2 = ('group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base', 'masks', 'values')


def _popcount64(a: np.ndarray) -> np.ndarray:
    """Set bits of each word of a uint64 array, as int64 of the same shape."""
    a = np.ascontiguousarray(a)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1, dtype=np.int64).reshape(a.shape)


def _group_bits(group_mask: np.ndarray) -> np.ndarray:
    """bool [F][64 Sf]: is group g of the frame non-empty (bit g % 64 of word g / 64; the words are little-endian on every host
    this package runs on)."""
    F, Sf = group_mask.shape
    return np.unpackbits(np.ascontiguousarray(group_mask).view(np.uint8).reshape(F, Sf * 8), axis=1, bitorder='little').astype(bool)


def validate2(frame_shape: Sequence[int], group_mask: np.ndarray, seg_offset: np.ndarray, grp_offset: np.ndarray, value_base: np.ndarray,
              mask_base: np.ndarray, masks: np.ndarray, values: np.ndarray, value_bits: int = VALUE_BITS) -> None:
    """Raise ValueError naming the defect unless the arrays are a consistent version-2 packed set (numpy, host)."""
    if int(value_bits) != VALUE_BITS:
        raise ValueError(f'value_bits = {int(value_bits)}: this reader knows {VALUE_BITS}-bit values only')
    E = math.prod(int(d) for d in frame_shape)
    if E < 1 or E >= 1 << 31:
        raise ValueError(f'frame_shape {tuple(frame_shape)}: a frame holds 1 .. 2^31 - 1 bytes')
    Gf, Sf = geometry(E)
    if group_mask.dtype != np.uint64 or group_mask.ndim != 2 or group_mask.shape[1] != Sf:
        raise ValueError(f'group_mask must be uint64 [F][{Sf}], got {group_mask.dtype} {group_mask.shape}')
    F = group_mask.shape[0]
    for name, a in (('seg_offset', seg_offset), ('grp_offset', grp_offset)):
        if a.dtype != np.uint32 or a.shape != (F, Sf + 1):
            raise ValueError(f'{name} must be uint32 [{F}][{Sf + 1}], got {a.dtype} {a.shape}')
    for name, a in (('value_base', value_base), ('mask_base', mask_base)):
        if a.dtype != np.int64 or a.shape != (F + 1,):
            raise ValueError(f'{name} must be int64 [{F + 1}], got {a.dtype} {a.shape}')
        if a[0] != 0 or np.any(np.diff(a) < 0):
            raise ValueError(f'{name} is not monotone from 0')
    if masks.dtype != np.uint64 or masks.ndim != 1:
        raise ValueError(f'masks must be a uint64 vector, got {masks.dtype} {masks.shape}')
    if values.dtype != np.uint8 or values.ndim != 1:
        raise ValueError(f'values must be a uint8 vector, got {values.dtype} {values.shape}')
    if int(value_base[-1]) != values.shape[0]:
        raise ValueError(f'value_base[F] = {int(value_base[-1])} but values hold {values.shape[0]} bytes')
    if int(mask_base[-1]) != masks.shape[0]:
        raise ValueError(f'mask_base[F] = {int(mask_base[-1])} but masks hold {masks.shape[0]} words')
    live = _group_bits(group_mask)                                                  # [F][64 Sf]
    if np.any(live[:, Gf:]):
        raise ValueError(f'tail bits set in group_mask: a frame has {Gf} groups')
    per_seg = live.reshape(F, Sf, 64).sum(axis=2, dtype=np.int64)
    want_g = np.zeros((F, Sf + 1), dtype=np.int64)
    np.cumsum(per_seg, axis=1, out=want_g[:, 1:])
    if not np.array_equal(want_g, grp_offset.astype(np.int64)):
        f, s = np.argwhere(want_g != grp_offset.astype(np.int64))[0]
        raise ValueError(f'popcount of group_mask disagrees with grp_offset at frame {f}, entry {s}: {want_g[f, s]} against {grp_offset[f, s]}')
    if not np.array_equal(np.diff(mask_base), want_g[:, -1]):
        raise ValueError('mask_base disagrees with the frames\' non-empty group counts in grp_offset')
    if np.any(masks == 0):
        raise ValueError('masks hold a zero word: an empty group has no stored mask')
    if E % GROUP_BYTES and F:
        last = live[:, Gf - 1]                                                      # frames whose last, partial group is stored:
        words = masks[mask_base[1:][last] - 1]                                      # it is the last word of the frame's run
        if np.any(words >> np.uint64(E % GROUP_BYTES)):
            raise ValueError(f'tail bits set in masks: the last group of a frame holds {E % GROUP_BYTES} bytes')
    # the stored masks of a segment are a run of `masks`: word k belongs to segment seg_of[k] of the F * Sf in frame order
    seg_of = np.repeat(np.arange(F * Sf), per_seg.reshape(-1))
    got_s = np.bincount(seg_of, weights=_popcount64(masks), minlength=F * Sf).astype(np.int64).reshape(F, Sf)
    want_s = np.zeros((F, Sf + 1), dtype=np.int64)
    np.cumsum(got_s, axis=1, out=want_s[:, 1:])
    if not np.array_equal(want_s, seg_offset.astype(np.int64)):
        f, s = np.argwhere(want_s != seg_offset.astype(np.int64))[0]
        raise ValueError(f'popcount of masks disagrees with seg_offset at frame {f}, entry {s}: {want_s[f, s]} against {seg_offset[f, s]}')
    if not np.array_equal(np.diff(value_base), want_s[:, -1]):
        raise ValueError('value_base disagrees with the frames\' non-zero counts in seg_offset')
    if np.any(values == 0):
        raise ValueError('values hold a zero byte')


def convert(packed, version: int):
    """`packed` in the other format version (host side, numpy, no device): 1 -> 2 drops the masks of empty groups behind a bit per
    group, 2 -> 1 puts zero words back.  The same version returns `packed` itself.  seg_offset, value_base and values are shared
    forms: the result holds views of them (values trimmed to nnz)."""
    if version not in (1, 2):
        raise ValueError(f'format version {version}: this package knows versions 1 and 2')
    have = 2 if isinstance(packed, PackedFrames2) else 1
    if have == version:
        return packed
    packed._host('convert')
    packed.check()
    F, E = packed.num_frames, packed.frame_bytes
    Gf, Sf = geometry(E)
    nnz = packed.nnz()
    if nnz > packed.values.numel():
        raise RuntimeError(f'values hold {packed.values.numel()} bytes of {nnz}: the pack ran out of capacity')
    status = torch.zeros(1, dtype=torch.int32)
    if version == 2:
        m1 = packed.masks.numpy().view(np.uint64)
        live = np.zeros((F, Sf * 64), dtype=bool)
        live[:, :Gf] = m1 != 0
        group_mask = np.packbits(live, axis=1, bitorder='little').view(np.uint64).reshape(F, Sf)
        grp_offset = np.zeros((F, Sf + 1), dtype=np.int64)
        np.cumsum(live.reshape(F, Sf, 64).sum(axis=2, dtype=np.int64), axis=1, out=grp_offset[:, 1:])
        mask_base = np.zeros(F + 1, dtype=np.int64)
        np.cumsum(grp_offset[:, -1], out=mask_base[1:])
        masks = m1[live[:, :Gf]]                                                    # row-major selection: frame order, then group order
        return PackedFrames2(packed.frame_shape, packed.dtype, torch.from_numpy(group_mask.view(np.int64)), packed.seg_offset,
                             torch.from_numpy(grp_offset.astype(np.uint32).view(np.int32)), packed.value_base, torch.from_numpy(mask_base),
                             torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)), packed.values[:nnz], status)
    ng = packed.ngroups()
    if ng > packed.masks.numel():
        raise RuntimeError(f'masks hold {packed.masks.numel()} words of {ng}: the pack ran out of capacity')
    live = _group_bits(packed.group_mask.numpy().view(np.uint64))[:, :Gf]
    if int(live.sum()) != ng:
        raise ValueError(f'group_mask names {int(live.sum())} non-empty groups, mask_base[F] = {ng}')
    m1 = np.zeros((F, Gf), dtype=np.uint64)
    m1[live] = packed.masks.numpy().view(np.uint64)[:ng]
    return PackedFrames(packed.frame_shape, packed.dtype, torch.from_numpy(m1.view(np.int64)), packed.seg_offset, packed.value_base,
                        packed.values[:nnz], status)


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


def _load2(path, z) -> PackedFrames2:
    missing = [k for k in ('value_bits', 'frame_shape', 'dtype') + _ARRAYS2 if k not in z.files]
    if missing:
        raise ValueError(f'{path}: not a version-2 packed-frames file, {missing} missing')
    name = str(z['dtype'])
    if name not in _DTYPES:
        raise ValueError(f'{path}: dtype {name!r} is neither uint8 nor int8')
    shape = tuple(int(d) for d in z['frame_shape'])
    a = {k: z[k] for k in _ARRAYS2}
    validate2(shape, *(a[k] for k in _ARRAYS2), value_bits=int(z['value_bits']))
    signed = {'group_mask': np.int64, 'seg_offset': np.int32, 'grp_offset': np.int32, 'masks': np.int64}
    t = {k: torch.from_numpy(v.view(signed[k]) if k in signed else v) for k, v in a.items()}
    return PackedFrames2(shape, _DTYPES[name], *(t[k] for k in _ARRAYS2), torch.zeros(1, dtype=torch.int32))


def load(path):
    """Read a file written by `save` and validate it before anything reaches a kernel: a `PackedFrames` for a version-1 file, a
    `PackedFrames2` for a version-2 one."""
    with np.load(path, allow_pickle=False) as z:
        if 'version' in z.files and int(z['version']) == 2:
            return _load2(path, z)
        missing = [k for k in ('version', 'frame_shape', 'dtype', 'masks', 'seg_offset', 'value_base', 'values') if k not in z.files]
        if missing:
            raise ValueError(f'{path}: not a packed-frames file, {missing} missing')
        if int(z['version']) != VERSION:
            raise ValueError(f'{path}: format version {int(z["version"])}, this reader knows versions {VERSION} and 2')
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
    if any(isinstance(p, PackedFrames2) for p in parts):
        return _concat2(parts)
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


def _concat2(parts: Sequence[PackedFrames2]) -> PackedFrames2:
    """concat for version-2 sets: the rows one behind the other, both variable-length runs back to back, both bases rebased."""
    for p in parts:
        if not isinstance(p, PackedFrames2):
            raise ValueError('concat of packed sets of format versions 1 and 2: convert() one of them first')
        p._host('concat')
        if p.frame_shape != parts[0].frame_shape or p.dtype != parts[0].dtype:
            raise ValueError(f'concat of {p.dtype} frames {p.frame_shape} with {parts[0].dtype} frames {parts[0].frame_shape}')
    counts, groups = [p.nnz() for p in parts], [p.ngroups() for p in parts]
    for p, n, g in zip(parts, counts, groups):
        if n > p.values.numel() or g > p.masks.numel():
            raise RuntimeError(f'values hold {p.values.numel()} bytes of {n}, masks {p.masks.numel()} words of {g}: the pack ran out of capacity')
    vbs, mbs, at, mat = [], [], 0, 0
    for p, n, g in zip(parts, counts, groups):
        vbs.append(p.value_base[:-1] + at)
        mbs.append(p.mask_base[:-1] + mat)
        at += n
        mat += g
    vbs.append(torch.tensor([at], dtype=torch.int64))
    mbs.append(torch.tensor([mat], dtype=torch.int64))
    return PackedFrames2(parts[0].frame_shape, parts[0].dtype, torch.cat([p.group_mask for p in parts]), torch.cat([p.seg_offset for p in parts]),
                         torch.cat([p.grp_offset for p in parts]), torch.cat(vbs), torch.cat(mbs),
                         torch.cat([p.masks[:g] for p, g in zip(parts, groups)]), torch.cat([p.values[:n] for p, n in zip(parts, counts)]),
                         torch.zeros(1, dtype=torch.int32))


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


def _check_set2(p: PackedFrames2) -> Tuple[int, int]:
    F, E = p.num_frames, p.frame_bytes
    Sf = geometry(E)[1]
    dev = p.device
    for name, t, dt, shape in (('group_mask', p.group_mask, torch.int64, (F, Sf)), ('seg_offset', p.seg_offset, torch.int32, (F, Sf + 1)),
                               ('grp_offset', p.grp_offset, torch.int32, (F, Sf + 1)), ('value_base', p.value_base, torch.int64, (F + 1,)),
                               ('mask_base', p.mask_base, torch.int64, (F + 1,)), ('status', p.status, torch.int32, (1,))):
        if t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous {dt} {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    if p.masks.dtype != torch.int64 or p.masks.dim() != 1 or p.masks.device != dev or not p.masks.is_contiguous():
        raise ValueError(f'masks must be a contiguous int64 vector on {dev}')
    if p.values.dtype != torch.uint8 or p.values.dim() != 1 or p.values.device != dev or not p.values.is_contiguous():
        raise ValueError(f'values must be a contiguous uint8 vector on {dev}')
    return F, E


def _pack_frames2(x: Tensor, capacity: Optional[int], out: Optional[PackedFrames2], mask_capacity: Optional[int]) -> PackedFrames2:
    """pack_frames for format version 2 (rvt_frames_pack2)."""
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
        mcap = F * geometry(E)[0] if mask_capacity is None else int(mask_capacity)
        if cap < 0 or mcap < 0:
            raise ValueError(f'capacity {cap} / mask_capacity {mcap} is negative')
        out = PackedFrames2.empty(frame_shape, _DTYPES[name], F, cap, mcap, dev)
    else:
        if not isinstance(out, PackedFrames2):
            raise ValueError('version=2 needs a PackedFrames2 as out')
        if out.frame_shape != frame_shape or out.dtype != x.dtype or out.num_frames != F or out.device != dev:
            raise ValueError(f'out holds {out.num_frames} {out.dtype} frames {out.frame_shape} on {out.device}, x is {F} {x.dtype} frames '
                             f'{frame_shape} on {dev}')
        _check_set2(out)
        cap = out.values.numel() if capacity is None else int(capacity)
        mcap = out.masks.numel() if mask_capacity is None else int(mask_capacity)
        if not 0 <= cap <= out.values.numel():
            raise ValueError(f'capacity {cap} outside out.values ({out.values.numel()} bytes)')
        if not 0 <= mcap <= out.masks.numel():
            raise ValueError(f'mask_capacity {mcap} outside out.masks ({out.masks.numel()} words)')
    ws_bytes = int(L.get_lib().rvt_frames_pack2_ws_bytes(F, E))
    if ws_bytes == 0:
        raise ValueError(f'{F} frames of {E} bytes are outside the supported range (E < 2^31)')
    st, ws = L.workspace('frames_pack2', x, ws_bytes, torch.uint8)
    L.call('rvt_frames_pack2', L.ptr(x), F, E, L.ptr(out.group_mask), L.ptr(out.seg_offset), L.ptr(out.grp_offset), L.ptr(out.value_base),
           L.ptr(out.mask_base), L.ptr(out.masks) if mcap else None, mcap, L.ptr(out.values) if cap else None, cap, L.ptr(out.status),
           L.ptr(ws), ws_bytes, st)
    return out


def pack_frames(x: Tensor, capacity: Optional[int] = None, out=None, version: int = 1, mask_capacity: Optional[int] = None):
    """x: contiguous uint8 / int8 (..., C, H, W); the leading dimensions flatten to F frames.  capacity = room for non-zero bytes
    (None: the worst case F * E); out: a PackedFrames of the same F and frame shape whose arrays are overwritten (nothing is
    allocated then).  Does not synchronise: `check()` / `nnz()` do, and say whether the capacity sufficed.
    version=2 (or a PackedFrames2 as out) packs to format version 2 and returns a PackedFrames2; mask_capacity = room for the masks of
    non-empty groups (None: the worst case F * Gf)."""
    if version == 2 or isinstance(out, PackedFrames2):
        return _pack_frames2(x, capacity, out, mask_capacity)
    if version != 1:
        raise ValueError(f'format version {version}: this package knows versions 1 and 2')
    if mask_capacity is not None:
        raise ValueError('mask_capacity belongs to format version 2 (version=2)')
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
    zero frame and sets a status bit that `packed.check()` raises on.  With `out` given nothing is allocated.  `packed` is a
    PackedFrames or a PackedFrames2 (rvt_frames_unpack2)."""
    v2 = isinstance(packed, PackedFrames2)
    F, E = _check_set2(packed) if v2 else _check_set(packed)
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
    if v2:
        nm = packed.masks.numel()
        L.call('rvt_frames_unpack2', L.ptr(packed.group_mask), L.ptr(packed.seg_offset), L.ptr(packed.grp_offset), L.ptr(packed.value_base),
               L.ptr(packed.mask_base), L.ptr(packed.masks) if nm else None, nm, L.ptr(packed.values) if n else None, n, F, E,
               None if index is None else L.ptr(index), Fout, L.ptr(out), L.ptr(packed.status), L.stream_of(out))
        return out
    L.call('rvt_frames_unpack', L.ptr(packed.masks), L.ptr(packed.seg_offset), L.ptr(packed.value_base),
           L.ptr(packed.values) if n else None, n, F, E, None if index is None else L.ptr(index), Fout, L.ptr(out), L.ptr(packed.status),
           L.stream_of(out))
    return out


def unpack_augment(packed: PackedFrames, index: Tensor, planes_table: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """`augment_planes(unpack_frames(packed, index), planes_table)` in one launch, bit for bit, without the dense tensor between
    the two (rvt_frames_unpack_augment).  index: int64 (T, B) on the device of `packed`, -1 = a zero frame whatever the table says,
    any other index outside [0, F) a zero frame and the status bit `packed.check()` raises on; planes_table: the int32 [B][8]
    table of `augment.make_tables` / `write_tables`, sample b = column b of the index.  Returns index.shape + frame_shape of
    packed.dtype (bytes are moved, never interpreted); with `out` given nothing is allocated.  Format version 1 only."""
    if isinstance(packed, PackedFrames2):
        raise NotImplementedError('unpack_augment: the fused route (rvt_frames_unpack_augment) reads format version 1 only; for a '
                                  'PackedFrames2 use unpack_frames + augment.augment_planes, or convert(packed, 1)')
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
    """The frames of `stores` (PackedFrames, or PackedFrames2: all of one format version, of one frame shape and dtype, on `device` or in pinned host memory) under one global
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
        # format version of the stores (all of one): the table's columns and the entry point follow it
        self.version = v = 2 if isinstance(stores[0], PackedFrames2) else 1
        self.cols, self._count_col = (GATHER2_COLS, 5) if v == 2 else (GATHER_COLS, 3)
        self._keep, rows = [], []
        for k, s in enumerate(stores):
            if isinstance(s, PackedFrames2) != (v == 2):
                raise ValueError(f'store {k} is of format version {3 - v}, store 0 of version {v}: convert() them to one version')
            if tuple(s.frame_shape) != self.frame_shape or s.dtype != self.dtype:
                raise ValueError(f'store {k} holds {s.dtype} frames {tuple(s.frame_shape)}, store 0 {self.dtype} frames {self.frame_shape}')
            if v == 2:
                rows.append(self._rows2(k, s, dev, Sf))
                continue
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
        cc = self._count_col
        self.value_base = np.concatenate(([0], np.cumsum(self._rows[:, cc]))).astype(np.int64)               # of the concatenated stores
        self.max_count = int(self._rows[:, cc].max()) if len(self._rows) else 0
        self.max_groups = int(self._rows[:, 6].max()) if v == 2 and len(self._rows) else 0                   # version 2: non-empty groups of a frame

    def _rows2(self, k: int, s: PackedFrames2, dev, Sf: int) -> np.ndarray:
        """The int64 [F][8] rows of a version-2 store (RVT_FRAMES_GATHER2_COLS), after the checks version 1's stores get."""
        _check_set2(s)
        kept = (s.group_mask, s.seg_offset, s.grp_offset, s.masks, s.values)
        for name, t in zip(('group_mask', 'seg_offset', 'grp_offset', 'masks', 'values'), kept):
            if t.device.type == 'cpu':
                if dev.type != 'cpu' and t.numel() and not t.is_pinned():          # (an empty array is never read)
                    raise ValueError(f'store {k}: {name} lies in pageable host memory; the device reads pinned memory only (pin_memory())')
            elif t.device != dev:
                raise ValueError(f'store {k}: {name} is on {t.device}, the gather runs on {dev}')
        vb, mb = s.value_base.cpu().numpy(), s.mask_base.cpu().numpy()
        if int(vb[-1]) > s.values.numel() or int(mb[-1]) > s.masks.numel():
            raise ValueError(f'store {k}: values hold {s.values.numel()} bytes of {int(vb[-1])}, masks {s.masks.numel()} words of '
                             f'{int(mb[-1])}: the pack ran out of capacity')
        F = s.num_frames
        f = np.arange(F, dtype=np.int64)
        r = np.zeros((F, GATHER2_COLS), dtype=np.int64)
        r[:, 0] = s.group_mask.data_ptr() + 8 * Sf * f
        r[:, 1] = s.seg_offset.data_ptr() + 4 * (Sf + 1) * f
        r[:, 2] = s.grp_offset.data_ptr() + 4 * (Sf + 1) * f
        r[:, 3] = s.masks.data_ptr() + 8 * mb[:-1]
        r[:, 4] = s.values.data_ptr() + vb[:-1]
        r[:, 5] = np.diff(vb)
        r[:, 6] = np.diff(mb)
        self._keep.append(kept)
        return r

    @property
    def num_frames(self) -> int:
        return int(self.base[-1])

    def table(self, global_index, out: Optional[np.ndarray] = None) -> np.ndarray:
        """int64 [n][4] rows ([n][8] for version-2 stores) of the frames `global_index` names, in its (flattened) order; into
        out[:n] when given."""
        idx = np.asarray(global_index, dtype=np.int64).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.num_frames):
            raise IndexError(f'frame index outside [0, {self.num_frames})')
        if out is None:
            return self._rows[idx]
        return np.take(self._rows, idx, axis=0, out=out[:idx.size])

    def _check_out(self, out, n: int) -> None:
        if isinstance(out, PackedFrames2) != (self.version == 2):
            raise ValueError(f'out is not a packed set of format version {self.version}, which the stores are')
        if tuple(out.frame_shape) != self.frame_shape or out.dtype != self.dtype:
            raise ValueError(f'out holds {out.dtype} frames {tuple(out.frame_shape)}, the stores {self.dtype} frames {self.frame_shape}')
        (_check_set2 if self.version == 2 else _check_set)(out)
        if out.device != self.device:
            raise ValueError(f'out is on {out.device}, the gather runs on {self.device}')
        if out.num_frames < n:
            raise ValueError(f'out has rows for {out.num_frames} frames, {n} are asked for')

    def launch(self, table_dev: Tensor, n: int, out, max_blocks: int = 0):
        """The launch alone, on the current stream: table_dev holds the n rows already (or will, by a copy enqueued before on the
        same stream).  Writes rows [0, n) of out.masks / seg_offset, out.value_base[0 .. n], the value bytes and out.status
        (version-2 stores: rows [0, n) of group_mask / seg_offset / grp_offset, both bases, the mask words and the value bytes)."""
        self._check_out(out, n)
        if table_dev.dtype != torch.int64 or table_dev.device != self.device or not table_dev.is_contiguous() or table_dev.numel() < self.cols * n:
            raise ValueError(f'table_dev must be a contiguous int64 tensor of at least {self.cols * n} entries on {self.device}')
        cap = out.values.numel()
        if self.version == 2:
            mcap = out.masks.numel()
            L.call('rvt_frames_gather2', L.ptr(table_dev), n, self.frame_bytes, L.ptr(out.group_mask), L.ptr(out.seg_offset),
                   L.ptr(out.grp_offset), L.ptr(out.value_base), L.ptr(out.mask_base), L.ptr(out.masks) if mcap else None, mcap,
                   L.ptr(out.values) if cap else None, cap, L.ptr(out.status), int(max_blocks), L.stream_of(out.group_mask))
            return out
        L.call('rvt_frames_gather', L.ptr(table_dev), n, self.frame_bytes, L.ptr(out.masks), L.ptr(out.seg_offset), L.ptr(out.value_base),
               L.ptr(out.values) if cap else None, cap, L.ptr(out.status), int(max_blocks), L.stream_of(out.masks))
        return out

    def gather(self, global_index, out, table_dev: Optional[Tensor] = None, max_blocks: int = 0, rows: Optional[np.ndarray] = None):
        """Frames `global_index` (any shape, flattened) into rows [0, n) of `out`, on the current stream; returns out.  rows: the
        int64 [n][4] table itself instead of an index (global_index None).  table_dev: a device int64 buffer the rows are copied to
        (none given: one is allocated).  Does not synchronise: out.check() says whether out.values had room."""
        if rows is None:
            rows = self.table(global_index)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.ndim != 2 or rows.shape[1] != self.cols:
                raise ValueError(f'rows must be int64 [n][{self.cols}], got {rows.shape}')
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

    def empty(self, n: int, capacity: int, mask_capacity: Optional[int] = None):
        """An uninitialised packed set on the device with rows for n frames and room for `capacity` value bytes (version-2 stores:
        a PackedFrames2 with room for `mask_capacity` mask words, None = the worst case n * Gf)."""
        if self.version == 2:
            mcap = n * geometry(self.frame_bytes)[0] if mask_capacity is None else mask_capacity
            out = PackedFrames2.empty(self.frame_shape, self.dtype, n, capacity, mcap, self.device)
        else:
            out = PackedFrames.empty(self.frame_shape, self.dtype, n, capacity, self.device)
        out.status.zero_()
        return out


def gather_frames(stores, global_index, out=None):
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
        out = (g.empty(rows.shape[0], int(rows[:, 5].sum()), int(rows[:, 6].sum())) if g.version == 2
               else g.empty(rows.shape[0], int(rows[:, 3].sum())))
    return g.gather(None, out, rows=rows)
