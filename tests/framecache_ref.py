"""Numpy restatement of the sparse frame-cache format, version 1, written from the format section of include/rvt_hip.h (not from
the kernels): an encoder and a decoder that share nothing with rvt_amd/csrc/framecache.hpp or rvt_amd/framecache.py.

A frame is E bytes; a group is 64 consecutive bytes, Gf = ceil(E / 64); a segment is 64 consecutive groups, Sf = ceil(Gf / 64).
  masks      uint64 [F][Gf]      bit i of group g set iff byte 64 g + i exists and is non-zero
  seg_offset uint32 [F][Sf + 1]  exclusive prefix sum of the per-segment non-zero counts; the last entry is the frame's count
  value_base int64  [F + 1]      exclusive prefix sum of the frames' counts
  values     uint8  [nnz]        the non-zero bytes, frame order then byte order
"""
import numpy as np


def geometry(E):
    Gf = -(-E // 64)
    return Gf, -(-Gf // 64)


def nbytes(F, E, nnz):
    Gf, Sf = geometry(E)
    return 8 * Gf * F + 4 * (Sf + 1) * F + 8 * (F + 1) + nnz


def encode(frames):
    """frames uint8 [F][E] -> dict(masks, seg_offset, value_base, values)."""
    frames = np.ascontiguousarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 2
    F, E = frames.shape
    Gf, Sf = geometry(E)
    nz = np.zeros((F, Sf * 4096), dtype=bool)
    nz[:, :E] = frames != 0
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    masks = (nz.reshape(F, Sf * 64, 64) * weights).sum(axis=2, dtype=np.uint64)[:, :Gf]
    per_seg = nz.reshape(F, Sf, 4096).sum(axis=2, dtype=np.int64)
    seg_offset = np.zeros((F, Sf + 1), dtype=np.int64)
    seg_offset[:, 1:] = np.cumsum(per_seg, axis=1)
    value_base = np.zeros(F + 1, dtype=np.int64)
    value_base[1:] = np.cumsum(seg_offset[:, -1])
    values = frames[frames != 0]                      # row-major boolean selection: frame order, then byte order
    assert values.shape[0] == value_base[-1]
    return dict(masks=np.ascontiguousarray(masks), seg_offset=seg_offset.astype(np.uint32), value_base=value_base, values=values)


def decode(enc, E, index=None):
    """The frames named by index (None: all, in order; -1: a zero frame) as uint8 [Fout][E]: every byte is looked up through
    value_base, seg_offset and its rank among the set bits of its segment, as a reader of the format would."""
    masks, seg_offset, value_base, values = enc['masks'], enc['seg_offset'].astype(np.int64), enc['value_base'], enc['values']
    F, Gf = masks.shape
    Sf = geometry(E)[1]
    index = np.arange(F) if index is None else np.asarray(index).reshape(-1)
    out = np.zeros((len(index), E), dtype=np.uint8)
    for o, f in enumerate(index):
        if f == -1:
            continue
        assert 0 <= f < F
        bits = np.zeros(Sf * 4096, dtype=bool)
        bits[:Gf * 64] = ((masks[f][:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1)
        assert not bits[E:].any()
        seg = bits.reshape(Sf, 4096)
        rank = np.cumsum(seg, axis=1) - 1                                       # rank of a set bit within its segment
        addr = value_base[f] + seg_offset[f][:Sf, None] + rank
        frame = np.zeros(Sf * 4096, dtype=np.uint8)
        frame[bits] = values[addr[seg]]
        out[o] = frame[:E]
    return out
