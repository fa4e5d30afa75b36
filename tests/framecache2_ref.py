"""Numpy restatement of the sparse frame-cache format, version 2, written from its format section in include/rvt_hip.h (not from
the kernels, and sharing nothing with rvt_amd/framecache.py).  Version 2 is built from version 1's arrays (tests/framecache_ref.py)
by the format's own rule, and decoded by looking every group's mask up through that rule.

Geometry as in version 1: a frame is E bytes; a group is 64 consecutive bytes, Gf = ceil(E / 64); a segment is 64 consecutive
groups, Sf = ceil(Gf / 64).
  group_mask uint64 [F][Sf]      bit g of segment s set iff group 64 s + g exists and holds a non-zero byte
  seg_offset uint32 [F][Sf + 1]  as in version 1
  grp_offset uint32 [F][Sf + 1]  exclusive prefix sum of popcount(group_mask[f][s]); the last entry is the frame's count of non-empty groups
  value_base int64  [F + 1]      as in version 1
  mask_base  int64  [F + 1]      exclusive prefix sum of the frames' non-empty group counts
  masks      uint64 [ngroups]    version 1's mask of each non-empty group, frame order then group order
  values     uint8  [nnz]        as in version 1
The mask of group g (segment s, bit j) is masks[mask_base[f] + grp_offset[f][s] + popcount(group_mask[f][s] & ((1 << j) - 1))] when
bit j of group_mask[f][s] is set, else 0.
"""
import numpy as np

from tests import framecache_ref as ref1

KEYS = ('group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base', 'masks', 'values')
geometry = ref1.geometry


def nbytes(F, E, ngroups, nnz):
    Sf = geometry(E)[1]
    return 16 * Sf * F + 8 * F + 16 * (F + 1) + 8 * ngroups + nnz


def from_v1(enc1, E):
    """Version 1's arrays (framecache_ref.encode) -> version 2's: one Python integer per segment, built bit by bit."""
    m1 = enc1['masks']
    F, Gf = m1.shape
    Sf = geometry(E)[1]
    group_mask = np.zeros((F, Sf), dtype=np.uint64)
    grp_offset = np.zeros((F, Sf + 1), dtype=np.uint32)
    mask_base = np.zeros(F + 1, dtype=np.int64)
    kept = []
    for f in range(F):
        row = m1[f].tolist()
        count = 0
        for s in range(Sf):
            word = 0
            for j, m in enumerate(row[64 * s:64 * s + 64]):
                if m:
                    word |= 1 << j
                    kept.append(m)
                    count += 1
            group_mask[f, s] = word
            grp_offset[f, s + 1] = count
        mask_base[f + 1] = mask_base[f] + count
    return dict(group_mask=group_mask, seg_offset=enc1['seg_offset'], grp_offset=grp_offset, value_base=enc1['value_base'],
                mask_base=mask_base, masks=np.array(kept, dtype=np.uint64), values=enc1['values'])


def encode(frames):
    """frames uint8 [F][E] -> the seven arrays of version 2."""
    frames = np.ascontiguousarray(frames)
    return from_v1(ref1.encode(frames), frames.shape[1])


def masks_v1(enc, E):
    """uint64 [F][Gf]: the mask of every group, looked up through the format's rule."""
    gm, go, mb, masks = enc['group_mask'], enc['grp_offset'], enc['mask_base'], enc['masks'].tolist()
    F, Sf = gm.shape
    Gf = geometry(E)[0]
    out = np.zeros((F, Sf * 64), dtype=np.uint64)
    for f in range(F):
        for s in range(Sf):
            word = int(gm[f, s])
            for j in range(64):
                if (word >> j) & 1:
                    out[f, 64 * s + j] = masks[int(mb[f]) + int(go[f, s]) + bin(word & ((1 << j) - 1)).count('1')]
    assert not out[:, Gf:].any()
    return np.ascontiguousarray(out[:, :Gf])


def decode(enc, E, index=None):
    """The frames named by index (None: all in order; -1: a zero frame) as uint8 [Fout][E]."""
    v1 = dict(masks=masks_v1(enc, E), seg_offset=enc['seg_offset'], value_base=enc['value_base'], values=enc['values'])
    return ref1.decode(v1, E, index)
