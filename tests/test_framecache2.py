"""Sparse frame cache, format version 2 (rvt_amd/framecache.py PackedFrames2, rvt_amd/csrc/capi_frames2.hip) against the numpy
restatement of the format (tests/framecache2_ref.py, built on tests/framecache_ref.py).  Every comparison is bit for bit: the format
is a lossless codec, so there is no tolerance anywhere.

Frame sizes: those of tests/test_framecache.py (the smallest at which an edge of a group, a segment or a 16-byte line can go wrong)
plus one byte, 20 x 24 x 32 (frames on 16-byte boundaries, four segments) and 3 x 37 x 53 (odd: frames start at every alignment).
F = 5, so that F * Sf is no multiple of the four waves of a workgroup wherever Sf admits it (Sf = 4 at 20 x 24 x 32 never does).
Fills: the mask level has its own edges, so beside uniform fills there are whole empty groups ("blobs"), one live group per
segment, only the frame's last byte, and the two bytes either side of the first group boundary of every segment."""
import functools
import os

import numpy as np
import pytest
import torch

import opmodel
from rvt_amd import _header, _lib, framecache as fc
from rvt_amd.framecache import PackedFrames, PackedFrames2, pack_frames, unpack_frames
from tests import framecache2_ref as ref
from tests import framecache_ref as ref1
from tests.backends import backend  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHAPES = {1: (1, 1, 1), 30: (2, 3, 5), 64: (1, 1, 64), 65: (1, 5, 13), 4095: (1, 63, 65), 4096: (1, 64, 64), 4097: (1, 17, 241),
          8257: (1, 23, 359), 3840: (20, 12, 16), 15360: (20, 24, 32), 5883: (3, 37, 53)}
FILLS = ('zero', 'full', 'u1', 'u30', 'blobs', 'byte_per_segment', 'last_byte', 'b63_64')
FIXTURES = ('evseq_gen1_like', 'evseq_ds2_small', 'evseq_md_gen1_like')
DTYPES = {'uint8': (np.uint8, torch.uint8), 'int8': (np.int8, torch.int8)}
F5 = 5
CANARY = 0x5A
CANARY64 = int.from_bytes(bytes([CANARY] * 8), 'little', signed=True)


def make_frames(F, E, fill, seed=0):
    """uint8 [F][E] of one of FILLS."""
    rng = np.random.default_rng(1000 * E + 10 * F + FILLS.index(fill) + seed)
    x = rng.integers(1, 256, size=(F, E), dtype=np.uint8)
    nseg = -(-E // 4096)
    if fill == 'zero':
        x[:] = 0
    elif fill == 'u1':
        x *= rng.random((F, E)) < 0.01
        x[0, 0] = 255                                  # never an accidentally empty case
    elif fill == 'u30':
        x *= rng.random((F, E)) < 0.30
    elif fill == 'blobs':                              # a group is live with probability 0.2, a byte of a live group non-zero with 0.15
        live = np.repeat(rng.random((F, -(-E // 64))) < 0.2, 64, axis=1)[:, :E]
        x *= live & (rng.random((F, E)) < 0.15)
    elif fill == 'byte_per_segment':
        keep = np.zeros((F, E), dtype=bool)
        for f in range(F):
            for s in range(nseg):
                keep[f, rng.integers(4096 * s, min(4096 * (s + 1), E))] = True
        x *= keep
    elif fill == 'last_byte':
        keep = np.zeros((F, E), dtype=bool)
        keep[:, E - 1] = True
        x *= keep
    elif fill == 'b63_64':
        keep = np.zeros((F, E), dtype=bool)
        for s in range(nseg):
            keep[:, [b for b in (4096 * s + 63, 4096 * s + 64) if b < E]] = True
        x *= keep
    else:
        assert fill == 'full'
    return x


@functools.lru_cache(maxsize=None)
def _case(E, F, fill):
    """(frames uint8 [F][E], their version-2 reference encoding); computed once per case, never written to."""
    x = make_frames(F, E, fill)
    x.setflags(write=False)
    return x, ref.encode(x)


def arrays_of(p: PackedFrames2, check=True):
    """The packed arrays as the format's numpy types, masks and values trimmed to what is in use."""
    if check:
        p.check()
    u = {'group_mask': np.uint64, 'seg_offset': np.uint32, 'grp_offset': np.uint32, 'masks': np.uint64}
    out = {k: getattr(p, k).cpu().numpy() for k in ref.KEYS}
    out = {k: (v.view(u[k]) if k in u else v) for k, v in out.items()}
    out['masks'], out['values'] = out['masks'][:p.ngroups()], out['values'][:p.nnz()]
    return out


def assert_same(got, want, keys=ref.KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        assert np.array_equal(got[k], want[k]), k


def packed_from(enc, frame_shape, dtype, dev):
    s = {'group_mask': np.int64, 'seg_offset': np.int32, 'grp_offset': np.int32, 'masks': np.int64}
    t = [torch.from_numpy((enc[k].view(s[k]) if k in s else enc[k]).copy()).to(dev) for k in ref.KEYS]
    return PackedFrames2(tuple(frame_shape), dtype, *t, torch.zeros(1, dtype=torch.int32, device=dev))


# ---- 0. the restatement itself: its rule decodes what version 1's restatement encodes -------------------------------------------------
@pytest.mark.parametrize('fill', FILLS)
def test_restatement_round_trip(fill):
    E = 8257
    x, enc = _case(E, F5, fill)
    assert np.array_equal(ref.decode(enc, E), x)
    Gf, Sf = ref.geometry(E)
    groups = int((np.pad(x, ((0, 0), (0, Gf * 64 - E))).reshape(F5, Gf, 64) != 0).any(axis=2).sum())
    assert enc['masks'].shape == (groups,) and int(enc['mask_base'][-1]) == groups and not (enc['masks'] == 0).any()
    if fill == 'full':
        assert groups == F5 * Gf
    if fill == 'zero':
        assert groups == 0


# ---- 1. pack == restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('E', list(SHAPES))
def test_pack_equals_restatement(backend, E, fill, dtype):
    x, want = _case(E, F5, fill)
    t = torch.from_numpy(x.view(DTYPES[dtype][0]).copy()).reshape((F5,) + SHAPES[E]).to(backend)
    p = pack_frames(t, version=2)
    assert isinstance(p, PackedFrames2) and p.frame_shape == SHAPES[E] and p.dtype == DTYPES[dtype][1] and p.num_frames == F5
    assert int(p.status[0]) == 0
    assert_same(arrays_of(p), want)
    nnz, ng = int(np.count_nonzero(x)), int(want['mask_base'][-1])
    Sf = ref.geometry(E)[1]
    assert p.nnz() == nnz and p.ngroups() == ng
    assert p.nbytes == fc.packed_nbytes2(F5, E, ng, nnz) == 16 * Sf * F5 + 8 * F5 + 16 * (F5 + 1) + 8 * ng + nnz == ref.nbytes(F5, E, ng, nnz)
    q = p.trim()
    assert q.values.numel() == nnz and q.masks.numel() == ng
    y = unpack_frames(p)
    assert y.dtype == t.dtype and torch.equal(y, t)


# ---- 2. unpack of the restatement's arrays ------------------------------------------------------------------------------------------------
INDEX = np.array([[4, 2, 0, -1], [3, 1, 1, 4], [-1, 0, 0, 2]])        # a permutation, repeats, padded tails, Fout = 12 != F; laid out (T, B)


@pytest.mark.parametrize('fill', FILLS)
@pytest.mark.parametrize('E', list(SHAPES))
def test_unpack_of_restatement(backend, E, fill):
    x, enc = _case(E, F5, fill)
    p = packed_from(enc, SHAPES[E], torch.uint8, backend)
    want = ref.decode(enc, E, INDEX)
    assert np.array_equal(want, np.where(INDEX.reshape(-1, 1) >= 0, x[INDEX.reshape(-1)], 0))
    n = INDEX.size * E
    for lead in (3, 16):                                                           # out at an odd byte offset, and at a whole line
        big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=backend)       # garbage prefill: written zeros are seen
        out = big[lead:lead + n].view(INDEX.shape + SHAPES[E])
        got = unpack_frames(p, torch.from_numpy(INDEX).to(backend), out=out)
        assert got.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
        assert np.array_equal(host[lead:lead + n].reshape(INDEX.size, E), want)
        assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()      # nothing outside out is written
    p.check()
    y = unpack_frames(p)                                                             # no index: every frame in order
    assert tuple(y.shape) == (F5,) + SHAPES[E] and np.array_equal(y.cpu().numpy().reshape(F5, E), x)


@pytest.mark.parametrize('bad', [5, -2], ids=['F', 'minus2'])
def test_index_out_of_range(backend, bad):
    E = 4097
    x, enc = _case(E, F5, 'u30')
    p = packed_from(enc, SHAPES[E], torch.uint8, backend)
    idx = np.array([1, bad, 3])
    n = idx.size * E
    big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=backend)
    out = big[5:5 + n].view((3,) + SHAPES[E])
    unpack_frames(p, torch.from_numpy(idx).to(backend), out=out)
    host = big.cpu().numpy()
    assert np.array_equal(host[5:5 + n].reshape(3, E), ref.decode(enc, E, np.array([1, -1, 3])))     # the bad index reads as a zero frame
    assert (host[:5] == 0xA5).all() and (host[5 + n:] == 0xA5).all()
    assert int(p.status[0]) == fc.STATUS_INDEX
    with pytest.raises(RuntimeError, match='index outside'):
        p.check()


def test_reads_stay_inside_short_arrays(backend):
    """masks and values shorter than the index arrays say: the reads are clamped to masks_len / values_len (missing masks read as
    empty groups), and nothing outside out is written."""
    E = 8257
    x, enc = _case(E, F5, 'u30')
    short = dict(enc, masks=enc['masks'][:len(enc['masks']) // 2], values=enc['values'][:len(enc['values']) // 3])
    p = packed_from(short, SHAPES[E], torch.uint8, backend)
    n = F5 * E
    big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=backend)
    unpack_frames(p, out=big[7:7 + n].view((F5,) + SHAPES[E]))
    host = big.cpu().numpy()
    assert (host[:7] == 0xA5).all() and (host[7 + n:] == 0xA5).all()
    first = int(np.searchsorted(enc['mask_base'], len(short['masks']), side='right')) - 1    # frames wholly inside both short arrays
    first = min(first, int(np.searchsorted(enc['value_base'], len(short['values']), side='right')) - 1)
    assert first >= 1 and np.array_equal(host[7:7 + first * E].reshape(first, E), x[:first])


# ---- 3. more than one tile of the 256-wide scans ----------------------------------------------------------------------------------------
# one frame with Sf = 258 (two tiles of the per-frame scans), sparse and full; F = 300 frames of 65 bytes (two tiles of the frame scans)
TILE_CASES = [(1, (1, 257, 4100), 'u1'), (1, (1, 257, 4100), 'full'), (300, (1, 5, 13), 'u30')]


@pytest.mark.parametrize('F,shape,fill', TILE_CASES, ids=[f'F{F}-{"x".join(map(str, s))}-{fl}' for F, s, fl in TILE_CASES])
def test_scan_tiles(backend, F, shape, fill):
    E = int(np.prod(shape))
    x = make_frames(F, E, fill, seed=17)
    assert fc.geometry(E)[1] > 256 or F > 256
    t = torch.from_numpy(x).reshape((F,) + shape).to(backend)
    p = pack_frames(t, version=2)
    assert_same(arrays_of(p), ref.encode(x))
    perm = np.random.default_rng(F).permutation(F)
    y = unpack_frames(p, torch.from_numpy(perm).to(backend))
    assert np.array_equal(y.cpu().numpy().reshape(F, E), x[perm])
    p.check()


# ---- 4. out of capacity: each side alone and both ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('short', ['values_one_byte', 'masks_one_word', 'both_zero'])
def test_out_of_capacity(backend, short):
    E = 8257
    x, want = _case(E, F5, 'u30')
    nnz, ng = len(want['values']), len(want['masks'])
    cap = {'values_one_byte': nnz - 1, 'masks_one_word': nnz, 'both_zero': 0}[short]
    mcap = {'values_one_byte': ng, 'masks_one_word': ng - 1, 'both_zero': 0}[short]
    t = torch.from_numpy(x.copy()).reshape((F5,) + SHAPES[E]).to(backend)
    Sf = fc.geometry(E)[1]
    bigv = torch.full((nnz + 256,), CANARY, dtype=torch.uint8, device=backend)      # the arrays [0, cap), then the canary
    bigm = torch.full((ng + 32,), CANARY64, dtype=torch.int64, device=backend)
    out = PackedFrames2.empty(SHAPES[E], torch.uint8, F5, 0, 0, backend)
    out.values, out.masks = bigv[:cap], bigm[:mcap]
    p = pack_frames(t, out=out)
    assert p is out and int(p.status[0]) == fc.STATUS_CAPACITY
    with pytest.raises(RuntimeError, match='capacity'):
        p.check()
    assert p.nnz() == nnz and p.ngroups() == ng                                     # the room a retry needs
    got = arrays_of(p, check=False)
    assert_same(got, want, keys=('group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base'))
    hv, hm = bigv.cpu().numpy(), bigm.cpu().numpy()
    assert np.array_equal(hv[:cap], want['values'][:cap]) and (hv[cap:] == CANARY).all()
    assert np.array_equal(hm[:mcap].view(np.uint64), want['masks'][:mcap]) and (hm[mcap:] == CANARY64).all()
    out.values, out.masks = bigv[:nnz], bigm[:ng]                                   # the retry
    p = pack_frames(t, out=out)
    assert_same(arrays_of(p), want)
    assert (bigv.cpu().numpy()[nnz:] == CANARY).all() and (bigm.cpu().numpy()[ng:] == CANARY64).all()
    assert torch.equal(unpack_frames(p), t)
    small = pack_frames(t, capacity=cap, mask_capacity=mcap, version=2)             # the allocating form says the same
    with pytest.raises(RuntimeError, match='capacity'):
        small.check()
    assert small.nnz() == nnz and small.ngroups() == ng and small.values.numel() == cap and small.masks.numel() == mcap


# ---- 5. the reference-built fixtures; convert; slice / concat -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_round_trip_on_fixture(backend, name):
    planes = np.load(os.path.join(GOLDEN, name + '.npz'))['planes']
    T, B = planes.shape[:2]
    t = torch.from_numpy(planes).to(backend)
    p2 = pack_frames(t, version=2)
    assert p2.num_frames == T * B and p2.frame_shape == tuple(planes.shape[2:]) and p2.dtype == t.dtype
    flat = planes.reshape(T * B, -1).view(np.uint8)
    assert_same(arrays_of(p2), ref.encode(flat))
    assert torch.equal(unpack_frames(p2, leading_shape=(T, B)), t)
    # convert: 1 -> 2 equals the version-2 pack, and 1 -> 2 -> 1 returns identical arrays
    h1, h2 = pack_frames(t).to('cpu').trim(), p2.to('cpu').trim()
    c2 = fc.convert(h1, 2)
    assert isinstance(c2, PackedFrames2)
    assert_same(arrays_of(c2), arrays_of(h2))
    c1 = fc.convert(c2, 1)
    assert isinstance(c1, PackedFrames)
    for k in ('masks', 'seg_offset', 'value_base', 'values'):
        assert torch.equal(getattr(c1, k), getattr(h1, k)), k
    assert fc.convert(h1, 1) is h1 and fc.convert(h2, 2) is h2
    assert h2.nbytes == fc.packed_nbytes2(T * B, flat.shape[1], h2.ngroups(), h2.nnz()) and h1.nnz() == h2.nnz()
    # host side: a slice and a concatenation equal packing the sliced / concatenated tensor directly
    frames = t.reshape((T * B,) + tuple(planes.shape[2:]))
    lo, hi = 1, T * B - 1
    assert_same(arrays_of(h2.slice(lo, hi)), arrays_of(pack_frames(frames[lo:hi].contiguous(), version=2)))
    both = fc.concat([h2.slice(hi, T * B), h2.slice(0, lo)])
    assert_same(arrays_of(both), arrays_of(pack_frames(torch.cat([frames[hi:], frames[:lo]]), version=2)))
    assert torch.equal(unpack_frames(both.to(backend)), torch.cat([frames[hi:], frames[:lo]]))
    with pytest.raises(ValueError, match='versions 1 and 2'):
        fc.concat([h2, h1])
    with pytest.raises(ValueError, match='versions 1 and 2'):
        fc.concat([h1, h2])


def test_unpack_augment_names_the_fused_route(backend):
    x, enc = _case(3840, F5, 'u30')
    p = packed_from(enc, SHAPES[3840], torch.uint8, backend)
    with pytest.raises(NotImplementedError, match='rvt_frames_unpack_augment'):
        fc.unpack_augment(p, torch.zeros(1, 1, dtype=torch.int64, device=backend), torch.zeros(1, 8, dtype=torch.int32, device=backend))


# ---- 6. save / load -----------------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip(backend, tmp_path):
    E = 8257
    x, want = _case(E, F5, 'blobs')
    t = torch.from_numpy(x.view(np.int8).copy()).reshape((F5,) + SHAPES[E]).to(backend)
    path = tmp_path / 'frames2.npz'
    pack_frames(t, version=2).to('cpu').save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(ref.KEYS + ('version', 'value_bits', 'frame_shape', 'dtype'))
        assert int(z['version']) == 2 and int(z['value_bits']) == 8 and tuple(z['frame_shape']) == SHAPES[E] and str(z['dtype']) == 'int8'
        assert_same({k: z[k] for k in ref.KEYS}, want)
    q = fc.load(path)
    assert isinstance(q, PackedFrames2) and q.frame_shape == SHAPES[E] and q.dtype == torch.int8 and q.device.type == 'cpu'
    assert torch.equal(unpack_frames(q.to(backend)), t)
    # a version-1 file still loads as PackedFrames
    path1 = tmp_path / 'frames1.npz'
    pack_frames(t).to('cpu').save(path1)
    q1 = fc.load(path1)
    assert isinstance(q1, PackedFrames) and torch.equal(unpack_frames(q1.to(backend)), t)


def _saved(tmp_path, E=4127):
    """A valid version-2 file of 3 frames whose last group is partial and stored, as its arrays."""
    rng = np.random.default_rng(5)
    x = rng.integers(1, 256, size=(3, E), dtype=np.uint8) * (rng.random((3, E)) < 0.2)
    x[:, E - 1] = 3
    arrs = dict(ref.encode(x), version=np.int64(2), value_bits=np.int64(8), frame_shape=np.array([1, 1, E], dtype=np.int64),
                dtype=np.str_('uint8'))
    path = tmp_path / 'ok.npz'
    np.savez(path, **arrs)
    q = fc.load(path)
    assert q.nnz() == int(np.count_nonzero(x)) and q.ngroups() == len(arrs['masks'])
    return arrs


def _flip_group_mask_bit(a):
    a['group_mask'] = a['group_mask'].copy()
    a['group_mask'][1, 0] ^= np.uint64(1) << np.uint64(17)


def _zero_mask_word(a):
    a['masks'] = a['masks'].copy()
    a['masks'][5] = 0


def _truncate_masks(a):
    a['masks'] = a['masks'][:-1]


def _wrong_grp_offset(a):
    a['grp_offset'] = a['grp_offset'].copy()
    a['grp_offset'][2, 1] += 1


def _set_tail_bit(a):
    a['masks'] = a['masks'].copy()
    a['masks'][-1] |= np.uint64(1) << np.uint64(63)


def _four_bit_values(a):
    a['value_bits'] = np.int64(4)


@pytest.mark.parametrize('corrupt,says', [(_flip_group_mask_bit, 'popcount of group_mask disagrees with grp_offset'),
                                          (_zero_mask_word, 'masks hold a zero word'), (_truncate_masks, r'masks hold \d+ words'),
                                          (_wrong_grp_offset, 'disagrees with grp_offset'), (_set_tail_bit, 'tail bits set in masks'),
                                          (_four_bit_values, 'value_bits = 4')],
                         ids=['flipped_group_mask_bit', 'zero_mask_word', 'truncated_masks', 'wrong_grp_offset', 'tail_bit', 'value_bits_4'])
def test_load_refuses_corrupted_files(tmp_path, corrupt, says):
    arrs = _saved(tmp_path)
    corrupt(arrs)
    path = tmp_path / 'bad.npz'
    np.savez(path, **arrs)
    with pytest.raises(ValueError, match=says):
        fc.load(path)


# ---- 9. graph capture (GPU only) ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture():
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    E = 8257
    shape = (F5,) + SHAPES[E]
    xs = [torch.from_numpy(_case(E, F5, fill)[0].copy()).reshape(shape).to(dev) for fill in ('u30', 'blobs', 'full')]
    x = xs[0].clone()
    packed = pack_frames(x, version=2)                                              # eager warm-up: the workspace is allocated and cached
    index = torch.tensor([[4, 0, -1], [2, 2, 1]], device=dev)
    out = torch.empty(tuple(index.shape) + SHAPES[E], dtype=torch.uint8, device=dev)
    unpack_frames(packed, index, out=out)
    torch.cuda.synchronize()
    g_pack, g_unpack = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_pack):
        pack_frames(x, out=packed)
    with torch.cuda.graph(g_unpack):
        unpack_frames(packed, index, out=out)
    for k, src in enumerate(xs[1:]):
        x.copy_(src)                                                                # new frames, a new index, the same addresses
        index.copy_(torch.tensor([[k, -1, 3], [4, k, k]], device=dev))
        for t in (packed.group_mask, packed.seg_offset, packed.grp_offset, packed.value_base, packed.mask_base, packed.masks):
            t.fill_(-1)
        packed.values.fill_(0)
        out.fill_(0xA5)
        g_pack.replay()
        g_unpack.replay()
        torch.cuda.synchronize()
        eager = pack_frames(x, version=2)
        assert_same(arrays_of(packed), arrays_of(eager))
        assert torch.equal(out, unpack_frames(eager, index))
        assert np.array_equal(out.cpu().numpy().reshape(6, E), ref.decode(ref.encode(src.cpu().numpy().reshape(F5, E)), E, index.cpu().numpy()))


# ---- 10. opmodel; the header's exports are the library's ------------------------------------------------------------------------------------
def test_opmodel_prices_the_entry_points():
    F, E, Fout, nnz, ng = 7, 8257, 12, 4321, 321
    Gf, Sf = fc.geometry(E)
    assert _header.PROTOS['rvt_frames_pack2'].argnames == ('frames', 'F', 'E', 'group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base',
                                                           'masks', 'mask_capacity', 'values', 'capacity', 'status', 'ws', 'ws_bytes', 'stream')
    assert _header.PROTOS['rvt_frames_unpack2'].argnames == ('group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base', 'masks',
                                                             'masks_len', 'values', 'values_len', 'F', 'E', 'index', 'Fout', 'out', 'status', 'stream')
    assert _header.PROTOS['rvt_frames_gather2'].argnames == ('table', 'n', 'E', 'group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base',
                                                             'masks', 'mask_capacity', 'values', 'capacity', 'status', 'max_blocks', 'stream')
    assert _header.ENUMS['RVT_FRAMES_GATHER2_COLS'] == 8 == fc.GATHER2_COLS
    assert opmodel.frames_pack2_bytes(F, E, ng, nnz) == 2.0 * F * E + fc.packed_nbytes2(F, E, ng, nnz) == 2.0 * F * E + ref.nbytes(F, E, ng, nnz)
    pack = (1, F, E, 2, 3, 4, 5, 6, 7, F * Gf, 8, F * E, 9, 10, 1024, None)
    assert opmodel.model('rvt_frames_pack2', pack) == (0.0, opmodel.frames_pack2_bytes(F, E, F * Gf, F * E))    # no counts in the arguments: the bound
    per_frame = 16 * Sf + 8 + 16
    assert opmodel.frames_unpack2_bytes(Fout, E, ng, nnz) == 1.0 * Fout * E + Fout * (per_frame + 8) + 8 * ng + nnz
    unpack = (1, 2, 3, 4, 5, 6, ng, 7, nnz, F, E, 8, Fout, 9, 10, None)
    assert opmodel.model('rvt_frames_unpack2', unpack) == (0.0, opmodel.frames_unpack2_bytes(Fout, E, ng, nnz))
    assert opmodel.frames_gather2_bytes(F, E, ng, nnz) == 2.0 * fc.packed_nbytes2(F, E, ng, nnz) + 64.0 * F
    gather = (1, F, E, 2, 3, 4, 5, 6, 7, ng, 8, nnz, 9, 0, None)
    assert opmodel.model('rvt_frames_gather2', gather) == (0.0, opmodel.frames_gather2_bytes(F, E, ng, nnz))
    for name, args in (('rvt_frames_pack2', pack), ('rvt_frames_unpack2', unpack), ('rvt_frames_gather2', gather)):
        assert opmodel.executed(name, args) == 0.0


def test_header_exports_equal_the_librarys():
    """Every prototype of the header is a symbol of the emulator build of the same sources (the gfx950 build is held to the same by
    tests/test_host.py), and the library exports no rvt_ symbol the header does not declare."""
    import re
    import subprocess
    from tests.backends import EMU_SO, emu_library
    lib = emu_library()
    for name in ('rvt_frames_pack2_ws_bytes', 'rvt_frames_pack2', 'rvt_frames_unpack2', 'rvt_frames_gather2'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    Sf = fc.geometry(8257)[1]
    assert lib.rvt_frames_pack2_ws_bytes(5, 8257) == ((2 * 5 * Sf + 2 * 5) * 4 + 15) // 16 * 16 and lib.rvt_frames_pack2_ws_bytes(0, 8257) == 0
    nm = subprocess.run(['nm', '-D', '--defined-only', EMU_SO], check=True, capture_output=True, text=True).stdout
    exported = sorted(set(re.findall(r'\b[TW] (rvt_[a-z0-9_]+)$', nm, re.M)))
    assert exported == _lib.EXPORTS
