"""Sparse frame cache (rvt_amd/framecache.py, rvt_amd/csrc/framecache.hpp) against the numpy restatement of its format
(tests/framecache_ref.py).  Every comparison is bit for bit.  The frame sizes are the smallest at which an edge can go wrong: less
than a group (30), one group (64), a group and a byte (65), a byte short of a segment (4095), one segment (4096), a segment and a
byte (4097), two segments and a bit (8257, odd, so that frames start at every alignment within a 16-byte line), and the smallest
shape the event builders emit (20 x 12 x 16)."""
import functools
import os

import numpy as np
import pytest
import torch

import opmodel
from rvt_amd import _header, framecache as fc
from rvt_amd.framecache import PackedFrames, pack_frames, unpack_frames
from tests import framecache_ref as ref
from tests.backends import backend  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SHAPES = {30: (2, 3, 5), 64: (1, 1, 64), 65: (1, 5, 13), 4095: (1, 63, 65), 4096: (1, 64, 64), 4097: (1, 17, 241), 8257: (1, 23, 359),
          3840: (20, 12, 16)}
FILLS = {'empty': 0.0, 'sparse': 0.01, 'half': 0.5, 'full': 1.0}
FIXTURES = ('evseq_gen1_like', 'evseq_ds2_small', 'evseq_md_gen1_like')


@functools.lru_cache(maxsize=None)
def _case(E, F, fill):
    """(frames uint8 [F][E], their reference encoding); computed once per case, never written to."""
    rng = np.random.default_rng(1000 * E + 10 * F + int(100 * FILLS[fill]) % 7)
    x = rng.integers(1, 256, size=(F, E), dtype=np.uint8)
    if FILLS[fill] < 1.0:
        x *= rng.random((F, E)) < FILLS[fill]
    if fill == 'sparse':
        x[0, 0] = 255                                  # never an accidentally empty case
    x.setflags(write=False)
    return x, ref.encode(x)


def _arrays(p: PackedFrames):
    """The packed arrays as the format's numpy types, values trimmed to nnz."""
    p.check()
    n = p.nnz()
    return dict(masks=p.masks.cpu().numpy().view(np.uint64), seg_offset=p.seg_offset.cpu().numpy().view(np.uint32),
                value_base=p.value_base.cpu().numpy(), values=p.values[:n].cpu().numpy())


def _assert_same(got, want):
    for k in ('masks', 'seg_offset', 'value_base', 'values'):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), k


def _packed_from(enc, frame_shape, dtype, dev, capacity=None):
    values = torch.from_numpy(enc['values'].copy())
    return PackedFrames(tuple(frame_shape), dtype, torch.from_numpy(enc['masks'].view(np.int64).copy()).to(dev),
                        torch.from_numpy(enc['seg_offset'].view(np.int32).copy()).to(dev), torch.from_numpy(enc['value_base'].copy()).to(dev),
                        values.to(dev), torch.zeros(1, dtype=torch.int32, device=dev))


# ---- 1. pack == restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('F', [1, 5])
@pytest.mark.parametrize('E', list(SHAPES))
def test_pack_equals_restatement(backend, E, F, fill):
    x, want = _case(E, F, fill)
    p = pack_frames(torch.from_numpy(x.copy()).reshape((F,) + SHAPES[E]).to(backend))
    assert p.frame_shape == SHAPES[E] and p.dtype == torch.uint8 and p.num_frames == F
    _assert_same(_arrays(p), want)
    nnz = int(np.count_nonzero(x))
    Gf, Sf = -(-E // 64), -(-(-(-E // 64)) // 64)
    assert p.nnz() == nnz and p.nbytes == 8 * Gf * F + 4 * (Sf + 1) * F + 8 * (F + 1) + nnz == ref.nbytes(F, E, nnz)
    assert p.trim().values.numel() == nnz


def _edge_frames(E, dtype):
    """dense, all-zero, dense, only the first byte, only the last byte, all 255 (uint8) / negative values (int8)."""
    rng = np.random.default_rng(E)
    x = np.zeros((6, E), dtype=np.uint8)
    x[0] = rng.integers(1, 256, size=E)
    x[2] = rng.integers(1, 256, size=E)
    x[3, 0] = 7
    x[4, E - 1] = 9
    x[5] = 255 if dtype == np.uint8 else rng.integers(128, 256, size=E)      # int8: -128 .. -1
    return x


@pytest.mark.parametrize('dtype', [np.uint8, np.int8], ids=['uint8', 'int8'])
@pytest.mark.parametrize('E', [30, 65, 4097, 8257])
def test_pack_edge_frames(backend, E, dtype):
    x = _edge_frames(E, dtype)
    t = torch.from_numpy(x.view(dtype).copy()).reshape((6,) + SHAPES[E]).to(backend)
    if dtype == np.int8:
        assert int(t[5].max()) < 0
    p = pack_frames(t)
    assert p.dtype == t.dtype
    _assert_same(_arrays(p), ref.encode(x))
    y = unpack_frames(p)
    assert y.dtype == t.dtype and torch.equal(y, t)


# ---- 2. unpack of restatement-encoded data == the source -----------------------------------------------------------------------------
@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('E', list(SHAPES))
def test_unpack_of_restatement(backend, E, fill):
    F = 5
    x, enc = _case(E, F, fill)
    p = _packed_from(enc, SHAPES[E], torch.uint8, backend)
    y = unpack_frames(p)
    assert tuple(y.shape) == (F,) + SHAPES[E] and y.dtype == torch.uint8
    assert np.array_equal(y.cpu().numpy().reshape(F, E), x)
    p.check()


# ---- 3. round trip with indices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [30, 4095, 4097, 8257, 3840])
def test_round_trip_with_indices(backend, E):
    F = 5
    x, enc = _case(E, F, 'half')
    p = pack_frames(torch.from_numpy(x.copy()).reshape((F,) + SHAPES[E]).to(backend))
    idx = np.array([[4, 2, 0, -1], [3, 1, 1, 4], [-1, 0, 0, 2]])                  # a permutation, repeats, padded tails; laid out (T, B)
    want = ref.decode(enc, E, idx)
    n = idx.size * E
    for lead in (3, 1, 16):                                                        # out at an odd byte offset, and at a whole line
        big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=backend)       # garbage prefill: written zeros are seen
        out = big[lead:lead + n].view(idx.shape + SHAPES[E])
        got = unpack_frames(p, torch.from_numpy(idx).to(backend), out=out)
        assert got.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
        assert np.array_equal(host[lead:lead + n].reshape(idx.size, E), want)
        assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()      # nothing outside out is written
    p.check()
    flat = unpack_frames(p, torch.from_numpy(idx.reshape(-1)).to(backend), leading_shape=(2, 6))
    assert tuple(flat.shape) == (2, 6) + SHAPES[E] and np.array_equal(flat.cpu().numpy().reshape(idx.size, E), want)


# ---- 3b. more than one tile of the 256-wide scans ------------------------------------------------------------------------------------
# (F, frame shape, fill): value_base over three tiles with a ragged last one; one frame past a tile; Sf = 258 (two tiles of the
# segment scan, and the largest per-frame run at full fill); Sf = 513 (three tiles, ragged by one)
TILE_CASES = [(600, (2, 3, 5), 0.5), (257, (1, 1, 64), 1.0), (2, (1, 257, 4100), 0.05), (2, (1, 257, 4100), 1.0), (1, (1, 513, 4096), 0.5)]


@functools.lru_cache(maxsize=None)
def _tile_case(F, shape, fill):
    """(frames uint8 [F][E], their reference encoding); computed once per case, never written to."""
    E = int(np.prod(shape))
    rng = np.random.default_rng(17 * F + E)
    x = rng.integers(1, 256, size=(F, E), dtype=np.uint8)
    if fill < 1.0:
        x *= rng.random((F, E)) < fill
    x.setflags(write=False)
    return x, ref.encode(x)


@pytest.mark.parametrize('F,shape,fill', TILE_CASES, ids=[f'F{F}-{"x".join(map(str, s))}-{int(100 * fl)}' for F, s, fl in TILE_CASES])
def test_scan_tiles(backend, F, shape, fill):
    x, want = _tile_case(F, shape, fill)
    E = x.shape[1]
    assert fc.geometry(E)[1] > 256 or F > 256                                        # a second tile in one of the scans
    p = pack_frames(torch.from_numpy(x.copy()).reshape((F,) + shape).to(backend))
    _assert_same(_arrays(p), want)
    perm = np.random.default_rng(F).permutation(F)
    y = unpack_frames(p, torch.from_numpy(perm).to(backend))
    assert np.array_equal(y.cpu().numpy().reshape(F, E), x[perm])
    p.check()


# ---- 4. the reference-built fixtures; slice / concat -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_round_trip_on_fixture(backend, name):
    planes = np.load(os.path.join(GOLDEN, name + '.npz'))['planes']
    T, B = planes.shape[:2]
    t = torch.from_numpy(planes).to(backend)
    p = pack_frames(t)
    assert p.num_frames == T * B and p.frame_shape == tuple(planes.shape[2:]) and p.dtype == t.dtype
    flat = planes.reshape(T * B, -1).view(np.uint8)
    _assert_same(_arrays(p), ref.encode(flat))
    assert torch.equal(unpack_frames(p, leading_shape=(T, B)), t)
    # host side: a slice and a concatenation equal packing the sliced / concatenated tensor directly
    host = p.to('cpu').trim()
    frames = t.reshape((T * B,) + tuple(planes.shape[2:]))
    lo, hi = 1, T * B - 1
    _assert_same(_arrays(host.slice(lo, hi)), _arrays(pack_frames(frames[lo:hi].contiguous())))
    both = fc.concat([host.slice(hi, T * B), host.slice(0, lo)])
    _assert_same(_arrays(both), _arrays(pack_frames(torch.cat([frames[hi:], frames[:lo]]))))
    assert torch.equal(unpack_frames(both.to(backend)), torch.cat([frames[hi:], frames[:lo]]))


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('short', ['one_byte', 'everything'])
def test_out_of_capacity(backend, short):
    E, F = 8257, 5
    x, want = _case(E, F, 'half')
    nnz = int(np.count_nonzero(x))
    cap = nnz - 1 if short == 'one_byte' else 0
    t = torch.from_numpy(x.copy()).reshape((F,) + SHAPES[E]).to(backend)
    Gf, Sf = fc.geometry(E)
    big = torch.full((nnz + 256,), 0x5A, dtype=torch.uint8, device=backend)         # values [0, cap), then the canary
    out = PackedFrames(SHAPES[E], torch.uint8, torch.empty(F, Gf, dtype=torch.int64, device=backend),
                       torch.empty(F, Sf + 1, dtype=torch.int32, device=backend), torch.empty(F + 1, dtype=torch.int64, device=backend),
                       big[:cap], torch.zeros(1, dtype=torch.int32, device=backend))
    p = pack_frames(t, out=out)
    assert int(p.status[0]) & fc.STATUS_CAPACITY
    with pytest.raises(RuntimeError, match='capacity'):
        p.check()
    assert p.nnz() == nnz == int(p.value_base[-1])                                  # the room a retry needs
    assert np.array_equal(p.masks.cpu().numpy().view(np.uint64), want['masks'])
    assert np.array_equal(p.seg_offset.cpu().numpy().view(np.uint32), want['seg_offset'])
    assert np.array_equal(p.value_base.cpu().numpy(), want['value_base'])
    host = big.cpu().numpy()
    assert np.array_equal(host[:cap], want['values'][:cap]) and (host[cap:] == 0x5A).all()
    out.values = big[:nnz]                                                          # the retry
    p = pack_frames(t, out=out)
    _assert_same(_arrays(p), want)
    assert (big.cpu().numpy()[nnz:] == 0x5A).all()
    assert torch.equal(unpack_frames(p), t)
    small = pack_frames(t, capacity=cap)                                            # the allocating form says the same
    with pytest.raises(RuntimeError, match='capacity'):
        small.check()
    assert small.nnz() == nnz and small.values.numel() == cap


# ---- 6. index out of range -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [5, -2], ids=['F', 'minus2'])
def test_index_out_of_range(backend, bad):
    E, F = 4097, 5
    x, enc = _case(E, F, 'half')
    p = pack_frames(torch.from_numpy(x.copy()).reshape((F,) + SHAPES[E]).to(backend))
    idx = np.array([1, bad, 3])
    n = idx.size * E
    big = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=backend)
    out = big[5:5 + n].view((3,) + SHAPES[E])
    unpack_frames(p, torch.from_numpy(idx).to(backend), out=out)
    host = big.cpu().numpy()
    want = ref.decode(enc, E, np.array([1, -1, 3]))                                  # the bad index reads as a zero frame
    assert np.array_equal(host[5:5 + n].reshape(3, E), want)
    assert (host[:5] == 0xA5).all() and (host[5 + n:] == 0xA5).all()
    assert int(p.status[0]) == fc.STATUS_INDEX
    with pytest.raises(RuntimeError, match='index outside'):
        p.check()


# ---- 7. save / load ------------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip(backend, tmp_path):
    E, F = 8257, 5
    x, want = _case(E, F, 'sparse')
    t = torch.from_numpy(x.view(np.int8).copy()).reshape((F,) + SHAPES[E]).to(backend)
    path = tmp_path / 'frames.npz'
    pack_frames(t).to('cpu').save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['dtype', 'frame_shape', 'masks', 'seg_offset', 'value_base', 'values', 'version']
        assert int(z['version']) == 1 and tuple(z['frame_shape']) == SHAPES[E] and str(z['dtype']) == 'int8'
        _assert_same({k: z[k] for k in want}, want)
    q = fc.load(path)
    assert q.frame_shape == SHAPES[E] and q.dtype == torch.int8 and q.device.type == 'cpu'
    assert torch.equal(unpack_frames(q.to(backend)), t)


def _saved(tmp_path, E=4127):
    """A valid file of 3 frames whose last group is partial, as its arrays."""
    rng = np.random.default_rng(5)
    x = rng.integers(1, 256, size=(3, E), dtype=np.uint8) * (rng.random((3, E)) < 0.2)
    enc = ref.encode(x)
    arrs = dict(enc, version=np.int64(1), frame_shape=np.array([1, 1, E], dtype=np.int64), dtype=np.str_('uint8'))
    path = tmp_path / 'ok.npz'
    np.savez(path, **arrs)
    assert fc.load(path).nnz() == int(np.count_nonzero(x))
    return arrs


def _flip_mask_bit(a):
    a['masks'] = a['masks'].copy()
    a['masks'][1, 3] ^= np.uint64(1) << np.uint64(17)


def _truncate_values(a):
    a['values'] = a['values'][:-1]


def _unsort_value_base(a):
    a['value_base'] = a['value_base'].copy()
    a['value_base'][1] = a['value_base'][2] + 1


def _set_tail_bit(a):
    a['masks'] = a['masks'].copy()
    a['masks'][2, -1] |= np.uint64(1) << np.uint64(63)


@pytest.mark.parametrize('corrupt,says', [(_flip_mask_bit, 'popcount of masks disagrees with seg_offset'), (_truncate_values, 'values hold'),
                                          (_unsort_value_base, 'value_base is not monotone'), (_set_tail_bit, 'tail bits')],
                         ids=['flipped_mask_bit', 'truncated_values', 'non_monotone_value_base', 'tail_bit'])
def test_load_refuses_corrupted_files(tmp_path, corrupt, says):
    arrs = _saved(tmp_path)
    corrupt(arrs)
    path = tmp_path / 'bad.npz'
    np.savez(path, **arrs)
    with pytest.raises(ValueError, match=says):
        fc.load(path)


# ---- 8. graph capture (GPU only) -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture():
    dev = torch.device('cuda', 0)
    E, F = 8257, 5
    shape = (F,) + SHAPES[E]
    xs = [torch.from_numpy(_case(E, F, fill)[0].copy()).reshape(shape).to(dev) for fill in ('half', 'sparse', 'full')]
    x = xs[0].clone()
    packed = pack_frames(x)                                                         # eager warm-up: the workspace is allocated and cached
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
        for t in (packed.masks, packed.seg_offset, packed.value_base):
            t.fill_(-1)
        packed.values.fill_(0)
        out.fill_(0xA5)
        g_pack.replay()
        g_unpack.replay()
        torch.cuda.synchronize()
        eager = pack_frames(x)
        _assert_same(_arrays(packed), _arrays(eager))
        assert torch.equal(out, unpack_frames(eager, index))
        assert np.array_equal(out.cpu().numpy().reshape(6, E), ref.decode(ref.encode(src.cpu().numpy().reshape(F, E)), E, index.cpu().numpy()))


# ---- 9. opmodel ----------------------------------------------------------------------------------------------------------------------
def test_opmodel_prices_both_entry_points():
    F, E, Fout, nnz = 7, 8257, 12, 4321
    Gf, Sf = fc.geometry(E)
    meta = 8 * Gf * F + 4 * (Sf + 1) * F + 8 * (F + 1)
    pack = (1, F, E, 2, 3, 4, 5, F * E, 6, 7, 1024, None)
    assert _header.PROTOS['rvt_frames_pack'].argnames == ('frames', 'F', 'E', 'masks', 'seg_offset', 'value_base', 'values', 'capacity',
                                                          'status', 'ws', 'ws_bytes', 'stream')
    assert opmodel.frames_pack_bytes(F, E, nnz) == 2.0 * F * E + meta + nnz == 2.0 * F * E + ref.nbytes(F, E, nnz)
    assert opmodel.model('rvt_frames_pack', pack) == (0.0, opmodel.frames_pack_bytes(F, E, F * E))     # no nnz in the arguments: the bound
    unpack = (1, 2, 3, 4, nnz, F, E, 5, Fout, 6, 7, None)
    per_frame = 8 * Gf + 4 * (Sf + 1) + 8
    assert opmodel.frames_unpack_bytes(Fout, E, nnz) == 1.0 * Fout * E + Fout * (per_frame + 8) + nnz
    assert opmodel.model('rvt_frames_unpack', unpack) == (0.0, opmodel.frames_unpack_bytes(Fout, E, nnz))
    assert opmodel.executed('rvt_frames_unpack', unpack) == 0.0
