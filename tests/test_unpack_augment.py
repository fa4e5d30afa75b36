"""Packed frames to augmented planes in one launch (rvt_amd.framecache.unpack_augment, rvt_frames_unpack_augment,
rvt_amd/csrc/frames_augment.hpp).  The contract is out == augment_planes(unpack_frames(packed, index), table), bit for bit.

Truth is two restatements that are not under test: the numpy decoder of the format (tests/framecache_ref.py) followed by the
plain-torch augmentation (tests/augment_ref.py).  Every comparison is for exact equality.  The shapes are the smallest at which an
edge can go wrong: less than a segment (2 x 12 x 16), the smallest shape the builders emit (20 x 12 x 16), rows on group boundaries
(1 x 8 x 640), the Gen1 width whose rows start inside a group and straddle segments on the 16-byte path (2 x 40 x 304), and the
byte path with rows at every alignment and E no multiple of 64 (3 x 23 x 359), the largest supported W on the 16-byte path
(1 x 3 x 2048) and the widest row on the byte path (1 x 5 x 2047)."""
import functools
import os

import numpy as np
import pytest
import torch

import opmodel
from rvt_amd import _header, augment as A, framecache as fc
from rvt_amd.augment import SpatialAugmentState
from rvt_amd.framecache import PackedFrames, pack_frames, unpack_augment, unpack_frames
from tests import augment_ref, casegen_augment as cg, framecache_ref as ref
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden
from tests.test_framecache import _edge_frames

SHAPES = [(2, 12, 16), (20, 12, 16), (1, 8, 640), (2, 40, 304), (3, 23, 359), (1, 3, 2048), (1, 5, 2047)]
FILLS = {'empty': 0.0, 'sparse': 0.01, 'half': 0.5, 'full': 1.0}
F_PACKED = 4


def _sid(shape):
    return 'x'.join(str(d) for d in shape)


@functools.lru_cache(maxsize=None)
def _case(shape, fill, F=F_PACKED):
    """(frames uint8 [F][E], their reference encoding); computed once per case, never written to."""
    E = int(np.prod(shape))
    rng = np.random.default_rng(7000 + 13 * E + int(100 * FILLS[fill]))
    x = rng.integers(1, 256, size=(F, E), dtype=np.uint8)
    if FILLS[fill] < 1.0:
        x *= rng.random((F, E)) < FILLS[fill]
    if fill == 'sparse':
        x[:, 0] = 255                                  # never an accidentally empty case
    x.setflags(write=False)
    return x, ref.encode(x)


def _odd_zoom_in(H, W):
    """A zoom-in factor that makes zh and zw odd, with odd x0 / y0 that fit."""
    for f in np.arange(1.03, 1.95, 0.005):
        zh, zw = int(H / f), int(W / f)
        if zh % 2 == 1 and zw % 2 == 1 and 1 + zh <= H and 1 + zw <= W:
            return float(f), (3 if 3 + zw <= W else 1), 1
    raise AssertionError(f'no odd zoom-in window for {H}x{W}')


@functools.lru_cache(maxsize=None)
def _states(H, W):
    """Identity, flip, zoom-in with and without flip (odd x0, y0, zh, zw), zoom-out flush to each corner (two of them flipped)."""
    f, x0, y0 = _odd_zoom_in(H, W)
    fo = 1.3
    zh, zw = int(H / fo), int(W / fo)
    assert 1 <= zh < H and 1 <= zw < W
    st = [SpatialAugmentState(), SpatialAugmentState(flip=True),
          SpatialAugmentState(mode=1, factor=f, x0=x0, y0=y0), SpatialAugmentState(flip=True, mode=1, factor=f, x0=x0, y0=y0),
          SpatialAugmentState(mode=2, factor=fo, x0=0, y0=0), SpatialAugmentState(flip=True, mode=2, factor=fo, x0=W - zw, y0=0),
          SpatialAugmentState(flip=True, mode=2, factor=fo, x0=0, y0=H - zh), SpatialAugmentState(mode=2, factor=fo, x0=W - zw, y0=H - zh)]
    zi = st[2].window_hw((H, W))
    assert zi[0] % 2 == 1 and zi[1] % 2 == 1 and st[2].x0 % 2 == 1 and st[2].y0 % 2 == 1
    return tuple(st)


def _truth(x, enc, shape, index, states):
    """decode (numpy restatement) then augment (torch restatement): uint8 (T, B) + shape."""
    index = np.asarray(index)
    E = int(np.prod(shape))
    dense = ref.decode(enc, E, index).reshape(tuple(index.shape) + tuple(shape))
    return augment_ref.planes_ref(torch.from_numpy(dense), list(states)).numpy()


def _packed_from(enc, shape, dtype, dev):
    return PackedFrames(tuple(shape), dtype, torch.from_numpy(enc['masks'].view(np.int64).copy()).to(dev),
                        torch.from_numpy(enc['seg_offset'].view(np.int32).copy()).to(dev), torch.from_numpy(enc['value_base'].copy()).to(dev),
                        torch.from_numpy(enc['values'].copy()).to(dev), torch.zeros(1, dtype=torch.int32, device=dev))


def _u8(t):
    return t.cpu().numpy().view(np.uint8)


# ---- 1. every shape, fill and state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_equals_restatements(backend, shape, fill):
    dev = backend
    x, enc = _case(shape, fill)
    st = _states(*shape[1:])
    B = len(st)
    index = np.array([[(3 * b + 1) % F_PACKED for b in range(B)], [(b + 2) % F_PACKED for b in range(B)]])     # T = 2; frames repeat under several rows
    p = _packed_from(enc, shape, torch.uint8, dev)
    it, _ = A.make_tables(st, shape[1:], dev)
    got = unpack_augment(p, torch.from_numpy(index).to(dev), it)
    assert tuple(got.shape) == (2, B) + shape and got.dtype == torch.uint8
    assert np.array_equal(_u8(got), _truth(x, enc, shape, index, st))
    p.check()
    # the two-launch route on the same backend
    two = A.augment_planes(unpack_frames(p, torch.from_numpy(index).to(dev)), it)
    assert torch.equal(got, two)


@pytest.mark.parametrize('dtype', [np.uint8, np.int8], ids=['uint8', 'int8'])
@pytest.mark.parametrize('shape', [(2, 12, 16), (2, 40, 304), (3, 23, 359)], ids=_sid)
def test_edge_frames(backend, shape, dtype):
    """dense, all zero, dense, first byte only, last byte only, all 255 / int8 negatives: each under every state."""
    dev = backend
    E = int(np.prod(shape))
    x = _edge_frames(E, dtype)
    enc = ref.encode(x)
    st = _states(*shape[1:])
    B = len(st)
    t = torch.from_numpy(x.view(dtype).copy()).reshape((6,) + shape).to(dev)
    p = pack_frames(t)
    index = np.repeat(np.arange(6)[:, None], B, axis=1)
    it, _ = A.make_tables(st, shape[1:], dev)
    got = unpack_augment(p, torch.from_numpy(index).to(dev), it)
    assert got.dtype == t.dtype and tuple(got.shape) == (6, B) + shape
    assert np.array_equal(_u8(got), _truth(x, enc, shape, index, st))
    p.check()


# ---- 2. a table outside the frame is clamped as augment_planes_kernel clamps it ---------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 12, 16), (3, 23, 359)], ids=_sid)
def test_table_outside_frame_is_clamped(backend, shape):
    dev = backend
    C, H, W = shape
    x, enc = _case(shape, 'half')
    zh, zw = int(H / 1.25), int(W / 1.25)
    raw = np.array([[1, 1, 99, -7, H + 5, W + 9, 0, 0],          # window larger than the frame: clamps to the frame = flip only
                    [0, 2, W, -3, zh, zw, 0, 0],                 # zoom-out window pushed back inside: x0 = W - zw, y0 = 0
                    [0, 7, 5, 5, 3, 3, 0, 0],                    # an unknown mode is mode 0
                    [0, 1, W + 4, H + 4, 0, -4, 0, 0]],          # an empty window is 1 x 1 at the last pixel
                   dtype=np.int32)
    index = np.array([[0, 1, 2, 3]])
    p = _packed_from(enc, shape, torch.uint8, dev)
    it = torch.from_numpy(raw).to(dev)
    got = _u8(unpack_augment(p, torch.from_numpy(index).to(dev), it))
    dense = ref.decode(enc, C * H * W, index).reshape((1, 4) + shape)
    known = [SpatialAugmentState(flip=True), SpatialAugmentState(mode=2, factor=1.25, x0=W - zw, y0=0), SpatialAugmentState()]
    want = augment_ref.planes_ref(torch.from_numpy(dense[:, :3].copy()), known).numpy()
    assert np.array_equal(got[:, :3], want)
    assert np.array_equal(got[0, 3], np.broadcast_to(dense[0, 3][:, H - 1:, W - 1:], shape))
    assert torch.equal(torch.from_numpy(got), A.augment_planes(unpack_frames(p, torch.from_numpy(index).to(dev)), it).cpu())
    p.check()


# ---- 3. the index ---------------------------------------------------------------------------------------------------------------------------
INDEXES = {'T3B2': np.array([[3, 1], [1, 3], [-1, 0]]), 'T2B3': np.array([[2, -1, 2], [0, 3, 1]])}


@pytest.mark.parametrize('shape', [(2, 40, 304), (3, 23, 359)], ids=_sid)
@pytest.mark.parametrize('lay', list(INDEXES))
def test_index(backend, shape, lay):
    """A permuted order, a frame repeated under two different table rows, -1 entries; then one entry out of range."""
    dev = backend
    x, enc = _case(shape, 'half')
    index = INDEXES[lay]
    B = index.shape[1]
    all_states = _states(*shape[1:])
    st = [all_states[3], all_states[5], all_states[1]][:B]        # every sample transformed, so a -1 frame shows "whatever the table says"
    p = pack_frames(torch.from_numpy(x.copy()).reshape((F_PACKED,) + shape).to(dev))
    it, _ = A.make_tables(st, shape[1:], dev)
    got = unpack_augment(p, torch.from_numpy(index).to(dev), it)
    want = _truth(x, enc, shape, index, st)
    assert np.array_equal(_u8(got), want)
    assert not _u8(got)[index == -1].any()
    p.check()
    assert torch.equal(got, A.augment_planes(unpack_frames(p, torch.from_numpy(index).to(dev)), it))
    for bad_value in (F_PACKED, -2):
        bad = index.copy()
        bad[1, 1] = bad_value
        zeroed = index.copy()
        zeroed[1, 1] = -1
        p.status.zero_()
        got = unpack_augment(p, torch.from_numpy(bad).to(dev), it)
        assert np.array_equal(_u8(got), _truth(x, enc, shape, zeroed, st))
        assert int(p.status[0]) == fc.STATUS_INDEX
        with pytest.raises(RuntimeError, match='index outside'):
            p.check()


# ---- 4. the reference-recorded augmentation fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cg.CASES))
def test_reference_golden(backend, name):
    """Pack the recorded input planes, run the fused call with the recorded states, compare with the reference's recorded output."""
    dev = backend
    gold = load_golden(name)
    hw = cg.CASES[name]['hw']
    st = [SpatialAugmentState(flip=bool(r[0]), mode=int(r[1]), x0=int(r[2]), y0=int(r[3]), factor=float(r[4])) for r in gold['states']]
    coded = torch.from_numpy(cg.coded_planes(hw)).to(dev)
    p = pack_frames(coded.unsqueeze(0))
    it, _ = A.make_tables(st, hw, dev)
    index = torch.zeros(1, len(st), dtype=torch.int64, device=dev)          # one packed frame under every recorded state
    got = unpack_augment(p, index, it)
    assert torch.equal(got[0].cpu(), torch.from_numpy(gold['coded']))
    p.check()


# ---- 5. out= inside a canary buffer; arrays that hold garbage ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 40, 304), (3, 23, 359)], ids=_sid)
def test_out_inside_canaries(backend, shape):
    dev = backend
    x, enc = _case(shape, 'half')
    st = _states(*shape[1:])[2:6]
    index = np.array([[0, 1, -1, 3], [2, 2, 1, 0]])
    want = _truth(x, enc, shape, index, st)
    p = _packed_from(enc, shape, torch.uint8, dev)
    it, _ = A.make_tables(st, shape[1:], dev)
    n = want.size
    for lead in (16, 3):                                                       # a whole line (16-byte stores when W % 16 == 0), an odd byte
        big = torch.full((n + 96,), 0xA5, dtype=torch.uint8, device=dev)
        base = (-big.data_ptr()) % 16 + lead
        out = big[base:base + n].view(want.shape)
        assert out.data_ptr() % 16 == lead % 16
        got = unpack_augment(p, torch.from_numpy(index).to(dev), it, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
        assert np.array_equal(host[base:base + n].reshape(want.shape), want)
        assert (host[:base] == 0xA5).all() and (host[base + n:] == 0xA5).all()
    p.check()


@pytest.mark.parametrize('what', ['truncated', 'garbage_values', 'garbage_everything'])
@pytest.mark.parametrize('shape', [(2, 40, 304), (3, 23, 359)], ids=_sid)
def test_garbage_arrays_stay_in_bounds(backend, shape, what):
    """Whatever the arrays hold, the call ends and nothing outside out changes; what the arrays still state truly is decoded truly."""
    dev = backend
    x, enc = _case(shape, 'half')
    enc = {k: v.copy() for k, v in enc.items()}
    rng = np.random.default_rng(11)
    nnz = enc['values'].shape[0]
    if what == 'truncated':
        enc['values'] = enc['values'][:nnz // 3]
    elif what == 'garbage_values':
        enc['values'] = rng.integers(0, 256, size=nnz, dtype=np.uint8)
    else:
        enc['values'] = rng.integers(0, 256, size=nnz // 2, dtype=np.uint8)
        enc['masks'] = rng.integers(0, 1 << 63, size=enc['masks'].shape, dtype=np.uint64) | (np.uint64(1) << np.uint64(63))
        enc['seg_offset'] = rng.integers(0, 1 << 32, size=enc['seg_offset'].shape, dtype=np.uint64).astype(np.uint32)
        enc['value_base'] = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, -5, 1 << 40, nnz][:F_PACKED + 1], dtype=np.int64)
    st = _states(*shape[1:])[2:6]
    index = np.array([[0, 1, 2, 3], [3, 2, 1, 0]])
    p = _packed_from(enc, shape, torch.uint8, dev)
    it, _ = A.make_tables(st, shape[1:], dev)
    n = index.size * int(np.prod(shape))
    big = torch.full((n + 96,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-big.data_ptr()) % 16 + 16
    out = big[base:base + n].view(tuple(index.shape) + shape)
    unpack_augment(p, torch.from_numpy(index).to(dev), it, out=out)
    host = big.cpu().numpy()
    assert (host[:base] == 0xA5).all() and (host[base + n:] == 0xA5).all()
    if what == 'truncated':                                                    # frame 0's values are all there: its outputs are exact
        keep = int(enc['value_base'][1]) <= enc['values'].shape[0]
        assert keep
        want = _truth(x, _case(shape, 'half')[1], shape, index, st)
        got = host[base:base + n].reshape(want.shape)
        assert np.array_equal(got[index == 0], want[index == 0])


# ---- 6. argument checks -------------------------------------------------------------------------------------------------------------------
def test_rejected_inputs(backend):
    dev = backend
    shape = (2, 12, 16)
    x, enc = _case(shape, 'half')
    p = _packed_from(enc, shape, torch.uint8, dev)
    it, _ = A.make_tables(_states(12, 16)[:2], (12, 16), dev)
    idx = torch.zeros(3, 2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match=r'index must be \(T, B=2\)'):
        unpack_augment(p, torch.zeros(2, 3, dtype=torch.int64, device=dev), it)
    with pytest.raises(ValueError, match=r'index must be \(T, B=2\)'):
        unpack_augment(p, torch.zeros(6, dtype=torch.int64, device=dev), it)
    with pytest.raises(ValueError, match='int64'):
        unpack_augment(p, idx.int(), it)
    with pytest.raises(ValueError, match='planes_table'):
        unpack_augment(p, idx, it.float())
    with pytest.raises(ValueError, match='out must be'):
        unpack_augment(p, idx, it, out=torch.empty(3, 2, 2, 12, 15, dtype=torch.uint8, device=dev))
    wide = PackedFrames((1, 1, 4096), torch.uint8, torch.zeros(1, 64, dtype=torch.int64, device=dev), torch.zeros(1, 2, dtype=torch.int32, device=dev),
                        torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match='W=4096 outside the supported range'):
        unpack_augment(wide, torch.zeros(1, 2, dtype=torch.int64, device=dev), it)


# ---- 7. graph capture (GPU only) ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture():
    """Captured once; replayed after the index, the table and the packed arrays were rewritten in place."""
    dev = torch.device('cuda', 0)
    shape = (2, 40, 304)
    st = list(_states(*shape[1:]))
    sets = [_case(shape, fill) for fill in ('half', 'sparse', 'full')]
    cap = max(s[1]['values'].shape[0] for s in sets)
    x0, enc0 = sets[0]
    p = _packed_from(enc0, shape, torch.uint8, dev)
    p.values = torch.zeros(cap, dtype=torch.uint8, device=dev)
    p.values[:enc0['values'].shape[0]] = torch.from_numpy(enc0['values'].copy()).to(dev)
    B = 3
    index = torch.tensor([[3, 0, -1], [2, 2, 1]], device=dev)
    it, ft = A.make_tables(st[:B], shape[1:], dev)
    out = torch.empty((2, B) + shape, dtype=torch.uint8, device=dev)
    unpack_augment(p, index, it, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_u8(out), _truth(x0, enc0, shape, index.cpu().numpy(), st[:B]))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        unpack_augment(p, index, it, out=out)
    for k, (x, enc) in enumerate(sets[1:]):
        new_index = np.array([[k, -1, 3], [1, k, k]])
        new_st = st[2 + 3 * k:5 + 3 * k]
        index.copy_(torch.from_numpy(new_index))
        A.write_tables(new_st, shape[1:], it, ft)
        p.masks.copy_(torch.from_numpy(enc['masks'].view(np.int64).copy()))
        p.seg_offset.copy_(torch.from_numpy(enc['seg_offset'].view(np.int32).copy()))
        p.value_base.copy_(torch.from_numpy(enc['value_base'].copy()))
        p.values.zero_()
        p.values[:enc['values'].shape[0]] = torch.from_numpy(enc['values'].copy()).to(dev)
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_u8(out), _truth(x, enc, shape, new_index, new_st))
        assert torch.equal(out, A.augment_planes(unpack_frames(p, index), it))
    p.check()


# ---- 8. opmodel and the header ----------------------------------------------------------------------------------------------------------------
def test_opmodel_prices_the_entry_point():
    F, Fout, nnz, B, C, H, W = 7, 12, 4321, 4, 3, 23, 359
    E = C * H * W
    Gf, Sf = fc.geometry(E)
    assert _header.PROTOS['rvt_frames_unpack_augment'].argnames == (
        'masks', 'seg_offset', 'value_base', 'values', 'values_len', 'F', 'E', 'index', 'Fout', 'table', 'B', 'C', 'H', 'W', 'out', 'status',
        'stream')
    args = (1, 2, 3, 4, nnz, F, E, 5, Fout, 6, B, C, H, W, 7, 8, None)
    per_frame = 8 * Gf + 4 * (Sf + 1) + 8
    want = 1.0 * Fout * E + Fout * (per_frame + 8) + nnz + 32.0 * B
    assert opmodel.frames_unpack_augment_bytes(Fout, E, nnz, B) == want == opmodel.frames_unpack_bytes(Fout, E, nnz) + 32.0 * B
    assert opmodel.model('rvt_frames_unpack_augment', args) == (0.0, want)
    assert opmodel.executed('rvt_frames_unpack_augment', args) == 0.0
    # one launch moves less than the two it replaces: no dense tensor written and read back
    two = opmodel.model('rvt_frames_unpack', args[:9] + (7, 8, None))[1] + opmodel.model('rvt_augment_planes', (1, 2, 3, Fout, B, C, H, W, None))[1]
    assert want + 2.0 * Fout * E == two
