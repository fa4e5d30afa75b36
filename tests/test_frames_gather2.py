"""rvt_frames_gather2 (rvt_amd/csrc/capi_frames2.hip, framecache.FrameGather / gather_frames over PackedFrames2 stores): frames of
format version 2 named by address, out of several packed stores, into one packed set on the device.  Every comparison is bit for
bit.  The yardsticks are not the code under test: the numpy restatement of the format (tests/framecache2_ref.py) builds the stores,
and the host-side `slice` / `concat` say what a gather must produce."""
import functools

import numpy as np
import pytest
import torch

from rvt_amd import _lib, framecache as fc
from rvt_amd.framecache import FrameGather, PackedFrames2, gather_frames, unpack_frames
from tests import framecache2_ref as ref
from tests import framecache_ref as ref1
from tests.backends import backend  # noqa: F401
from tests.test_framecache2 import CANARY, CANARY64, SHAPES, make_frames, packed_from

CANARY32 = int.from_bytes(bytes([CANARY] * 4), 'little', signed=True)
SIZES = [30, 65, 4097, 8257, 3840, 5883]


@functools.lru_cache(maxsize=None)
def _frames(E):
    """Three recordings of different F as uint8 [F][E]: mixed fills with empty frames between (6), only all-zero frames (3: empty
    `masks` and `values`), blobs (7)."""
    a = np.concatenate([make_frames(1, E, 'full'), np.zeros((1, E), np.uint8), make_frames(1, E, 'u30'), make_frames(1, E, 'last_byte'),
                        np.zeros((1, E), np.uint8), make_frames(1, E, 'b63_64')])
    xs = (a, np.zeros((3, E), dtype=np.uint8), make_frames(7, E, 'blobs', seed=3))
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def _host_stores(E):
    """The host packed sets of `_frames` (never written to) and their frames one behind the other."""
    xs = _frames(E)
    stores = tuple(packed_from(ref.encode(x), SHAPES[E], torch.uint8, 'cpu') for x in xs)
    assert stores[1].values.numel() == 0 and stores[1].masks.numel() == 0
    return stores, np.concatenate(xs)


def _want(stores, idx):
    """concat of the single-frame slices in index order: what the gather must equal."""
    base = np.concatenate(([0], np.cumsum([s.num_frames for s in stores])))
    parts = []
    for i in idx:
        k = int(np.searchsorted(base, i, side='right')) - 1
        parts.append(stores[k].slice(int(i - base[k]), int(i - base[k]) + 1))
    return fc.concat(parts)


def _assert_set(got: PackedFrames2, want: PackedFrames2, n=None, nnz=None, ng=None):
    n = want.num_frames if n is None else n
    nnz = int(want.value_base[-1]) if nnz is None else nnz
    ng = int(want.mask_base[-1]) if ng is None else ng
    for k in ('group_mask', 'seg_offset', 'grp_offset'):
        assert torch.equal(getattr(got, k)[:n].cpu(), getattr(want, k)), k
    assert torch.equal(got.value_base[:n + 1].cpu(), want.value_base) and torch.equal(got.mask_base[:n + 1].cpu(), want.mask_base)
    assert torch.equal(got.masks[:ng].cpu(), want.masks[:ng]) and torch.equal(got.values[:nnz].cpu(), want.values[:nnz])


SHUFFLED = np.array([3, 9, 15, 3, 7, 1, 10, 9, 0, 4, 12, 6, 2, 14, 11, 13, 5, 8, 0])      # every frame, repeats, empty frames between


# ---- 1. equality with slice + concat -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_blocks', [1, 3, 0], ids=['blocks1', 'blocks3', 'default'])
@pytest.mark.parametrize('E', SIZES)
def test_gather_equals_slice_concat(backend, E, max_blocks):
    host, x = _host_stores(E)
    stores = [s.to(backend) for s in host]
    g = FrameGather(stores, backend)
    assert g.version == 2 and g.cols == 8 and g.num_frames == 16 and g.base.tolist() == [0, 6, 9, 16]
    for idx in (SHUFFLED, np.array([12]), np.array([7]), np.arange(10, 14)):
        want = _want(host, idx)
        out = g.empty(len(idx) + 2, want.nnz() + 5, want.ngroups() + 3)             # spare rows and room
        tab = torch.zeros(8 * (len(idx) + 1), dtype=torch.int64, device=backend)
        assert g.gather(idx.reshape(1, -1), out, table_dev=tab, max_blocks=max_blocks) is out
        out.check()
        _assert_set(out, want)
        assert np.array_equal(tab[:8 * len(idx)].cpu().numpy().reshape(-1, 8), g.table(idx))
    got = gather_frames(stores, SHUFFLED)                                             # the one-shot form: sized exactly
    want = _want(host, SHUFFLED)
    assert isinstance(got, PackedFrames2) and got.num_frames == len(SHUFFLED) and got.device == backend
    got.check()
    _assert_set(got, want)
    assert got.values.numel() == want.nnz() and got.masks.numel() == want.ngroups()
    assert np.array_equal(unpack_frames(got).cpu().numpy().reshape(len(SHUFFLED), E), x[SHUFFLED])


# ---- 2. a mask run across a 16 KiB piece boundary ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case():
    """A frame of 64 * 2100 bytes, all non-zero: 2100 stored masks = 16800 bytes, more than one 16 KiB piece; and a sparse one."""
    E = 64 * 2100
    x = np.concatenate([make_frames(1, E, 'u1'), make_frames(1, E, 'full'), make_frames(1, E, 'blobs')])
    x.setflags(write=False)
    return x, packed_from(ref.encode(x), (1, 2100, 64), torch.uint8, 'cpu')


@pytest.mark.parametrize('max_blocks', [1, 0], ids=['blocks1', 'default'])
def test_mask_run_across_a_piece_boundary(backend, max_blocks):
    x, host = _long_case()
    assert int(host.mask_base[2] - host.mask_base[1]) == 2100 and 8 * 2100 > 16384
    store = host.to(backend)
    idx = np.array([0, 1, 2, 1])
    want = _want([host], idx)
    g = FrameGather([store], backend)
    out = g.gather(idx, g.empty(len(idx), want.nnz(), want.ngroups()), max_blocks=max_blocks)
    out.check()
    _assert_set(out, want)
    assert np.array_equal(unpack_frames(out).cpu().numpy().reshape(len(idx), -1), x[idx])


# ---- 3. capacity, bad counts and the write discipline ---------------------------------------------------------------------------------
def _guarded(n, E, cap, mcap, dev, odd):
    """A version-2 set of n frames whose seven arrays (and status) are views into canary-filled buffers, at 16-byte aligned
    addresses or (odd) at the least alignment each array admits.  Returns (set, check); check(written, mwritten) asserts the
    canaries around the arrays and behind the written value bytes and mask words."""
    Sf = fc.geometry(E)[1]
    l8, l4, l1 = (1, 1, 3) if odd else (2, 4, 16)
    bg = torch.full((n * Sf + 8,), CANARY64, dtype=torch.int64, device=dev)
    bs = torch.full((n * (Sf + 1) + 16,), CANARY32, dtype=torch.int32, device=dev)
    bo = torch.full((n * (Sf + 1) + 16,), CANARY32, dtype=torch.int32, device=dev)
    bv = torch.full((n + 1 + 8,), CANARY64, dtype=torch.int64, device=dev)
    bb = torch.full((n + 1 + 8,), CANARY64, dtype=torch.int64, device=dev)
    bm = torch.full((mcap + 8,), CANARY64, dtype=torch.int64, device=dev)
    by = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device=dev)
    bt = torch.full((3,), CANARY32, dtype=torch.int32, device=dev)
    out = PackedFrames2(SHAPES[E], torch.uint8, bg[l8:l8 + n * Sf].view(n, Sf), bs[l4:l4 + n * (Sf + 1)].view(n, Sf + 1),
                        bo[l4:l4 + n * (Sf + 1)].view(n, Sf + 1), bv[l8:l8 + n + 1], bb[l8:l8 + n + 1], bm[l8:l8 + mcap], by[l1:l1 + cap], bt[1:2])

    def check(written=cap, mwritten=mcap):
        assert (bg[:l8] == CANARY64).all() and (bg[l8 + n * Sf:] == CANARY64).all(), 'group_mask'
        assert (bs[:l4] == CANARY32).all() and (bs[l4 + n * (Sf + 1):] == CANARY32).all(), 'seg_offset'
        assert (bo[:l4] == CANARY32).all() and (bo[l4 + n * (Sf + 1):] == CANARY32).all(), 'grp_offset'
        assert (bv[:l8] == CANARY64).all() and (bv[l8 + n + 1:] == CANARY64).all(), 'value_base'
        assert (bb[:l8] == CANARY64).all() and (bb[l8 + n + 1:] == CANARY64).all(), 'mask_base'
        assert (bm[:l8] == CANARY64).all() and (bm[l8 + mwritten:] == CANARY64).all(), 'masks'
        assert (by[:l1] == CANARY).all() and (by[l1 + written:] == CANARY).all(), 'values'
        assert int(bt[0]) == CANARY32 and int(bt[2]) == CANARY32, 'status'
    return out, check


@pytest.mark.parametrize('odd', [False, True], ids=['aligned16', 'odd'])
@pytest.mark.parametrize('short', ['values_one_byte', 'masks_one_word', 'both_zero', 'room'])
def test_capacity_and_canaries(backend, short, odd):
    E = 4097
    host, _ = _host_stores(E)
    stores = [s.to(backend) for s in host]
    want = _want(host, SHUFFLED)
    nnz, ng = want.nnz(), want.ngroups()
    cap = {'values_one_byte': nnz - 1, 'masks_one_word': nnz, 'both_zero': 0, 'room': nnz}[short]
    mcap = {'values_one_byte': ng, 'masks_one_word': ng - 1, 'both_zero': 0, 'room': ng}[short]
    g = FrameGather(stores, backend)
    out, canaries = _guarded(len(SHUFFLED), E, cap, mcap, backend, odd)
    g.gather(SHUFFLED, out)
    if short == 'room':
        out.check()
    else:
        assert int(out.status[0]) == fc.STATUS_CAPACITY
        with pytest.raises(RuntimeError, match='capacity'):
            out.check()
    assert out.nnz() == nnz and out.ngroups() == ng                                   # the five index arrays are complete
    _assert_set(out, want, nnz=cap, ng=mcap)                                          # exactly the entries below the capacities
    canaries()


@pytest.mark.parametrize('bad', ['count_minus1', 'count_E_plus_1', 'groups_minus1', 'groups_Gf_plus_1'])
def test_bad_count_is_taken_as_zero(backend, bad):
    E = 4097
    Gf = fc.geometry(E)[0]
    host, _ = _host_stores(E)
    stores = [s.to(backend) for s in host]
    idx = np.array([9, 0, 12, 2, 15])
    g = FrameGather(stores, backend)
    rows = g.table(idx)
    assert rows.shape == (5, 8) and rows.dtype == np.int64 and rows[1, 5] == E and rows[1, 6] == Gf and (rows[:, 7] == 0).all()     # frame 0 is dense
    col = 5 if bad.startswith('count') else 6
    rows[1, col] = {'count_minus1': -1, 'count_E_plus_1': E + 1, 'groups_minus1': -1, 'groups_Gf_plus_1': Gf + 1}[bad]
    want = _want(host, idx)
    counts, groups = np.diff(want.value_base.numpy()), np.diff(want.mask_base.numpy())
    keepv, keepm = np.ones(want.nnz(), dtype=bool), np.ones(want.ngroups(), dtype=bool)
    if col == 5:
        keepv[int(want.value_base[1]):int(want.value_base[2])] = False
        counts[1] = 0
    else:
        keepm[int(want.mask_base[1]):int(want.mask_base[2])] = False
        groups[1] = 0
    out, canaries = _guarded(len(idx), E, int(counts.sum()) + 7, int(groups.sum()) + 2, backend, True)
    g.gather(None, out, rows=rows)
    assert int(out.status[0]) == fc.STATUS_COUNT
    with pytest.raises(RuntimeError, match='outside'):
        out.check()
    for k in ('group_mask', 'seg_offset', 'grp_offset'):
        assert torch.equal(getattr(out, k).cpu(), getattr(want, k)), k
    assert np.array_equal(out.value_base.cpu().numpy(), np.concatenate(([0], np.cumsum(counts))))
    assert np.array_equal(out.mask_base.cpu().numpy(), np.concatenate(([0], np.cumsum(groups))))
    assert np.array_equal(out.values[:int(counts.sum())].cpu().numpy(), want.values.numpy()[keepv])
    assert np.array_equal(out.masks[:int(groups.sum())].cpu().numpy(), want.masks.numpy()[keepm])
    canaries(written=int(counts.sum()), mwritten=int(groups.sum()))


def test_guards(backend):
    host, _ = _host_stores(4097)
    g = FrameGather(host, 'cpu')
    v1 = fc.convert(host[0], 1)
    with pytest.raises(ValueError, match='format version'):
        FrameGather([host[0], v1], 'cpu')
    with pytest.raises(ValueError, match='format version'):
        FrameGather([v1, host[0]], 'cpu')
    with pytest.raises(ValueError, match='format version'):
        g.gather([0], FrameGather([v1], 'cpu').empty(1, 100))
    with pytest.raises(ValueError, match=r'rows must be int64 \[n\]\[8\]'):
        g.gather(None, g.empty(2, 100, 10), rows=np.zeros((2, 4), dtype=np.int64))
    assert g.table([]).shape == (0, 8)
    Sf = fc.geometry(4097)[1]
    rows = g.table(np.arange(16))
    assert rows[7, 0] == host[1].group_mask.data_ptr() + 8 * Sf and rows[10, 2] == host[2].grp_offset.data_ptr() + 4 * (Sf + 1)
    assert rows[11, 3] == host[2].masks.data_ptr() + 8 * int(host[2].mask_base[2]) and rows[11, 4] == host[2].values.data_ptr() + int(host[2].value_base[2])
    assert g.max_count == int(rows[:, 5].max()) and g.max_groups == int(rows[:, 6].max())


# ---- 4. pinned host stores, a device destination; graph replay (GPU only) ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('E', [4097, 3840])
def test_pinned_sources(E):
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    host, x = _host_stores(E)
    stores = [s.pin_memory() for s in host]
    assert all(s.group_mask.is_pinned() and s.grp_offset.is_pinned() for s in stores)
    g = FrameGather(stores, dev)
    for idx in (SHUFFLED, np.array([7]), np.arange(10, 14)):
        want = _want(host, idx)
        out = g.gather(idx, g.empty(len(idx), want.nnz(), want.ngroups()))
        out.check()
        _assert_set(out, want)
        assert np.array_equal(unpack_frames(out).cpu().numpy().reshape(len(idx), E), x[idx])
    mixed = [stores[0], host[1].to(dev), stores[2]]                                     # device and pinned stores in one table
    _assert_set(gather_frames(mixed, SHUFFLED).check(), _want(host, SHUFFLED))


@pytest.mark.gpu
def test_graph_replay_follows_the_table():
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    E = 8257
    host, x = _host_stores(E)
    g = FrameGather([s.pin_memory() for s in host], dev)
    n = 6
    orders = [np.array([0, 9, 10, 3, 6, 15]), np.array([12, 7, 2, 2, 14, 5]), np.array([8, 4, 13, 11, 1, 0])]
    out = g.empty(n, n * E)
    table = torch.zeros(8 * n, dtype=torch.int64, device=dev)
    index = torch.tensor([[5, 0, -1], [2, 2, 4]], device=dev)
    dense = torch.empty(tuple(index.shape) + SHAPES[E], dtype=torch.uint8, device=dev)
    table.copy_(torch.from_numpy(g.table(orders[0]).reshape(-1)))
    g.launch(table, n, out)                                                           # eager warm-up
    unpack_frames(out, index, out=dense)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.launch(table, n, out)
        unpack_frames(out, index, out=dense)
    for order in orders[1:]:
        table.copy_(torch.from_numpy(g.table(order).reshape(-1)))                     # other frames of other stores, the same addresses
        for t in (out.group_mask, out.seg_offset, out.grp_offset, out.value_base, out.mask_base, out.masks):
            t.fill_(-1)
        out.values.fill_(0)
        dense.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        out.check()
        _assert_set(out, _want(host, order))
        want = np.zeros((index.numel(), E), dtype=np.uint8)
        for j, i in enumerate(index.reshape(-1).tolist()):
            if i >= 0:
                want[j] = x[order[i]]
        assert np.array_equal(dense.cpu().numpy().reshape(-1, E), want)
        eager = g.gather(order, g.empty(n, n * E))
        _assert_set(out, eager.check().to('cpu'))
