"""BatchLoader over stores of frame-cache format version 2 (framecache.PackedFrames2): every route that serves version 1 but the
fused one.  The yardstick is the same loader over the same data as version-1 stores (framecache.convert, host-side numpy) with the
same seeds: the batches - EV_REPR, the label tensors, both masks, the drawn augmentation states - must be equal bit for bit."""
import numpy as np
import pytest
import torch

from rvt_amd import framecache as fc
from rvt_amd.framecache import PackedFrames, PackedFrames2
from rvt_amd.loader import BatchLoader, SequenceStore
from rvt_amd.types import DatasetSamplingMode as SM, Mode
from tests import framecache2_ref as ref
from tests.backends import backend  # noqa: F401
from tests.test_framecache2 import packed_from
from tests.test_loader import AUGM
from tests.test_loader_gather import SHAPE, STORES, T, _epoch, _frames, _rows, _same

ROUTES = {'device': dict(resident='device'), 'host_copy': dict(resident='host', staging='copy'),
          'host_gather': dict(resident='host', staging='gather')}


def _stores(version):
    """The four recordings of tests/test_loader_gather.py as version-2 stores built by the restatement, or as their conversion."""
    out = []
    for k in sorted(STORES):
        N, o2r = STORES[k]
        rows = [_rows(100 * k + f, 1 + f % 2) for f in range(len(o2r))]
        frames = packed_from(ref.encode(_frames(k, N).reshape(N, -1)), SHAPE, torch.uint8, 'cpu')
        out.append(SequenceStore(frames if version == 2 else fc.convert(frames, 1), np.asarray(o2r, dtype=np.int64), rows))
    return out


def _loader(version, mode, dataset_mode, dev, B, **kw):
    augm = AUGM if dataset_mode == Mode.TRAIN else None
    return BatchLoader(_stores(version), B, T, mode, dataset_mode, device=dev, dataset_hw=SHAPE[1:], augm_config=augm, seed=6, **kw)


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('mode', [SM.RANDOM, SM.STREAM], ids=['random', 'stream'])
def test_batches_equal_those_of_the_converted_stores(backend, mode, route):
    v2 = _loader(2, mode, Mode.TRAIN, backend, 2, **ROUTES[route])
    assert v2.version == 2 and all(isinstance(s.frames, PackedFrames2) for s in v2.stores) and not v2.fused
    if route == 'device':
        assert isinstance(v2.packed, PackedFrames2)
    else:
        sets = [st for p in v2.parts.values() for st in p['staging']]
        assert all(isinstance(st.dev, PackedFrames2) for st in sets)
        # sized from the stores' largest per-frame value and group counts
        n = T * 2
        cap = max(int(np.diff(s.frames.value_base.numpy()).max()) for s in v2.stores)
        mcap = max(int(np.diff(s.frames.mask_base.numpy()).max()) for s in v2.stores)
        assert all(st.dev.values.numel() == n * cap and st.dev.masks.numel() == n * mcap for st in sets)
        if route == 'host_gather':
            assert v2.gatherer.version == 2 and all(st.table_dev.numel() == 8 * n for st in sets)
    got = _epoch(v2, 17)
    assert any(e['ev'].any() for e in got) and len({(s.flip, s.mode) for e in got for s in e['states']}) > 1
    v1 = _loader(1, mode, Mode.TRAIN, backend, 2, **ROUTES[route])
    assert v1.version == 1 and all(isinstance(s.frames, PackedFrames) for s in v1.stores)
    _same(got, _epoch(v1, 17), 3)
    _same(_epoch(v2, 18), _epoch(v1, 18), 3)                          # a second epoch over the same staging sets


def test_fused_route_and_mixed_versions_are_refused():
    with pytest.raises(ValueError, match='fused=True'):
        _loader(2, SM.RANDOM, Mode.TRAIN, 'cpu', 2, fused=True)
    mixed = _stores(2)[:2] + _stores(1)[2:]
    with pytest.raises(ValueError, match='format versions 1 and 2'):
        BatchLoader(mixed, 2, T, SM.RANDOM, Mode.TRAIN, device='cpu', dataset_hw=SHAPE[1:], seed=6)


def test_sequence_store_save_load_keeps_the_version(tmp_path):
    s = _stores(2)[1]
    s.save(tmp_path / 'rec')
    q = SequenceStore.load(tmp_path / 'rec')
    assert isinstance(q.frames, PackedFrames2) and q.num_windows == s.num_windows
    for k in ref.KEYS:
        assert torch.equal(getattr(q.frames, k), getattr(s.frames, k)), k
    assert np.array_equal(q.rows, s.rows) and np.array_equal(q.objframe_idx_2_repr_idx, s.objframe_idx_2_repr_idx)
