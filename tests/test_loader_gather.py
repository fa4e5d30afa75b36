"""BatchLoader(resident='host', staging='gather'): the frames of the next batch fetched from the host stores by one gather launch
(framecache.FrameGather) instead of collected on the host and copied.  The batches must equal those of staging='copy' and of
resident='device' bit for bit: the same seed, augmentation on, whole epochs, so that both staging buffers are reused."""
import numpy as np
import pytest
import torch

from rvt_amd.loader import BatchLoader, SequenceStore
from rvt_amd.types import DataType, DatasetSamplingMode as SM, Mode
from tests.backends import backend  # noqa: F401
from tests.test_loader import AUGM, _host_packed

T = 3
SHAPE = (20, 12, 16)
# four tiny recordings of unequal length: dense labels; gaps larger than T (several clusters, a padded tail); one label; a late start
STORES = {0: (11, [2, 3, 5, 8, 10]), 1: (26, [1, 2, 12, 14, 24]), 2: (5, [3]), 3: (17, [6, 7, 9, 15, 16])}


def _frames(k, N):
    """Window w of recording k: a fill that differs per window (some planes empty, one window all zero), values that name (k, w)."""
    rng = np.random.default_rng(50 + k)
    x = rng.integers(1, 256, size=(N,) + SHAPE, dtype=np.uint8) * (rng.random((N,) + SHAPE) < rng.random((N, 1, 1, 1)) * 0.3)
    x[:, 0, 0, 0] = np.arange(1, N + 1)
    x[:, 0, 0, 1] = k + 1
    x[N // 2] = 0
    return x


def _rows(frame, n):
    r = np.zeros((n, 7), dtype=np.float32)
    for i in range(n):
        r[i] = (1000 * frame + i, 2 + i, 3, 5, 4, i % 3, 1.0)
    return r


def _stores():
    out = []
    for k in sorted(STORES):
        N, o2r = STORES[k]
        rows = [_rows(100 * k + f, 1 + f % 2) for f in range(len(o2r))]
        out.append(SequenceStore(_host_packed(_frames(k, N), SHAPE), np.asarray(o2r, dtype=np.int64), rows))
    return out


def _loader(mode, dataset_mode, dev, B, **kw):
    augm = AUGM if dataset_mode == Mode.TRAIN else None
    return BatchLoader(_stores(), B, T, mode, dataset_mode, device=dev, dataset_hw=SHAPE[1:], augm_config=augm, seed=6, **kw)


def _flat(v):
    return torch.stack(list(v)) if isinstance(v, (list, tuple)) else v


def _epoch(ld, seed):
    torch.manual_seed(seed)
    out = []
    for batch in ld:
        parts = batch if SM.RANDOM in batch or SM.STREAM in batch else {None: batch}
        for part in parts.values():
            d = part['data']
            out.append(dict(ev=_flat(d[DataType.EV_REPR]).cpu().clone(), first=d[DataType.IS_FIRST_SAMPLE].cpu().clone(),
                            pad=_flat(d[DataType.IS_PADDED_MASK]).cpu().clone(), states=part['states'],
                            labels=[[None if lab is None else lab.clone() for lab in sl.labels] for sl in d[DataType.OBJLABELS_SEQ]]))
    return out


def _same(a, b, min_batches):
    assert len(a) == len(b) >= min_batches
    for x, y in zip(a, b):
        assert torch.equal(x['ev'], y['ev']) and torch.equal(x['first'], y['first']) and torch.equal(x['pad'], y['pad'])
        assert x['states'] == y['states']
        for lx, ly in zip(x['labels'], y['labels']):
            assert [(p is None) for p in lx] == [(q is None) for q in ly]
            assert all(torch.equal(p, q) for p, q in zip(lx, ly) if p is not None)


@pytest.mark.parametrize('B', [2, 3])
@pytest.mark.parametrize('mode,dataset_mode', [(SM.RANDOM, Mode.TRAIN), (SM.STREAM, Mode.TRAIN), (SM.STREAM, Mode.VAL), (SM.MIXED, Mode.TRAIN)],
                         ids=['random', 'stream_train', 'stream_eval', 'mixed'])
def test_gather_staging_equals_copy_and_device(backend, mode, dataset_mode, B):
    gather = _loader(mode, dataset_mode, backend, B, resident='host', staging='gather')
    assert gather.staging == 'gather' and gather.gatherer.num_frames == sum(N for N, _ in STORES.values())
    assert all(st.host is None and st.table_dev.numel() == 4 * T * p['B'] for p in gather.parts.values() for st in p['staging'])
    got = _epoch(gather, 17)
    assert any(e['ev'].any() for e in got) and (dataset_mode != Mode.TRAIN or len({(s.flip, s.mode) for e in got for s in e['states']}) > 1)
    copy = _loader(mode, dataset_mode, backend, B, resident='host', staging='copy')
    assert copy.staging == 'copy' and all(st.table_dev is None for p in copy.parts.values() for st in p['staging'])
    min_batches = 6 if mode == SM.MIXED else 3                       # (a mixed batch is two part batches)
    _same(got, _epoch(copy, 17), min_batches)
    _same(got, _epoch(_loader(mode, dataset_mode, backend, B, resident='device'), 17), min_batches)
    _same(_epoch(gather, 18), _epoch(copy, 18), min_batches)          # a second epoch over the same staging sets


def test_staging_needs_host_residency():
    for staging in ('copy', 'gather'):
        with pytest.raises(ValueError, match="needs resident='host'"):
            _loader(SM.RANDOM, Mode.TRAIN, 'cpu', 2, resident='device', staging=staging)
    with pytest.raises(ValueError, match='staging must be'):
        _loader(SM.RANDOM, Mode.TRAIN, 'cpu', 2, resident='host', staging='dma')


def test_default_staging(backend):
    assert _loader(SM.RANDOM, Mode.TRAIN, backend, 2, resident='host').staging == 'gather'   # the measured default (profiles/frames_gather_bench.txt)
    assert _loader(SM.RANDOM, Mode.TRAIN, backend, 2).staging is None
