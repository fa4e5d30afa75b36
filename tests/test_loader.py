"""Epoch loader over the frame cache (rvt_amd/loader.py): index rules, epoch behaviour of the three sampling modes, the batches
against the numpy restatements (tests/framecache_ref.py decode + tests/augment_ref.py), the step on loader batches, and store I/O.

Frames are (2, 12, 16) uint8 whose bytes encode the window number (plane 0) and the recording (plane 1), so window ranges are read
back from the data.  The index rules are checked against fixtures recorded from the unmodified reference classes
(tests/golden/loader_*.npz, cases in tests/casegen_loader.py, recorder tests/make_golden_loader.py) and on hand-worked values of the
reference's rules (sequence_rnd.py:24-50, sequence_for_streaming.py:25-54, 72-86, stream_sharded_datapipe.py:19-67, genx.py:116-129,
dataset_rnd.py:115-149)."""
import numpy as np
import pytest
import torch

from rvt_amd import augment as A, loader as LD
from rvt_amd.framecache import PackedFrames
from rvt_amd.loader import BatchLoader, SequenceStore, SparseLabels
from rvt_amd.step import BackboneSequenceModule
from rvt_amd.types import DataType, DatasetSamplingMode as SM, Mode
from tests import augment_ref, casegen, casegen_loader as cgl, framecache_ref as ref
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden

T = 5
SHAPE = (2, 12, 16)
STREAM_AUGM = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.8, zoom_out=dict(weight=1, factor=dict(min=1, max=1.2))))
RANDOM_AUGM = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)), zoom_out=dict(weight=2, factor=dict(min=1, max=1.2))))
AUGM = dict(random=RANDOM_AUGM, stream=STREAM_AUGM)


def _host_packed(x, shape):
    enc = ref.encode(x.reshape(x.shape[0], -1))
    return PackedFrames(tuple(shape), torch.uint8, torch.from_numpy(enc['masks'].view(np.int64).copy()),
                        torch.from_numpy(enc['seg_offset'].view(np.int32).copy()), torch.from_numpy(enc['value_base'].copy()),
                        torch.from_numpy(enc['values'].copy()), torch.zeros(1, dtype=torch.int32))


def _coded_frames(store_id, N):
    """Window w of recording k: plane 0 holds w + 1 on a sparse pattern (corners included), plane 1 holds k + 1."""
    x = np.zeros((N,) + SHAPE, dtype=np.uint8)
    pat = np.zeros(SHAPE[1:], dtype=bool)
    pat[::3, ::2] = True
    pat[0, 0] = pat[-1, -1] = pat[0, -1] = pat[-1, 0] = True
    for w in range(N):
        x[w, 0][pat] = w + 1
        x[w, 1][pat.T.reshape(SHAPE[1:])] = store_id + 1
    return x


def _rows(frame, n):
    r = np.zeros((n, 7), dtype=np.float32)
    for i in range(n):
        r[i] = (1000 * frame + i, 2 + i, 3, 5, 4, i % 3, 1.0)
    return r


def _store(store_id, N, o2r, nrows=None):
    x = _coded_frames(store_id, N)
    rows = [_rows(100 * store_id + f, (nrows or {}).get(f, 1 + f % 2)) for f in range(len(o2r))]
    return SequenceStore(_host_packed(x, SHAPE), np.asarray(o2r, dtype=np.int64), rows), x


# three tiny recordings: dense labels; label gaps larger than T (three clusters) and a padded tail; a single labelled frame
STORES = {0: (14, [2, 4, 5, 8, 11]), 1: (43, [1, 3, 20, 22, 40]), 2: (9, [6])}


def _three():
    built = [_store(k, *STORES[k]) for k in sorted(STORES)]
    return [b[0] for b in built], [b[1] for b in built]


def _loader(mode, dataset_mode, dev='cpu', B=2, **kw):
    stores, _ = _three()
    return BatchLoader(stores, B, T, mode, dataset_mode, device=dev, dataset_hw=SHAPE[1:], **kw)


# ---- 1. index rules ------------------------------------------------------------------------------------------------------------------------
def test_random_access_rules():
    o2r = np.array([2, 4, 5, 8, 11])
    assert LD.random_access_offset(o2r, T) == 1 and LD.random_access_len(o2r, T) == 4          # first label before window T - 1
    assert [LD.random_access_item(o2r, T, i) for i in range(4)] == [(0, 5), (1, 6), (4, 9), (7, 12)]
    assert LD.random_access_offset(np.array([1, 3]), T) == 2 and LD.random_access_len(np.array([1, 3]), T) == 0   # no label reachable
    assert LD.random_access_len(np.array([6]), T) == 1 and LD.random_access_item(np.array([6]), T, 0) == (2, 7)
    store, _ = _store(0, *STORES[0])
    s = LD.random_access_sample(store, 0, T, 1, only_load_end_labels=False)
    assert s.windows.tolist() == [1, 2, 3, 4, 5] and s.is_first_sample and not s.is_padded_mask.any()
    assert [None if lab is None else lab.shape[0] for lab in s.labels] == [None, 1, None, 2, 1]   # frames 0 (w2), 1 (w4), 2 (w5)
    assert np.array_equal(s.labels[3], store.frame_rows(1))
    e = LD.random_access_sample(store, 0, T, 1, only_load_end_labels=True)
    assert [None if lab is None else lab.shape[0] for lab in e.labels] == [None, None, None, None, 1]


def test_streaming_rules():
    assert LD.streaming_range(np.array([2, 4, 5, 8, 11]), 14, T) == (0, 14)
    assert LD.streaming_range(np.array([20, 22]), 43, T) == (16, 43)
    assert LD.streaming_chunks(0, 14, T) == [(0, 5), (5, 10), (10, 14)]                          # N no multiple of T: a padded tail
    assert LD.streaming_chunks(16, 26, T) == [(16, 21), (21, 26)]
    assert LD.label_cluster_ranges(np.array([1, 3, 20, 22, 40]), T) == [(0, 4), (16, 23), (36, 41)]   # gaps larger than T
    assert LD.label_cluster_ranges(np.array([2, 4, 5, 8, 11]), T) == [(0, 12)]                    # dense: 8 - 5 <= T, 11 - 8 <= T
    assert LD.label_cluster_ranges(np.array([0, 5, 11]), T) == [(0, 6), (7, 12)]                  # a gap of exactly T stays, T + 1 splits
    assert LD.label_cluster_ranges(np.array([6]), T) == [(2, 7)]
    store, _ = _store(0, *STORES[0])
    chunks = LD.streaming_chunks(0, 14, T)
    s0, s2 = LD.streaming_sample(store, 0, T, chunks[0], 0), LD.streaming_sample(store, 0, T, chunks[2], 2)
    assert s0.is_first_sample and not s2.is_first_sample
    assert s2.windows.tolist() == [10, 11, 12, 13, -1] and s2.is_padded_mask.tolist() == [False] * 4 + [True]
    assert s2.labels[1] is not None and s2.labels[4] is None and [lab is None for lab in s2.labels] == [True, False, True, True, True]
    p = LD.padded_sample(T)
    assert p.is_padded_mask.all() and not p.is_first_sample and p.labels == [None] * T


def test_sharding_rules():
    lengths = (5, 9, 2, 7, 7, 1, 3)                                  # sorted long to short, stable: 1 3 4 0 6 2 5
    assert LD.assign_to_worker(lengths, 1, 0) == [1, 3, 4, 0, 6, 2, 5]
    assert [LD.assign_to_worker(lengths, 2, r) for r in range(2)] == [[1, 0, 6], [3, 4, 2, 5]]          # pyramid 0 1 1 0 0 1 1
    assert [LD.assign_to_worker(lengths, 3, r) for r in range(3)] == [[1, 2, 5], [3, 6], [4, 0]]        # pyramid 0 1 2 2 1 0 0
    assert LD.assign_to_slots([9, 5, 3], 2) == [[0], [1, 2]]
    assert LD.assign_to_slots([9, 5, 3], 1) == [[0, 1, 2]]
    assert LD.assign_to_slots([2, 7, 7, 1], 2) == [[1, 3], [2, 0]]   # 7 7 2 1 dealt 0 1 1 0
    with pytest.raises(AssertionError, match="Each worker must at least get 'batch_size' number of datapipes"):
        LD.assign_to_slots([7, 3], 3)
    with pytest.raises(AssertionError):
        LD.assign_to_worker((3, 2), 3, 0)


@pytest.mark.parametrize('B,wr,ws,want', [(24, 1, 1, (12, 12)), (8, 1, 1, (4, 4)), (2, 1, 1, (1, 1)), (5, 3, 1, (4, 1)), (5, 1, 1, (2, 3))])
def test_mixed_split(B, wr, ws, want):
    assert LD.mixed_batch_split(B, wr, ws) == want


def test_sampler_weights_hand_case():
    # classes over all items: 0 twice, 1 twice -> class weight 1/2 each; an item's weight is the sum over its labels
    assert LD.sampler_weights([np.array([0, 0, 1]), np.array([1])]) == [1.5, 0.5]
    assert LD.sampler_weights([np.array([2.0]), np.array([2.0, 2.0, 7.0])]) == [1 / 3, 2 / 3 + 1.0]


# ---- 1b. index rules against fixtures recorded from the unmodified reference (tests/make_golden_loader.py) ----------------------------------
def _golden_store(name):
    c = cgl.SEQ_CASES[name]
    return SequenceStore(_host_packed(cgl.frames(name), cgl.SHAPE), np.asarray(c['o2r'], dtype=np.int64), cgl.label_rows(name)), cgl.frames(name)


def _assert_items(gold, prefix, samples, x):
    """The loader's host samples against the recorded items: windows as read back from the data, flags, label rows per step."""
    assert len(samples) == len(gold[prefix + '_first'])
    rows = []
    for k, s in enumerate(samples):
        ev = np.zeros((cgl.T,) + cgl.SHAPE, dtype=np.uint8)
        ev[s.windows >= 0] = x[s.windows[s.windows >= 0]]
        assert np.array_equal(cgl.windows_of(ev), gold[prefix + '_windows'][k]) and np.array_equal(s.windows, gold[prefix + '_windows'][k])
        assert s.is_first_sample == bool(gold[prefix + '_first'][k])
        assert np.array_equal(s.is_padded_mask, gold[prefix + '_padded'][k])
        assert [-1 if lab is None else lab.shape[0] for lab in s.labels] == gold[prefix + '_label_n'][k].tolist()
        rows += [lab for lab in s.labels if lab is not None]
    got = np.concatenate(rows) if rows else np.zeros((0, 7), dtype=np.float32)
    assert got.dtype == gold[prefix + '_rows'].dtype and np.array_equal(got, gold[prefix + '_rows'])


@pytest.mark.parametrize('name', list(cgl.SEQ_CASES))
def test_sequence_rules_vs_reference_golden(name):
    gold = load_golden(name)
    store, x = _golden_store(name)
    o2r = store.objframe_idx_2_repr_idx
    n = LD.random_access_len(o2r, cgl.T)
    for prefix, end in (('rnd', False), ('rnd_end', True)):
        _assert_items(gold, prefix, [LD.random_access_sample(store, 0, cgl.T, i, only_load_end_labels=end) for i in range(n)], x)
    chunks = LD.streaming_chunks(*LD.streaming_range(o2r, store.num_windows, cgl.T), cgl.T)
    _assert_items(gold, 'it', [LD.streaming_sample(store, 0, cgl.T, c, i) for i, c in enumerate(chunks)], x)
    ranges = LD.label_cluster_ranges(o2r, cgl.T)
    assert ranges == [tuple(r) for r in gold['guar_ranges'].tolist()]
    subs = [(k, i, c) for k, r in enumerate(ranges) for i, c in enumerate(LD.streaming_chunks(*r, cgl.T))]
    _assert_items(gold, 'guar', [LD.streaming_sample(store, 0, cgl.T, c, i) for _, i, c in subs], x)
    assert [k for k, _, _ in subs] == gold['guar_seq'].tolist()
    filler = LD.padded_sample(cgl.T)
    assert filler.is_first_sample == bool(gold['filler_first']) and np.array_equal(filler.is_padded_mask, gold['filler_padded'])


def test_sharding_vs_reference_golden():
    gold = load_golden('loader_sharding')
    lengths = cgl.SHARD_LENGTHS
    for w in cgl.SHARD_WORLDS:
        for r in range(w):
            mine = LD.assign_to_worker(lengths, w, r)
            assert mine == gold[f'assign_W{w}_R{r}'].tolist()
            for b in cgl.SHARD_BATCH_SIZES:
                want = gold[f'slots_W{w}_R{r}_B{b}']
                if want.size == 0:                                        # the reference's assertion fired
                    with pytest.raises(AssertionError, match="Each worker must at least get 'batch_size' number of datapipes"):
                        LD.assign_to_slots([lengths[p] for p in mine], b)
                    continue
                slots = LD.assign_to_slots([lengths[p] for p in mine], b)
                assert [[mine[i] for i in s] for s in slots] == [[p for p in row if p >= 0] for row in want.tolist()]


# ---- 2. epoch behaviour (host side only) -----------------------------------------------------------------------------------------------------
def test_random_epochs():
    ld = _loader(SM.RANDOM, Mode.TRAIN, B=3, seed=5)
    n = len(ld.items)
    assert n == 4 + 3 + 1                                             # offsets 1 (window 2 < T - 1), 2 (windows 1, 3) and 0
    seen = [(s.store, int(s.windows[-1])) for batch in ld._random_batches(3) for s in batch]
    assert len(seen) == 6 == len(set(seen))                            # every item at most once, drop_last drops the last two
    every = [(s.store, int(s.windows[-1])) for batch in _loader(SM.RANDOM, Mode.TRAIN, B=2, seed=5)._random_batches(2) for s in batch]
    assert len(every) == n == len(set(every))                          # every item once per epoch
    g = torch.Generator()
    g.manual_seed(5 + 0)
    order = torch.randperm(n, generator=g).tolist()
    halves = [_loader(SM.RANDOM, Mode.TRAIN, B=2, seed=5, rank=r, world_size=2).random_order() for r in range(2)]
    assert halves[0] == order[0::2] and halves[1] == order[1::2] and sorted(halves[0] + halves[1]) == list(range(n))
    ev = _loader(SM.RANDOM, Mode.VAL, B=4)
    got = [(s.store, int(s.windows[-1])) for batch in ev._random_batches(4) for s in batch]
    assert got == [(0, 4), (0, 5), (0, 8), (0, 11), (1, 20), (1, 22), (1, 40), (2, 6)][:8] and len(got) == 8
    w = _loader(SM.RANDOM, Mode.TRAIN, B=2, seed=1, weighted_sampling=True)
    assert w.weights.shape == (n,) and len(w.random_order()) == n
    ids = [np.concatenate([lab[:, 5] for lab in LD.random_access_sample(w.stores[k], k, T, i).labels if lab is not None]) for k, i in w.items]
    assert w.weights.tolist() == LD.sampler_weights(ids)


def test_stream_train_epoch():
    B = 3
    ld = _loader(SM.STREAM, Mode.TRAIN, B=B, augm_config=AUGM)
    assert ld.streams == [(0, 0, 12), (1, 0, 4), (1, 16, 23), (1, 36, 41), (2, 2, 7)]
    torch.manual_seed(3)
    perms = [torch.randperm(len(ld.streams)).tolist() for _ in range(B)]
    torch.manual_seed(3)
    calls = [dict(randomize=0, draw=0) for _ in range(B)]
    for b, aug in enumerate(ld.augm_str):
        def wrap(name, fn, b=b):
            def f(*a, **k):
                calls[b][name] += 1
                return fn(*a, **k)
            return f
        aug.randomize_augmentation = wrap('randomize', aug.randomize_augmentation)
        aug.draw = wrap('draw', aug.draw)
    batches = []
    for batch in ld._stream_batches(B):
        ld._states(SM.STREAM, batch)
        batches.append(batch)
    n_chunks = [len(c) for c in ld.stream_chunks]
    walked = []
    for b in range(B):
        seq = [(s.store, int(s.windows[0])) for batch in batches for s in [batch[b]] if s.new_sequence]
        want = [(ld.streams[p][0], ld.streams[p][1]) for p in perms[b]]
        assert seq == want[:len(seq)]                                  # the slot's own permutation, drawn first in slot order
        walked.append(seq)
        for batch in batches:
            assert batch[b].is_first_sample == batch[b].new_sequence == (int(batch[b].windows[0]) in [ld.streams[p][1] for p in range(len(ld.streams))
                                                                                                       if ld.streams[p][0] == batch[b].store])
        assert calls[b] == dict(randomize=len(seq), draw=len(batches))  # once per sub-sequence, once per chunk
    assert len(batches) == sum(n_chunks)                                # every slot walks all streams: the first exhausted slot ends the epoch
    first = [s.is_first_sample for batch in batches for s in batch]
    assert sum(first) == B * len(ld.streams)


def test_stream_eval_epoch():
    want = {(k, w) for k, (N, o2r) in STORES.items() for w in range(max(o2r[0] - T + 1, 0), N)}
    for world, B in ((1, 2), (3, 1), (1, 3)):
        seen = []
        for r in range(world):
            ld = _loader(SM.STREAM, Mode.VAL, B=B, rank=r, world_size=world)
            batches = list(ld._stream_batches(B))
            for b in range(B):
                col = [batch[b] for batch in batches]
                done = False
                for s in col:
                    if s.store is None:
                        done = True                                    # an exhausted slot: only fillers follow
                        assert s.is_padded_mask.all() and not s.is_first_sample
                        continue
                    assert not done
                    pad = s.is_padded_mask
                    assert not pad[0] and (np.diff(pad.astype(int)) >= 0).all()          # padding only at the tail of a chunk
                    if pad.any():
                        assert int(s.windows[~pad][-1]) == STORES[s.store][0] - 1        # ... of a sequence's last chunk
                    seen += [(s.store, int(w)) for w in s.windows[~pad]]
            assert any(s.store is not None for s in batches[-1])
        assert sorted(seen) == sorted(want) and len(seen) == len(want)   # every window exactly once over all ranks
    with pytest.raises(AssertionError, match="Each worker must at least get 'batch_size' number of datapipes"):
        list(_loader(SM.STREAM, Mode.VAL, B=2, rank=0, world_size=2)._stream_batches(2))


# ---- 3. batches --------------------------------------------------------------------------------------------------------------------------------
def _dense(xs, samples):
    out = np.zeros((T, len(samples)) + xs[0].shape[1:], dtype=np.uint8)
    for b, s in enumerate(samples):
        for t, w in enumerate(s.windows):
            if w >= 0:
                out[t, b] = xs[s.store][w]
    return out


def _epoch(ld, seed):
    torch.manual_seed(seed)
    out = []
    for batch in ld:
        d = batch['data']
        out.append(dict(ev=d[DataType.EV_REPR].cpu().clone(), first=d[DataType.IS_FIRST_SAMPLE].cpu().clone(),
                        pad=d[DataType.IS_PADDED_MASK].cpu().clone(), states=batch['states'], samples=batch['samples'],
                        labels=[[None if lab is None else lab.clone() for lab in sl.labels] for sl in d[DataType.OBJLABELS_SEQ]]))
    return out


def _same_epochs(a, b):
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert torch.equal(x['ev'], y['ev']) and torch.equal(x['first'], y['first']) and torch.equal(x['pad'], y['pad'])
        assert x['states'] == y['states']
        for lx, ly in zip(x['labels'], y['labels']):
            assert [(p is None) for p in lx] == [(q is None) for q in ly]
            assert all(torch.equal(p, q) for p, q in zip(lx, ly) if p is not None)


@pytest.mark.parametrize('mode,dataset_mode', [(SM.RANDOM, Mode.TRAIN), (SM.STREAM, Mode.TRAIN), (SM.STREAM, Mode.VAL)],
                         ids=['random_train', 'stream_train', 'stream_val'])
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'two_launches'])
def test_batches_equal_restatement(backend, mode, dataset_mode, fused):
    _, xs = _three()
    ld = _loader(mode, dataset_mode, dev=backend, B=2, augm_config=AUGM, seed=11, fused=fused)
    ep = _epoch(ld, 21)
    assert len(ep) >= 2
    modes = set()
    for e in ep:
        want = augment_ref.planes_ref(torch.from_numpy(_dense(xs, e['samples'])), e['states'])
        assert torch.equal(e['ev'], want)
        assert e['first'].tolist() == [s.is_first_sample for s in e['samples']]
        assert torch.equal(e['pad'], torch.from_numpy(np.stack([s.is_padded_mask for s in e['samples']], axis=1)))
        rows, count = A.pack_labels([[s.labels[t] for s in e['samples']] for t in range(T)], G=ld.G)
        ro, co, _ = augment_ref.labels_ref(rows, count, e['states'], SHAPE[1:])
        keep = A.labelled_frames(co, e['states'])
        for t in range(T):
            for b in range(2):
                lab = e['labels'][t][b]
                assert (lab is not None) == bool(keep[t, b])
                if lab is not None:
                    assert torch.equal(lab, ro[t, b, :int(co[t, b])])
        modes |= {(s.flip, s.mode) for s in e['states']}
    if dataset_mode == Mode.TRAIN:
        assert len(modes) > 1                                           # the draw did something
    else:
        assert modes == {(False, 0)}


@pytest.mark.parametrize('mode', [SM.RANDOM, SM.STREAM], ids=['random', 'stream'])
def test_routes_and_residencies_agree(backend, mode):
    base = _epoch(_loader(mode, Mode.TRAIN, dev=backend, augm_config=AUGM, seed=4, fused=True), 9)
    default = _loader(mode, Mode.TRAIN, dev=backend, augm_config=AUGM, seed=4)
    assert default.fused is False                                       # the measured default route (profiles/loader_bench.txt)
    _same_epochs(base, _epoch(default, 9))
    _same_epochs(base, _epoch(_loader(mode, Mode.TRAIN, dev=backend, augm_config=AUGM, seed=4, fused=False), 9))
    _same_epochs(base, _epoch(_loader(mode, Mode.TRAIN, dev=backend, augm_config=AUGM, seed=4, resident='host', fused=True), 9))
    _same_epochs(base, _epoch(_loader(mode, Mode.TRAIN, dev=backend, augm_config=AUGM, seed=4, resident='host', fused=False), 9))


def test_previous_batch_stays_intact(backend):
    ld = _loader(SM.STREAM, Mode.VAL, dev=backend, B=2)
    it = iter(ld)
    first = next(it)
    ev = first['data'][DataType.EV_REPR]
    keep, rows_keep = ev.clone(), first['device_labels'][0].clone()
    second = next(it)
    assert second['data'][DataType.EV_REPR].data_ptr() != ev.data_ptr()
    assert torch.equal(ev, keep) and torch.equal(first['device_labels'][0], rows_keep)
    assert not torch.equal(second['data'][DataType.EV_REPR], keep)


def test_mixed_batch_merges(backend):
    from rvt_amd.states import merge_mixed_batches
    ld = _loader(SM.MIXED, Mode.TRAIN, dev=backend, B=3, augm_config=AUGM, w_random=3, w_stream=1, seed=2)
    assert (ld.b_rnd, ld.b_str) == (2, 1)
    torch.manual_seed(5)
    batch = next(iter(ld))
    assert set(batch) == {SM.RANDOM, SM.STREAM}
    merged = merge_mixed_batches(batch)['data']
    assert len(merged[DataType.EV_REPR]) == T and tuple(merged[DataType.EV_REPR][0].shape) == (3,) + SHAPE
    assert torch.equal(merged[DataType.EV_REPR][1][:1], batch[SM.STREAM]['data'][DataType.EV_REPR][1])
    assert torch.equal(merged[DataType.EV_REPR][1][1:], batch[SM.RANDOM]['data'][DataType.EV_REPR][1])
    assert merged[DataType.IS_FIRST_SAMPLE].shape == (3,) and all(len(sl) == 3 for sl in merged[DataType.OBJLABELS_SEQ])
    with pytest.raises(ValueError, match='training mode'):
        _loader(SM.MIXED, Mode.VAL, dev=backend, B=3)


# ---- 4. the step on loader batches -----------------------------------------------------------------------------------------------------------
def _detect_fn(feats, labels):
    assert all(torch.is_tensor(lab) and lab.shape[1] == 7 for lab in labels)
    return {'loss': sum((s * 0.01) * (f.float() ** 2).mean() for s, f in feats.items())}


def _micro_stores():
    H, W = casegen.CASES['micro']['hw']
    r = np.random.default_rng(77)
    out = []
    for k, (N, o2r) in enumerate(((9, [2, 4, 7]), (3, [1]), (3, [2]))):          # 3, 1 and 1 chunks of T = 3
        x = (r.integers(0, 11, (N, 20, H, W)) * (r.random((N, 20, H, W)) < 0.2)).astype(np.uint8)
        rows = [np.array([[f, 10 + f, 8, 20, 15, f % 2, 1.0]], dtype=np.float32) for f in range(len(o2r))]
        out.append(SequenceStore(_host_packed(x, (20, H, W)), np.asarray(o2r, dtype=np.int64), rows))
    return out


def _states_of(mod, mode):
    return [(h.float().cpu().clone(), c.float().cpu().clone()) for h, c in mod.mode_2_rnn_states[mode].get_states(0)]


def test_step_on_loader_batches(backend):
    from tests.test_backbone import build_model
    Tm = casegen.CASES['micro']['T']
    stores = _micro_stores()
    model = build_model('micro', backend, torch.float32)
    kw = dict(device=backend, augm_config=AUGM, seed=3, fused=True)
    # RANDOM and MIXED training batches
    for mode, B in ((SM.RANDOM, 2), (SM.MIXED, 2)):
        mod = BackboneSequenceModule(model, _detect_fn)
        torch.manual_seed(1)
        batch = next(iter(BatchLoader(stores, B, Tm, mode, Mode.TRAIN, **kw)))
        out = mod.training_step(batch, 0)
        assert torch.isfinite(out['loss']) and float(out['loss'].detach()) > 0
        model.zero_grad()
        out['loss'].backward()
    # two consecutive STREAM training batches: the states carry over
    mod = BackboneSequenceModule(model, _detect_fn)
    torch.manual_seed(1)
    it = iter(BatchLoader(stores, 2, Tm, SM.STREAM, Mode.TRAIN, **kw))
    for k in range(2):
        out = mod.training_step(next(it), k)
        assert torch.isfinite(out['loss'])
    assert mod.mode_2_rnn_states[Mode.TRAIN].get_states(0) is not None
    # evaluation stream: slot 0 walks the long recording, slot 1 the two short ones, so batch 2 resets slot 1 only
    ld = BatchLoader(stores, 2, Tm, SM.STREAM, Mode.VAL, device=backend)
    it = iter(ld)
    b1, b2 = next(it), next(it)
    assert b1['data'][DataType.IS_FIRST_SAMPLE].tolist() == [True, True] and b2['data'][DataType.IS_FIRST_SAMPLE].tolist() == [False, True]
    b2 = {'worker_id': 0, 'data': {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b2['data'].items()}}
    mod = BackboneSequenceModule(model, _detect_fn)
    assert 'loss' in mod.validation_step(b1, 0)
    assert 'loss' in mod.validation_step(b2, 1)
    carried = _states_of(mod, Mode.VAL)
    fresh = BackboneSequenceModule(model, _detect_fn)
    fresh.validation_step(b2, 0)
    alone = _states_of(fresh, Mode.VAL)
    for (h, c), (fh, fc_) in zip(carried, alone):
        assert torch.allclose(h[1], fh[1], atol=1e-5) and torch.allclose(c[1], fc_[1], atol=1e-5)      # slot 1 was reset: as if from nothing
        assert not torch.allclose(c[0], fc_[0], atol=1e-5)                                          # slot 0 carried its state


# ---- 5. store I/O ------------------------------------------------------------------------------------------------------------------------------
def test_store_save_load_round_trip(tmp_path):
    store, _ = _store(1, *STORES[1], nrows={0: 3, 2: 0})
    store.save(tmp_path / 'rec')
    back = SequenceStore.load(tmp_path / 'rec')
    assert np.array_equal(back.objframe_idx_2_repr_idx, store.objframe_idx_2_repr_idx)
    assert np.array_equal(back.rows, store.rows) and np.array_equal(back.row_offset, store.row_offset)
    for k in ('masks', 'seg_offset', 'value_base', 'values'):
        assert torch.equal(getattr(back.frames, k), getattr(store.frames, k))
    assert back.frames.frame_shape == SHAPE and back.labels_at(1).shape == (3, 7) and back.labels_at(2) is None
    assert back.labels_at(20) is None                                   # an empty labelled frame reads as no labels


class _Frames:
    frameidx_2_repridx = np.array([1, 3, 20])

    def rows(self, f, downsample_by_2=False):
        return _rows(f, f + 1) * (0.5 if downsample_by_2 else 1.0)


def test_store_from_label_frames():
    x = _coded_frames(0, 25)
    s = SequenceStore.from_label_frames(_host_packed(x, SHAPE), _Frames())
    assert s.objframe_idx_2_repr_idx.tolist() == [1, 3, 20] and [s.frame_rows(f).shape[0] for f in range(3)] == [1, 2, 3]
    h = SequenceStore.from_label_frames(_host_packed(x, SHAPE), _Frames(), downsample_by_2=True)
    assert np.array_equal(h.frame_rows(2), _rows(2, 3) * 0.5)


def _labels_file(tmp_path, **override):
    store, _ = _store(0, *STORES[0])
    store.save(tmp_path / 'rec')
    arrs = dict(objframe_idx_2_repr_idx=store.objframe_idx_2_repr_idx, rows=store.rows, row_offset=store.row_offset)
    arrs.update(override)
    np.savez(tmp_path / 'rec' / 'labels.npz', **arrs)
    return tmp_path / 'rec'


def test_store_load_rejects_bad_label_files(tmp_path):
    with pytest.raises(ValueError, match='not increasing'):
        SequenceStore.load(_labels_file(tmp_path, objframe_idx_2_repr_idx=np.array([2, 5, 4, 8, 11])))
    with pytest.raises(ValueError, match='outside'):
        SequenceStore.load(_labels_file(tmp_path, objframe_idx_2_repr_idx=np.array([2, 4, 5, 8, 14])))
    with pytest.raises(ValueError, match=r'float32 \[n\]\[7\]'):
        SequenceStore.load(_labels_file(tmp_path, rows=np.zeros((7, 6), dtype=np.float32)))
    with pytest.raises(ValueError, match='row_offset'):
        SequenceStore.load(_labels_file(tmp_path, row_offset=np.array([0, 1, 3, 4, 6, 9])))
