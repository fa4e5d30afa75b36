"""Raw recordings on the host side (rvt_amd/recordings.py): the DAT header, the label filters, the labelled frames with their window
ends, and the per-frame rows, against fixtures recorded from the unmodified reference (tests/make_golden_recordings.py).
Integers are compared exactly, the float32 rows with ==."""
import os

import numpy as np
import pytest
import torch

from rvt_amd import _lib, augment
from rvt_amd.evaluation import BBOX_DTYPE
from rvt_amd.recordings import DatHeader, LabelFrames, NoLabels, Recording, filter_labels, frame_labels, read_dat_header
from rvt_amd.representations import EventSequenceBuilder
from tests.backends import emu_library
from tests.casegen_recordings import DAT_CASES, HW, LABEL_CASES

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FRAMED = [n for n in LABEL_CASES if n != 'all_filtered']


def gold(kind, name):
    return np.load(os.path.join(GOLD, f'rec_{kind}_{name}.npz'))


def framed(name):
    c, g = LABEL_CASES[name], gold('labels', name)
    lab = filter_labels(g['inp'], c['dataset'], c['split'], c['psee'], c['faulty'])
    return c, g, frame_labels(lab, c['dataset'], c['align_t_ms'], c['step_ms'])


@pytest.mark.parametrize('name', list(DAT_CASES))
def test_read_dat_header(tmp_path, name):
    g = gold('dat', name)
    path = tmp_path / f'{name}_td.dat'
    g['raw'].tofile(path)
    hdr = read_dat_header(path)
    off, ev_type, ev_size, height, width = (int(v) for v in g['header'])
    assert hdr == DatHeader(off, ev_type, ev_size, None if height < 0 else height, None if width < 0 else width)
    assert (g['raw'].size - hdr.offset) == 8 * g['t'].size


def test_read_dat_header_refuses_other_events(tmp_path):
    path = tmp_path / 'cd.dat'
    path.write_bytes(b'% Data file containing CD events.\n% Version 2\n' + bytes([12, 8]) + bytes(16))
    with pytest.raises(ValueError, match='type 12 with 8-byte'):
        read_dat_header(path)
    path.write_bytes(b'% Version 2\n' + bytes([0, 16]) + bytes(16))
    with pytest.raises(ValueError, match='type 0 with 16-byte'):
        read_dat_header(path)


@pytest.mark.parametrize('name', list(LABEL_CASES))
def test_filter_labels(name):
    c, g = LABEL_CASES[name], gold('labels', name)
    inp = g['inp']
    assert inp.dtype.names == BBOX_DTYPE.names
    before = inp.copy()
    got = filter_labels(inp, c['dataset'], c['split'], c['psee'], c['faulty'])
    assert np.array_equal(inp, before)                   # the caller's array is not modified (the reference crops in place)
    if name == 'all_filtered':
        assert got.size == 0 and got.dtype == BBOX_DTYPE
        with pytest.raises(NoLabels):
            frame_labels(got, c['dataset'], c['align_t_ms'], c['step_ms'])
        return
    want = g['filtered']
    assert got.dtype == BBOX_DTYPE and got.shape == want.shape
    for k in BBOX_DTYPE.names:
        assert np.array_equal(got[k], want[k]), k
    assert 0 < got.size < inp.size                       # every case loses some boxes and keeps some


@pytest.mark.parametrize('name', FRAMED)
def test_frame_labels(name):
    c, g, fr = framed(name)
    assert isinstance(fr, LabelFrames) and len(fr) == g['frame_ts_us'].size
    for k in ('objframe_idx_2_label_idx', 'frame_ts_us', 'ev_repr_ts_end_us', 'frameidx_2_repridx'):
        got = getattr(fr, k)
        assert got.dtype == np.int64 and np.array_equal(got, g[k]), k
    assert fr.labels.dtype == BBOX_DTYPE and fr.labels.shape == g['labels'].shape
    for k in BBOX_DTYPE.names:
        assert np.array_equal(fr.labels[k], g['labels'][k]), k
    assert np.array_equal(fr.ev_repr_ts_end_us[fr.frameidx_2_repridx], fr.frame_ts_us)


def test_fixture_cases_are_what_they_claim():
    """One surviving frame; a label time refused by the jitter gate; labels in front of align_t_ms; classes 3-6 and boxes
    hanging out of the frame in the 1 Mpx cases."""
    g = gold('labels', 'single_frame')
    assert g['frame_ts_us'].size == 1 and np.unique(g['filtered']['t']).size == 2 and g['ev_repr_ts_end_us'][-1] == g['frame_ts_us'][0]
    g = gold('labels', 'gen1_val_jitter')
    assert np.unique(g['filtered']['t']).size == g['frame_ts_us'].size + 2
    g = gold('labels', 'align_late')
    assert g['filtered']['t'].min() < 600_000 <= g['frame_ts_us'][0]
    for name in ('gen4_60hz', 'gen4_30hz'):
        g = gold('labels', name)
        H, W = HW['gen4']
        assert set(np.unique(g['inp']['class_id'])) == set(range(7)) and g['filtered']['class_id'].max() <= 2
        assert (g['inp']['x'] < 0).any() and (g['inp']['x'] + g['inp']['w'] > W).any() and (g['inp']['y'] + g['inp']['h'] > H).any()
    assert 'no_labels' in gold('labels', 'all_filtered').files


@pytest.mark.parametrize('name', FRAMED)
def test_rows(name):
    c, g, fr = framed(name)
    for key, ds in (('full', False), ('half', True)):
        want, off = g[f'rows_{key}'], g[f'rows_{key}_off']
        assert want.dtype == np.float32 and off.size == len(fr) + 1
        for f in range(len(fr)):
            got = fr.rows(f, downsample_by_2=ds)
            assert got.dtype == np.float32 and got.shape == (off[f + 1] - off[f], 7)
            assert (got == want[off[f]:off[f + 1]]).all(), (key, f)
    H, W = HW[c['dataset']]
    half = g['rows_half']
    assert (half[:, 1] + half[:, 3] <= 0.5 * W - 1).all() and (half[:, 2] + half[:, 4] <= 0.5 * H - 1).all()
    with pytest.raises(IndexError):
        fr.rows(len(fr))


def test_window_rows_go_through_pack_labels():
    """Two recordings side by side: window_rows per sample -> labels_seq[t][b] -> pack_labels."""
    T = 6
    frs = [framed('gen1_train')[2], framed('align_late')[2]]
    first = [int(fr.frameidx_2_repridx[0]) - 1 for fr in frs]
    per_sample = [fr.window_rows(f0, T, downsample_by_2=False) for fr, f0 in zip(frs, first)]
    assert all(len(w) == T for w in per_sample)
    labels_seq = [[per_sample[b][t] for b in range(2)] for t in range(T)]
    rows, count = augment.pack_labels(labels_seq)
    assert tuple(rows.shape[:2]) == (T, 2) and rows.shape[-1] == 7 and count.dtype == torch.int32
    for b, (fr, f0) in enumerate(zip(frs, first)):
        on_frame = {int(r) - f0: f for f, r in enumerate(fr.frameidx_2_repridx)}
        for t in range(T):
            if t in on_frame:
                want = fr.rows(on_frame[t])
                assert int(count[t, b]) == want.shape[0] and np.array_equal(rows[t, b, :want.shape[0]].numpy(), want)
            else:
                assert per_sample[b][t] is None and int(count[t, b]) == -1
        assert sum(w is not None for w in per_sample[b]) >= 2


def test_recording_feeds_the_builder(tmp_path):
    """A recording on disk -> decoded, repaired events + window ends + rows; the builder (emulator) slices the repaired stream."""
    name, lname = 'windows', 'gen1_train'
    g, gl = gold('dat', name), gold('labels', lname)
    dat, bbox = tmp_path / 'rec_td.dat', tmp_path / 'rec_bbox.npy'
    g['raw'].tofile(dat)
    np.save(bbox, gl['inp'])
    c = LABEL_CASES[lname]
    step_us = 1000 * c['step_ms']
    _lib._install_test_library(emu_library())
    try:
        rec = Recording(dat, bbox, c['dataset'], c['split'], apply_psee_bbox_filter=c['psee'], apply_faulty_bbox_filter=c['faulty'],
                        align_t_ms=c['align_t_ms'], ts_step_ev_repr_ms=c['step_ms'], device=torch.device('cpu'))
        assert rec.header.height == 240 and rec.header.width == 304 and rec._decoder is None       # lazy on the events
        assert np.array_equal(rec.frames.ev_repr_ts_end_us, gl['ev_repr_ts_end_us'])
        T = 7
        ends = rec.window_ends(0, T)
        assert ends.dtype == torch.int64 and np.array_equal(ends.numpy(), gl['ev_repr_ts_end_us'][:T])
        with pytest.raises(IndexError):
            rec.window_ends(0, 10_000)
        table = rec.table(ends)                          # the recording's own window ends go to the builder
        assert table.T == T and table.ts_end is ends
        n = g['t'].size
        x, y, p, t = (a.numpy() for a in table.streams[0])
        assert np.array_equal(t[:n], g['t_repaired']) and np.array_equal(x[:n], g['x']) and np.array_equal(p[:n], g['p'])
        H, W = rec.height, rec.width
        eb = EventSequenceBuilder(4, H, W, count_cutoff=10, window_us=step_us)
        planes, bounds = eb.build_from_table(table)
        want_end = np.searchsorted(g['t_repaired'], ends.numpy(), side='right')
        want_start = np.searchsorted(g['t_repaired'], ends.numpy() - step_us, side='left')
        assert np.array_equal(bounds[0, :, 0].numpy(), want_start) and np.array_equal(bounds[0, :, 1].numpy(), want_end)
        assert int(((want_end - want_start) > 100).sum()) >= 5                    # the recording's clock covers most of these windows
        streams = [tuple(torch.from_numpy(g[k].copy()) for k in 'xyp') + (torch.from_numpy(g['t_repaired'].copy()),)]
        want, _ = EventSequenceBuilder(4, H, W, count_cutoff=10, window_us=step_us).build(streams, ends)
        assert torch.equal(planes, want) and all(int(planes[w].sum()) > 0 for w in range(5))
        assert (g['t'] != g['t_repaired']).any()                                  # and it steps back: the decode repaired it
        assert rec.table() is table                                               # decoded once
        rows = rec.window_rows(int(rec.frames.frameidx_2_repridx[0]), 1)
        assert np.array_equal(rows[0], gl['rows_full'][:gl['rows_full_off'][1]])
    finally:
        _lib._install_test_library(None)
    np.save(bbox, gold('labels', 'all_filtered')['inp'])
    with pytest.raises(NoLabels):
        Recording(dat, bbox, 'gen4', 'train')


def test_rows_that_go_flat_at_half_scale():
    """Boxes 0.8 px wide at the right and bottom edge (the label factory alone: no filter lets them through) have an area at full
    size and none at half scale; a frame that loses all its boxes is None in window_rows."""
    g = np.load(os.path.join(GOLD, 'rec_rows_edge.npz'))
    ts = np.unique(g['labels']['t']).astype(np.int64)
    fr = LabelFrames(g['labels'], g['objframe_idx_2_label_idx'], ts, ts, np.arange(ts.size, dtype=np.int64), 'gen4')
    for key, ds in (('full', False), ('half', True)):
        want, off = g[f'rows_{key}'], g[f'rows_{key}_off']
        for f in range(len(fr)):
            got = fr.rows(f, downsample_by_2=ds)
            assert got.shape == (off[f + 1] - off[f], 7) and (got == want[off[f]:off[f + 1]]).all(), (key, f)
    assert g['rows_full'].shape[0] == 4 and g['rows_half_off'].tolist() == [0, 1, 1]
    full, half = fr.window_rows(0, 2, downsample_by_2=False), fr.window_rows(0, 2, downsample_by_2=True)
    assert [r.shape[0] for r in full] == [3, 1] and half[0].shape[0] == 1 and half[1] is None
