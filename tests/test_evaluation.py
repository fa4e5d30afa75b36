"""Prophesee / COCO mAP evaluation on the device: rvt_amd.evaluation on the HIP kernels (emulator build on the CPU, gfx950 build
on the GPU) against fixtures recorded from the reference, against a numpy restatement, and against answers known by hand.

Fixtures (tests/golden/eval_*.npz, tests/make_golden_evaluation.py) come from the UNMODIFIED reference
`PropheseeEvaluator.evaluate_buffer`: its box filter, time windowing and COCO-dictionary conversion ran as shipped.  pycocotools is
not installed where they were recorded, so ONLY the COCOeval core behind the reference was a stand-in: tests/cocoeval_ref.py, a
plain numpy restatement of the published algorithm, installed as pycocotools at run time.  The known-answer tests do not depend on
that restatement.

Bars.  Integer results (per-image matched / ignored flags, npig, image count) are compared for exact equality.  Every precision
entry is one correctly rounded double quotient of small integers, so it is compared to 1e-12 absolute - five orders below the 1 / N
step of any real change; the six metrics, means of such entries, to 1e-9."""

import numpy as np
import pytest
import torch

from rvt_amd.evaluation import BBOX_DTYPE, METRICS, DetectionEvaluator, PropheseeEvaluator
from tests import casegen_evaluation as cg
from tests import cocoeval_ref as ref
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden

TABLE_ATOL, METRIC_ATOL = 1e-12, 1e-9


def _to(case, dev):
    return tuple(torch.from_numpy(case[k]).to(dev) for k in ('det', 'count', 'rows', 'lcount', 't_us'))


def _check_metrics(got, want, what=''):
    for k in METRICS:
        print(f'{what} {k}: got {got[k]!r} want {want[k]!r}')
    for k in METRICS:
        assert abs(got[k] - want[k]) <= METRIC_ATOL, f'{what} {k}: got {got[k]!r}, expected {want[k]!r}'


def _check_table(got, want, what=''):
    assert got.shape == want.shape and got.dtype == np.float64
    err = float(np.abs(got - want).max())
    print(f'{what} precision table: max abs err {err:.3e}')
    assert err <= TABLE_ATOL, f'{what}: precision differs by {err:.3e} at {np.unravel_index(np.abs(got - want).argmax(), got.shape)}'


def _check_records(ev, want, what=''):
    """Per image, category and area range: the records' matched / ignored bits equal the restatement's dtMatches != 0 / dtIgnore,
    the scores equal dtScores, and a (frame, category) the restatement does not evaluate has no record."""
    rec = ev.records()
    image_of_frame = {f: i for i, f in enumerate(want['image_frames'])}
    assert set(np.unique(rec['frame']).tolist()) <= set(image_of_frame), f'{what}: records of a frame that is not an image'
    seen = 0
    for f, i in image_of_frame.items():
        in_frame = rec['frame'] == f
        for k in range(ev.num_classes):
            sel = np.nonzero(in_frame & (rec['category'] == k))[0]
            e0 = want['per_image'].get((i, k, 0))
            n_want = 0 if e0 is None else len(e0['dtScores'])
            assert sel.size == n_want, f'{what} frame {f} category {k}: {sel.size} records, expected {n_want}'
            if n_want == 0:
                continue
            assert np.array_equal(rec['score'][sel], np.asarray(e0['dtScores'], dtype=np.float32))
            for a in range(4):
                e = want['per_image'][i, k, a]
                for t in range(10):
                    bit = 4 * t + a
                    assert np.array_equal((rec['matched'][sel] >> bit) & 1, (e['dtMatches'][t] != 0).astype(np.int64)), \
                        f'{what} frame {f} category {k} area {a} threshold {t}: matched flags differ'
                    assert np.array_equal((rec['ignored'][sel] >> bit) & 1, e['dtIgnore'][t].astype(np.int64)), \
                        f'{what} frame {f} category {k} area {a} threshold {t}: ignored flags differ'
            seen += n_want
    assert seen == rec['frame'].size


def _restate(case, dataset, ds2, K):
    frames = cg.to_frames(case)
    want = ref.evaluate_frames(frames, dataset, ds2, K)
    diag, side = ref.filter_constants(dataset, ds2)
    want['image_frames'] = [f for f, (gt, _, t) in enumerate(frames) if gt.shape[0] and ref._keep(gt[:, 2], gt[:, 3], t, diag, side).any()]
    assert len(want['image_frames']) == want['images']
    return want


def _check_against(ev, want, what=''):
    c = ev.counts()
    assert c['images'] == want['images'], f"{what}: {c['images']} images, expected {want['images']}"
    assert np.array_equal(c['npig'], want['npig']), f"{what}: npig {c['npig'].tolist()}, expected {want['npig'].tolist()}"
    _check_table(ev.precision_table(), want['precision'], what)
    got = ev.evaluate()
    _check_metrics(got, want['metrics'], what)
    return got


# ---- 1. fixtures from the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cg.CASES))
def test_restatement_matches_reference_golden(name):
    """Pins tests/cocoeval_ref.evaluate_frames (filter, image decision, zero-detection case on per-frame arrays) to what the
    unmodified reference evaluator recorded for the same frames (CPU only)."""
    c, gold = cg.CASES[name], load_golden(name)
    want = ref.evaluate_frames(cg.to_frames(cg.make_case(name)), c['dataset'], c['ds2'], c['K'])
    assert want['images'] == int(gold['images']) and np.array_equal(want['npig'], gold['npig'])
    assert np.array_equal(want['precision'], gold['precision'])
    assert np.array_equal(np.array([want['metrics'][k] for k in METRICS]), gold['metrics'])


def test_edges_fixture_holds_its_edges():
    """The 'edges' case really contains what it is there for."""
    c = cg.CASES['eval_edges']
    case = cg.make_case('eval_edges')
    frames = cg.to_frames(case)
    diag, side = ref.filter_constants(c['dataset'], c['ds2'])
    early = [f for f, fr in enumerate(frames) if fr[2] <= 500000]
    assert early and any(frames[f][0].shape[0] and frames[f][1].shape[0] for f in early)
    small = [f for f, (gt, dt, t) in enumerate(frames) if t > 500000 and gt.shape[0] and dt.shape[0]
             and not ref._keep(gt[:, 2], gt[:, 3], t, diag, side).any()]
    assert small, 'no frame whose every label is under the size limits while it holds detections'
    areas = np.concatenate([gt[:, 2] * gt[:, 3] for gt, _, _ in frames])
    assert (areas < 1024).any() and ((areas > 1024) & (areas < 9216)).any() and (areas > 9216).any()
    assert any(((dt[:, 5] == 0) & ref._keep(dt[:, 2], dt[:, 3], t, diag, side)).sum() > 100 for _, dt, t in frames)
    gcls = np.concatenate([gt[:, 4] for gt, _, _ in frames])
    dcls = np.concatenate([dt[:, 5] for _, dt, _ in frames])
    assert not (gcls == 2).any() and (dcls == 2).any() and (gcls == 1).any() and not (dcls == 1).any()
    scores = np.concatenate([dt[:, 4] for _, dt, _ in frames])
    assert np.unique(scores).size < scores.size                                            # exact ties across frames
    assert any(np.unique(dt[:, 4]).size < dt.shape[0] for _, dt, _ in frames)              # and within a frame
    assert any(np.unique(dt, axis=0).shape[0] < dt.shape[0] for _, dt, _ in frames)        # duplicated detections


@pytest.mark.parametrize('name', list(cg.CASES))
def test_evaluator_vs_reference_golden(backend, name):
    """The kernels against the reference's recorded results: image count and npig exactly, every precision entry to 1e-12, the
    six metrics to 1e-9; the per-image matched / ignored flags exactly against the restatement (pinned to the same fixture)."""
    dev = backend
    c, gold = cg.CASES[name], load_golden(name)
    case = cg.make_case(name)
    ev = DetectionEvaluator(c['dataset'], c['ds2'])
    assert ev.num_classes == c['K']
    ev.add_frames(*_to(case, dev))
    want = {'images': int(gold['images']), 'npig': gold['npig'], 'precision': gold['precision'],
            'metrics': dict(zip(METRICS, gold['metrics'].tolist()))}
    got = _check_against(ev, want, name)
    assert got['truncated_frames'] == 0 and ev.frames == c['F']
    _check_records(ev, _restate(case, c['dataset'], c['ds2'], c['K']), name)


@pytest.mark.parametrize('name', ['eval_gen1', 'eval_edges'])
def test_prophesee_surface_vs_reference_golden(backend, name):
    """The reference's surface, fed with the structured arrays the reference evaluator was fed with."""
    c, gold = cg.CASES[name], load_golden(name)
    labels, preds = cg.to_prophesee(cg.make_case(name))
    ev = PropheseeEvaluator(c['dataset'], c['ds2'])
    assert not ev.has_data()
    half = len(labels) // 2
    ev.add_labels(labels[:half])
    ev.add_predictions(preds[:half])
    ev.add_labels(labels[half:])
    ev.add_predictions(preds[half:])
    assert ev.has_data()
    got = ev.evaluate_buffer(img_height=c['hw'][0], img_width=c['hw'][1])
    assert set(got) == set(METRICS)
    _check_metrics(got, dict(zip(METRICS, gold['metrics'].tolist())), name)
    ev.reset_buffer()
    assert not ev.has_data()


# ---- 2. known answers, independent of the restatement ----------------------------------------------------------------------------
def _boxes(entries):
    """[(x, y, w, h, class, score)] -> BBOX_DTYPE array at t filled in by the caller."""
    a = np.zeros((len(entries),), dtype=BBOX_DTYPE)
    for i, (x, y, w, h, c, s) in enumerate(entries):
        a[i]['x'], a[i]['y'], a[i]['w'], a[i]['h'], a[i]['class_id'], a[i]['class_confidence'] = x, y, w, h, c, s
    return a


def _frame(t, gts, dts):
    lab, pred = _boxes([g + (1.0,) for g in gts]), _boxes(dts)
    lab['t'], pred['t'] = t, t
    return lab, pred


def _run_known(kind, dev, frames, dataset='gen1'):
    """frames: [(labels, predictions)] structured arrays -> the six metrics through either evaluator class."""
    if kind == 'prophesee':
        ev = PropheseeEvaluator(dataset, False)
        ev.add_labels([f[0] for f in frames])
        ev.add_predictions([f[1] for f in frames])
        return ev.evaluate_buffer(240, 304)
    F, G, D = len(frames), max(1, max(f[0].size for f in frames)), max(1, max(f[1].size for f in frames))
    det, rows = np.zeros((F, D, 7), np.float32), np.zeros((F, G, 7), np.float32)
    count, lcount, t_us = np.zeros(F, np.int32), np.full(F, -1, np.int32), np.zeros(F, np.int64)
    for j, (lab, pred) in enumerate(frames):
        t_us[j] = lab['t'][0] if lab.size else pred['t'][0]
        for c, n in enumerate(('t', 'x', 'y', 'w', 'h', 'class_id', 'class_confidence')):
            rows[j, :lab.size, c] = lab[n]
        det[j, :pred.size, 0], det[j, :pred.size, 1] = pred['x'], pred['y']
        det[j, :pred.size, 2], det[j, :pred.size, 3] = pred['x'] + pred['w'], pred['y'] + pred['h']     # small integers: exact
        det[j, :pred.size, 4], det[j, :pred.size, 5], det[j, :pred.size, 6] = 0.5, pred['class_confidence'], pred['class_id']
        count[j], lcount[j] = pred.size, lab.size if lab.size else -1
    ev = DetectionEvaluator(dataset, False)
    ev.add_frames(*(torch.from_numpy(a).to(dev) for a in (det, count, rows, lcount, t_us)))
    out = ev.evaluate()
    assert out.pop('truncated_frames') == 0
    return out


HIT = _frame(600000, [(10, 10, 40, 40, 0)], [(10, 10, 40, 40, 0, 0.8)])
KNOWN = {
    # the ground truth itself is detected: area 1600 is 'medium'; the other ranges have no ground truth
    'hit': ([HIT], dict(AP=1, AP_50=1, AP_75=1, AP_S=-1, AP_M=1, AP_L=-1)),
    # a miss at .9 in front of the hit at .8: precision 1 / 2 at every recall level
    'miss_then_hit': ([_frame(600000, [(10, 10, 40, 40, 0)], [(100, 100, 40, 40, 0, 0.9), (10, 10, 40, 40, 0, 0.8)])],
                      dict(AP=0.5, AP_50=0.5, AP_75=0.5, AP_S=-1, AP_M=0.5, AP_L=-1)),
    # IoU 31 / 50 = 0.62: a match at thresholds .5, .55, .6 only
    'iou_062': ([_frame(600000, [(0, 0, 50, 50, 0)], [(0, 0, 50, 31, 0, 0.9)])], dict(AP=0.3, AP_50=1, AP_75=0)),
    # a frame at t = 500000 holding only a false positive is filtered away as a whole
    'early_frame': ([HIT, _frame(500000, [(10, 10, 40, 40, 0)], [(100, 100, 40, 40, 0, 0.95)])],
                    dict(AP=1, AP_50=1, AP_75=1, AP_S=-1, AP_M=1, AP_L=-1)),
    # a frame whose only ground truth is 9 wide is not an image: its false positive does not count
    'small_gt_frame': ([HIT, _frame(700000, [(10, 10, 9, 40, 0)], [(100, 100, 40, 40, 0, 0.95)])],
                       dict(AP=1, AP_50=1, AP_75=1, AP_S=-1, AP_M=1, AP_L=-1)),
    'no_detections': ([_frame(600000, [(10, 10, 40, 40, 0)], [])], dict(AP=0, AP_50=0, AP_75=0, AP_S=0, AP_M=0, AP_L=0)),
    # the only detection is 5 x 5: the filter drops it, which is the zero-detection case
    'tiny_detection': ([_frame(600000, [(10, 10, 40, 40, 0)], [(10, 10, 5, 5, 0, 0.9)])],
                       dict(AP=0, AP_50=0, AP_75=0, AP_S=0, AP_M=0, AP_L=0)),
}


@pytest.mark.parametrize('kind', ['device', 'prophesee'])
@pytest.mark.parametrize('name', list(KNOWN))
def test_known_answers(backend, name, kind):
    """Answers worked out by hand (they differ from the round numbers only by the 2.2e-16 in the precision quotient), through
    both evaluator classes, to 1e-9."""
    frames, want = KNOWN[name]
    got = _run_known(kind, backend, frames)
    for k, v in want.items():
        print(f'{name} {kind} {k}: got {got[k]!r} want {v!r}')
    for k, v in want.items():
        assert abs(got[k] - v) <= METRIC_ATOL, f'{name} {k}: got {got[k]!r}, expected {v!r}'


# ---- 3. random cases beyond the fixtures --------------------------------------------------------------------------------------------
# (seed, dataset, downsample_by_2, K, F, G, max_det, overflow)
RANDOM = [
    (0, 'gen1', False, 2, 1, 4, 16, False), (1, 'gen4', False, 3, 200, 6, 24, False), (2, 'gen1', True, 1, 40, 1, 12, False),
    (3, 'gen4', True, 16, 30, 128, 40, False), (4, 'gen1', False, 2, 60, 5, 6, True), (5, 'gen4', True, 3, 50, 33, 200, False),
    (6, 'gen1', True, 2, 300, 3, 10, True),
]


@pytest.mark.parametrize('seed,dataset,ds2,K,F,G,max_det,overflow', RANDOM)
def test_random_cases_vs_restatement(backend, seed, dataset, ds2, K, F, G, max_det, overflow):
    """F = 1 and in the hundreds, G = 1 and at the cap, count > max_det (reported as truncated_frames; the rows that exist are
    scored), 1 / 2 / 3 / 16 classes, both cameras: everything the fixtures check, against the restatement."""
    dev = backend
    case = cg.random_case(100 + seed, dataset, ds2, K, F, G, max_det, edges=(seed % 2 == 1 and K >= 3), overflow=overflow)
    ev = DetectionEvaluator(dataset, ds2, num_classes=K)
    ev.add_frames(*_to(case, dev))
    want = _restate(case, dataset, ds2, K)
    got = _check_against(ev, want, f'seed {seed}')
    n_over = int((case['count'] > max_det).sum())
    assert got['truncated_frames'] == n_over and (n_over > 0) == overflow
    _check_records(ev, want, f'seed {seed}')


def test_split_calls_give_identical_tables(backend):
    """The same frames in one add_frames call or split over several (with different batch sizes): identical tables, bit for bit."""
    dev = backend
    name = 'eval_1mpx_ds2'
    c, case = cg.CASES[name], cg.make_case(name)
    whole = DetectionEvaluator(c['dataset'], c['ds2'])
    whole.add_frames(*_to(case, dev))
    split = DetectionEvaluator(c['dataset'], c['ds2'])
    cuts = [0, 1, 50, 51, 180, c['F']]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        split.add_frames(*_to({k: v[lo:hi] for k, v in case.items()}, dev))
    assert np.array_equal(whole.precision_table(), split.precision_table())
    assert whole.evaluate() == split.evaluate()
    assert all(np.array_equal(v, split.counts()[k]) for k, v in whole.counts().items())
    # reset() forgets everything: the next evaluation is that of the new frames alone
    split.reset()
    split.add_frames(*_to(case, dev))
    assert np.array_equal(whole.precision_table(), split.precision_table())


# ---- 4. surface and plumbing ------------------------------------------------------------------------------------------------------------
def test_prophesee_surface_edges(backend):
    ev = PropheseeEvaluator('gen1', False)
    assert (ev.LABELS, ev.PREDICTIONS) == ('lables', 'predictions')         # the reference's spelling
    with pytest.warns(UserWarning, match='Attempt to use prophesee evaluation buffer, but it is empty'):
        assert ev.evaluate_buffer(240, 304) is None
    lab, pred = _frame(600000, [(10, 10, 40, 40, 0), (60, 60, 40, 40, 0)], [(10, 10, 40, 40, 0, 0.8)])
    lab['t'][1] = 700000
    ev.add_labels([lab])
    ev.add_predictions([pred])
    with pytest.raises(NotImplementedError, match='distinct timestamps'):
        ev.evaluate_buffer(240, 304)
    with pytest.raises(AssertionError):
        PropheseeEvaluator('gen3', False)


def test_bad_shapes_and_caps_raise_before_any_launch(backend):
    dev = backend
    ev = DetectionEvaluator('gen1', False)
    ok = _to(cg.random_case(1, 'gen1', False, 2, 3, 4, 8), dev)
    with pytest.raises(ValueError, match=r'det must be \[F\]\[max_det\]\[7\]'):
        ev.add_frames(ok[0][:, :, :6], *ok[1:])
    with pytest.raises(ValueError, match='label_rows must be'):
        ev.add_frames(ok[0], ok[1], ok[2][:2], ok[3], ok[4])
    with pytest.raises(ValueError, match='count must be'):
        ev.add_frames(ok[0], ok[1].long(), *ok[2:])
    with pytest.raises(ValueError, match='t_us must be'):
        ev.add_frames(*ok[:4], ok[4].int())
    with pytest.raises(ValueError, match="dataset must be 'gen1' or 'gen4'"):
        DetectionEvaluator('gen3', False)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)     # noqa: E731
    with pytest.raises(RuntimeError, match='max_det=1025 outside the supported range'):
        ev.add_frames(z(1, 1025, 7), z(1, dt=torch.int32), z(1, 4, 7), z(1, dt=torch.int32), z(1, dt=torch.int64))
    with pytest.raises(RuntimeError, match='G=129 label rows outside the supported range'):
        ev.add_frames(z(1, 8, 7), z(1, dt=torch.int32), z(1, 129, 7), z(1, dt=torch.int32), z(1, dt=torch.int64))
    with pytest.raises(RuntimeError, match='num_classes=17 outside the supported range'):
        DetectionEvaluator('gen1', False, num_classes=17).add_frames(*ok)
    assert ev.frames == 0                                                     # nothing was added by the refused calls
    # the caps themselves are accepted: max_det 1024, G 128, 16 classes
    top = DetectionEvaluator('gen4', False, num_classes=16)
    top.add_frames(z(2, 1024, 7), z(2, dt=torch.int32), z(2, 128, 7), z(2, dt=torch.int32), z(2, dt=torch.int64))
    assert top.evaluate() == dict({k: 0.0 for k in METRICS}, truncated_frames=0)


def test_head_eval_then_postprocess_then_evaluate(backend):
    """Eval head -> postprocess_padded -> add_frames -> evaluate on the head_micro maps: runs end to end with no copy in between,
    and equals the restatement applied to the same detections."""
    from rvt_amd.postprocess import postprocess_padded
    from tests import casegen_head as cgh
    from tests.test_head import _build
    dev = backend
    m, _ = _build('head_micro', dev, torch.float32)
    m.eval()
    xs = [torch.from_numpy(a).to(dev) for a in cgh.make_inputs('head_micro')]
    with torch.no_grad():
        pred, _ = m(xs)
    nc = cgh.CASES['head_micro']['nc']
    B = pred.shape[0]
    det, count, _ = postprocess_padded(pred, nc, 0.001, 0.45, max_det=64)
    # labels: per image the first two detections that pass the Gen1 half-resolution filter, as they are (IoU 1 with themselves)
    d = det.cpu().numpy()
    rows, lcount = np.zeros((B, 2, 7), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        w, h = d[b, :, 2] - d[b, :, 0], d[b, :, 3] - d[b, :, 1]
        for g in np.nonzero((w >= 5) & (h >= 5) & (w * w + h * h >= 225))[0][:2]:
            rows[b, lcount[b]] = (600000, d[b, g, 0], d[b, g, 1], w[g], h[g], d[b, g, 6], 1.0)
            lcount[b] += 1
    assert lcount.max() > 0, 'no detection of head_micro passes the filter: the test checks nothing'
    t_us = np.full(B, 600000, np.int64)
    ev = DetectionEvaluator('gen1', True, num_classes=nc)
    ev.add_frames(det, count, torch.from_numpy(rows).to(dev), torch.from_numpy(lcount).to(dev), torch.from_numpy(t_us).to(dev))
    case = dict(det=d, count=count.cpu().numpy(), rows=rows, lcount=lcount, t_us=t_us)
    want = _restate(case, 'gen1', True, nc)
    assert want['images'] == int((lcount > 0).sum())
    got = _check_against(ev, want, 'head_micro')
    assert got['truncated_frames'] == int((case['count'] > 64).sum())
    _check_records(ev, want, 'head_micro')
    assert got['AP_50'] > 0 and ev.counts()['records'].sum() > 0


@pytest.mark.gpu
def test_add_frames_graph_capture():
    """add_frames allocates nothing once the store is reserved and never synchronises: reset + add_frames captures into a
    torch.cuda.graph and replays on new contents at the same addresses, giving the evaluation of the replayed batch."""
    dev = torch.device('cuda', 0)
    c = cg.CASES['eval_gen1']
    cases = [cg.random_case(s, c['dataset'], c['ds2'], c['K'], 64, c['G'], c['max_det']) for s in (21, 22, 23)]
    bufs = _to(cases[0], dev)
    ev = DetectionEvaluator(c['dataset'], c['ds2'])
    ev.add_frames(*bufs)                                                   # eager warm-up: store, counters and tables allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.reset()
        ev.add_frames(*bufs)
    for case in cases[1:]:
        for b, src in zip(bufs, _to(case, dev)):
            b.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        ev.invalidate()                                                    # the replay changed the store behind the host's back
        eager = DetectionEvaluator(c['dataset'], c['ds2'])
        eager.add_frames(*_to(case, dev))
        assert eager.counts()['images'] > 0
        assert np.array_equal(ev.precision_table(), eager.precision_table())
        assert ev.evaluate() == eager.evaluate()
