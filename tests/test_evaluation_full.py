"""Recall table, full COCO summary, merge and all_gather of rvt_amd.evaluation.DetectionEvaluator (rvt_coco_recall on the emulator
build on the CPU and on the gfx950 build on the GPU).

Yardsticks.  tests/cocoeval_full_ref.py adds the published recall accumulation and the twelve-number summarize to the restatement
tests/test_evaluation.py already pins to the reference; tests/golden/evalfull_*.npz (tests/make_golden_evaluation_full.py) were
recorded from the UNMODIFIED reference evaluator with that class standing in for pycocotools.

Bars.  A recall cell is ONE double division of two integers on both sides, so recall_table() is compared for exact equality; the
twelve numbers of summary() are means of such cells and take the bar tests/test_evaluation.py sets for the six (METRIC_ATOL,
imported from there).  merge() and all_gather() promise the bits of a single evaluator: exact equality throughout."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rvt_amd import _lib as L
from rvt_amd.evaluation import METRICS, SUMMARY_KEYS, DetectionEvaluator
from tests import casegen_evaluation as cg
from tests import casegen_evaluation_full as cgf
from tests import cocoeval_full_ref as full
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden
from tests.test_evaluation import METRIC_ATOL, RANDOM, _to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _restated(name):
    c = cgf.CASES[name]
    return full.evaluate_frames(cg.to_frames(cgf.make_case(name)), c['dataset'], c['ds2'], c['K'])


@functools.lru_cache(maxsize=None)
def _random(seed, dataset, ds2, K, F, G, max_det, overflow):
    case = cg.random_case(100 + seed, dataset, ds2, K, F, G, max_det, edges=(seed % 2 == 1 and K >= 3), overflow=overflow)
    return case, full.evaluate_frames(cg.to_frames(case), dataset, ds2, K)


def _per_class(precision, recall):
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    return [{'AP': mean(precision[:, :, k, 0]), 'AP_50': mean(precision[0, :, k, 0]), 'AR_100': mean(recall[:, k, 0, 2])}
            for k in range(precision.shape[2])]


def _check_summary(got, want, what=''):
    assert list(got)[:12] == list(full.STAT_KEYS) == list(SUMMARY_KEYS) and set(got) == set(SUMMARY_KEYS) | {'per_class', 'truncated_frames'}
    for k in SUMMARY_KEYS:
        print(f'{what} {k}: got {got[k]!r} want {want[k]!r}')
    for k in SUMMARY_KEYS:
        assert abs(got[k] - want[k]) <= METRIC_ATOL, f'{what} {k}: got {got[k]!r}, expected {want[k]!r}'


def _check_full(ev, want, what=''):
    """Recall exactly, the twelve numbers and the per-class numbers to METRIC_ATOL, against a restatement result."""
    got = ev.recall_table()
    assert got.shape == want['recall'].shape and got.dtype == np.float64
    print(f'{what} recall table: {int((got != want["recall"]).sum())} cells differ')
    assert np.array_equal(got, want['recall']), f'{what}: recall differs at {np.argwhere(got != want["recall"])[:4].tolist()}'
    s = ev.summary()
    _check_summary(s, want['stats'], what)
    assert {k: s[k] for k in METRICS} == {k: v for k, v in ev.evaluate().items() if k != 'truncated_frames'}
    if any(v != 0.0 for v in want['stats'].values()):                         # (all zero: no detection survived, nothing per class)
        for k, (g, w) in enumerate(zip(s['per_class'], _per_class(want['precision'], want['recall']))):
            assert set(g) == {'AP', 'AP_50', 'AR_100'}
            for key in g:
                assert abs(g[key] - w[key]) <= METRIC_ATOL, f'{what} class {k} {key}: got {g[key]!r}, expected {w[key]!r}'
    return s


# ---- 1. the yardstick against what is already recorded --------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cg.CASES))
def test_full_restatement_precision_is_the_recorded_one(name):
    """COCOevalFull leaves the parent's precision alone: its table at maxDets 100 equals the one stored in the existing fixture
    (recorded from the reference), exactly, and so do its first six stats (CPU only; passes without the feature by design)."""
    gold, want = load_golden(name), _restated(name)
    assert np.array_equal(want['precision'], gold['precision'])
    assert np.array_equal(np.array([want['stats'][k] for k in METRICS]), gold['metrics'])


@pytest.mark.parametrize('name', list(cgf.CASES))
def test_full_restatement_matches_reference_golden(name):
    """Pins cocoeval_full_ref.evaluate_frames (per-frame arrays) to what the unmodified reference evaluator recorded (CPU only)."""
    gold, want = load_golden(cgf.golden_name(name)), _restated(name)
    assert want['images'] == int(gold['images']) and np.array_equal(want['npig'], gold['npig'])
    assert np.array_equal(want['recall'], gold['recall'])
    assert np.array_equal(np.array([want['stats'][k] for k in full.STAT_KEYS]), gold['stats'])


def test_ranks_fixture_holds_its_properties():
    """'eval_ranks' really contains what it is there for, in its inputs, in the restatement and in the recorded fixture."""
    want = _restated('eval_ranks')
    cgf.ranks_properties(cgf.ranks_case(), want)
    gold = load_golden(cgf.golden_name('eval_ranks'))
    s = dict(zip(full.STAT_KEYS, gold['stats'].tolist()))
    assert s['AR_1'] < s['AR_10'] < s['AR_100'] and int(gold['images']) == 4
    assert (gold['recall'][:, 2] == -1).all() and (gold['npig'][2] == 0).all()
    assert (gold['recall'][:, 0, 0, 0] < gold['recall'][:, 0, 0, 1]).all() and (gold['recall'][:, 0, 0, 1] < gold['recall'][:, 0, 0, 2]).all()
    assert np.unique(gold['recall'][:, 0, 0, 2]).size > 1                     # a match that some thresholds accept and others do not


# ---- 2. the device against fixtures and restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cgf.CASES))
def test_recall_and_summary_vs_reference_golden(backend, name):
    """recall_table() equals the reference's recorded recall exactly; summary()'s twelve numbers meet METRIC_ATOL."""
    dev = backend
    c, gold = cgf.CASES[name], load_golden(cgf.golden_name(name))
    ev = DetectionEvaluator(c['dataset'], c['ds2'])
    ev.add_frames(*_to(cgf.make_case(name), dev))
    got = ev.recall_table()
    assert got.shape == (10, c['K'], 4, 3) and got.dtype == np.float64
    print(f'{name} recall table: {int((got != gold["recall"]).sum())} of {got.size} cells differ')
    assert np.array_equal(got, gold['recall'])
    s = ev.summary()
    _check_summary(s, dict(zip(full.STAT_KEYS, gold['stats'].tolist())), name)
    assert s['truncated_frames'] == int((cgf.make_case(name)['count'] > c['max_det']).sum())
    assert len(s['per_class']) == c['K']
    _check_full(ev, _restated(name), name)
    if name == 'eval_ranks':
        assert s['AR_1'] < s['AR_10'] < s['AR_100'] and s['truncated_frames'] == 1
        assert s['per_class'][2] == {'AP': -1.0, 'AP_50': -1.0, 'AR_100': -1.0}


@pytest.mark.parametrize('split', [False, True], ids=['one_call', 'two_strides'])
@pytest.mark.parametrize('seed,dataset,ds2,K,F,G,max_det,overflow', RANDOM)
def test_random_cases_vs_full_restatement(backend, seed, dataset, ds2, K, F, G, max_det, overflow, split):
    """The shapes of tests/test_evaluation.py's RANDOM list against the restatement; `two_strides` adds the second half of the
    frames with seven more (empty) detection rows per frame, so that two record strides sit in one store."""
    dev = backend
    case, want = _random(seed, dataset, ds2, K, F, G, max_det, overflow)
    ev = DetectionEvaluator(dataset, ds2, num_classes=K)
    n_over = int((case['count'] > max_det).sum())
    if split and F > 1:
        cut = F // 2
        ev.add_frames(*_to({k: v[:cut] for k, v in case.items()}, dev))
        rest = {k: v[cut:] for k, v in case.items()}
        rest['det'] = np.concatenate([rest['det'], np.zeros((F - cut, 7, 7), np.float32)], axis=1)
        rest['count'] = np.minimum(rest['count'], max_det)                    # the rows that exist, as the first half scores them
        ev.add_frames(*_to(rest, dev))
        assert len({R for _, _, R in ev._spans}) == 2
        n_over = int((case['count'][:cut] > max_det).sum())
    else:
        ev.add_frames(*_to(case, dev))
    assert np.array_equal(ev.precision_table(), want['precision'])
    s = _check_full(ev, want, f'seed {seed}')
    assert s['truncated_frames'] == n_over


# ---- 3. kernel contract ---------------------------------------------------------------------------------------------------------
def test_tp_table_repeats_and_ignores_the_batching(backend):
    """The integer table is the same on every run, with the frames added in one call or one per call, and over more rows than a
    launch has waves (1080 rows in one run of spans: every wave walks two rows): 18 times the table of the 60 frames."""
    dev = backend
    case = cg.random_case(104, 'gen1', False, 2, 60, 5, 6, overflow=True)
    one = DetectionEvaluator('gen1', False)
    one.add_frames(*_to(case, dev))
    tp = one.recall_counts().copy()
    assert tp.shape == (3, 2, 10, 4) and tp.dtype == np.int64 and tp[2].sum() > 0
    assert (tp[0] <= tp[1]).all() and (tp[1] <= tp[2]).all() and (tp[0] < tp[2]).any()
    for _ in range(2):
        one.invalidate()
        assert np.array_equal(one.recall_counts(), tp)
        assert np.array_equal(one._recall_tp().cpu().numpy().reshape(3, 2, 10, 4), tp)
    each = DetectionEvaluator('gen1', False)
    for f in range(60):
        each.add_frames(*_to({k: v[f:f + 1] for k, v in case.items()}, dev))
    assert np.array_equal(each.recall_counts(), tp) and np.array_equal(each.recall_table(), one.recall_table())
    many = DetectionEvaluator('gen1', False)
    bufs = _to(case, dev)
    for _ in range(18):
        many.add_frames(*bufs)
    assert many.frames == 1080 and np.array_equal(many.recall_counts(), 18 * tp)
    assert np.array_equal(many.recall_table(), one.recall_table())           # tp and npig both 18-fold: the same quotients


def test_recall_unsupported_shapes_refused_before_any_launch(backend):
    dev = backend
    planes = torch.full((3, 2 * 1025), 0x7fffffffffffffff, dtype=torch.int64, device=dev)
    tp = torch.zeros(3, 16, 40, dtype=torch.int64, device=dev)

    def run(F, R, K):
        L.call('rvt_coco_recall', L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]), F, R, K, L.ptr(tp), L.stream_of(tp))
    for F, R, K, says in ((2, 0, 3, 'rec_stride=0 outside the supported range 1..1024'), (2, 1025, 3, 'rec_stride=1025 outside'),
                          (2, 8, 0, 'num_classes=0 outside the supported range 1..16'), (2, 8, 17, 'num_classes=17 outside'),
                          (0, 8, 3, 'F=0 frames')):
        with pytest.raises(RuntimeError, match=says):
            run(F, R, K)
    run(2, 1024, 16)                                                          # the caps themselves are accepted
    run(1, 1, 1)
    assert int(tp.abs().sum()) == 0                                           # unused slots only: nothing counted


def test_summary_before_any_frame_raises(backend):
    ev = DetectionEvaluator('gen1', False)
    for fn in (ev.summary, ev.recall_table, ev.recall_counts, ev.evaluate):
        with pytest.raises(RuntimeError, match='before any add_frames'):
            fn()


def test_summary_is_zero_without_detections(backend):
    """No detection survives in any image: all twelve are 0.0, the rule evaluate() applies to its six."""
    dev = backend
    case = cgf.ranks_case()
    case['count'][:] = 0
    ev = DetectionEvaluator('gen4', True)
    ev.add_frames(*_to(case, dev))
    s = ev.summary()
    assert all(s[k] == 0.0 for k in SUMMARY_KEYS) and s['per_class'] == [{'AP': 0.0, 'AP_50': 0.0, 'AR_100': 0.0}] * 3
    assert (ev.recall_table()[:, :2, 0] == 0.0).all() and (ev.recall_table()[:, 2] == -1.0).all()


# ---- 4. merge -------------------------------------------------------------------------------------------------------------------
def _same_results(a, b):
    assert np.array_equal(a.precision_table(), b.precision_table()) and np.array_equal(a.recall_table(), b.recall_table())
    ca, cb = a.counts(), b.counts()
    assert set(ca) == set(cb) and all(np.array_equal(v, cb[k]) for k, v in ca.items())
    assert a.summary() == b.summary() and a.evaluate() == b.evaluate()
    assert a.frames == b.frames and a.slots == b.slots


def test_merge_equals_one_evaluator_at_every_split(backend):
    """A's frames then B's: after A.merge(B) every table, counter and number has the bits of one evaluator fed all frames in
    order, for every split 0..F (empty halves included); frames 1 and 4 tie exactly, so the arrival order shows."""
    dev = backend
    c, case = cgf.RANKS, cgf.ranks_case()
    whole = DetectionEvaluator(c['dataset'], c['ds2'])
    whole.add_frames(*_to(case, dev))
    for cut in range(c['F'] + 1):
        a, b = DetectionEvaluator(c['dataset'], c['ds2']), DetectionEvaluator(c['dataset'], c['ds2'])
        if cut > 0:
            a.add_frames(*_to({k: v[:cut] for k, v in case.items()}, dev))
        if cut < c['F']:
            b.add_frames(*_to({k: v[cut:] for k, v in case.items()}, dev))
        b_slots = b.slots
        a.merge(b)
        _same_results(a, whole)
        assert b.slots == b_slots and b.frames == c['F'] - cut               # the other evaluator is left as it was
    # the swapped order is another evaluation: the tie goes the other way
    a, b = DetectionEvaluator(c['dataset'], c['ds2']), DetectionEvaluator(c['dataset'], c['ds2'])
    a.add_frames(*_to({k: v[:3] for k, v in case.items()}, dev))
    b.add_frames(*_to({k: v[3:] for k, v in case.items()}, dev))
    b.merge(a)
    assert np.array_equal(b.recall_table(), whole.recall_table()) and not np.array_equal(b.precision_table(), whole.precision_table())


def test_merge_refuses_mismatches_and_leaves_the_store_alone(backend):
    dev = backend
    c, case = cgf.RANKS, cgf.ranks_case()
    a = DetectionEvaluator(c['dataset'], c['ds2'])
    a.add_frames(*_to(case, dev))
    before = (a.slots, a.frames, list(a._spans), a._planes[:, :a.slots].clone(), a._counters.clone(), a.summary())
    others = [DetectionEvaluator(c['dataset'], c['ds2'], num_classes=2), DetectionEvaluator('gen1', c['ds2'], num_classes=3),
              DetectionEvaluator(c['dataset'], not c['ds2'])]
    for o, says in zip(others, ('num_classes differs', 'dataset differs', 'downsample_by_2 differs')):
        if o.num_classes == 3:
            o.add_frames(*_to(case, dev))
        with pytest.raises(ValueError, match=says):
            a.merge(o)
    with pytest.raises(ValueError, match='itself'):
        a.merge(a)
    with pytest.raises(ValueError, match='takes a DetectionEvaluator'):
        a.merge(None)
    assert (a.slots, a.frames, a._spans) == before[:3] and torch.equal(a._planes[:, :a.slots], before[3])
    assert torch.equal(a._counters, before[4]) and a.summary() == before[5]


# ---- 5. all_gather, world 2 over gloo -------------------------------------------------------------------------------------------
def _digest(ev):
    s = ev.summary()
    h = hashlib.sha256()
    h.update(ev.precision_table().tobytes())
    h.update(ev.recall_table().tobytes())
    h.update(np.array([s[k] for k in SUMMARY_KEYS] + [v for pc in s['per_class'] for v in pc.values()], dtype=np.float64).tobytes())
    h.update(np.array([s['truncated_frames'], ev.frames, ev.slots], dtype=np.int64).tobytes())
    return h.hexdigest()


GATHER_CUT = 11
GATHER_WORKER = r'''
import os, sys, torch, torch.distributed as dist
root, out_dir = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from rvt_amd import _lib
from rvt_amd.evaluation import DetectionEvaluator
from tests.backends import emu_library
from tests.test_evaluation import _to
from tests.test_evaluation_full import GATHER_CUT, _digest, _gather_case
_lib._install_test_library(emu_library())
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
dist.init_process_group('gloo')
torch.set_num_threads(2)
(dataset, ds2, K), case = _gather_case()
F = case['det'].shape[0]
lines = []                                                                    # written to a file per rank: two processes share the pipe
parts = {'split': ((0, GATHER_CUT), (GATHER_CUT, F)), 'rank1_empty': ((0, GATHER_CUT), None), 'rank0_empty': (None, (0, F))}
for run, part in parts.items():
    ev = DetectionEvaluator(dataset, ds2, num_classes=K)
    if part[rank] is not None:
        lo, hi = part[rank]
        ev.add_frames(*_to({k: v[lo:hi] for k, v in case.items()}, torch.device('cpu')))
    ev.all_gather()
    lines.append(f'DIGEST {run} {rank} {_digest(ev)}')
bad = DetectionEvaluator(dataset, ds2, num_classes=K + rank)                  # the ranks disagree: every rank raises, none hangs
try:
    bad.all_gather()
    lines.append(f'NO ERROR {rank}')
except ValueError as e:
    lines.append(f'REFUSED {rank} {str(e)[:60]}')
dist.destroy_process_group()
with open(os.path.join(out_dir, f'rank{rank}.txt'), 'w') as f:
    f.write('\n'.join(lines) + '\n')
'''


def _gather_case():
    return ('gen4', True, 3), cg.random_case(131, 'gen4', True, 3, 30, 6, 24)


def test_all_gather_world2_gloo(tmp_path):
    """Two CPU processes on the emulator build over gloo: after all_gather both ranks hold the union in rank order and print the
    digest of the single-process evaluation - each rank writes its lines to a file of its own - with the frames split over the ranks, with rank 1 holding nothing and with rank 0
    holding nothing (an evaluator that never saw a tensor)."""
    from tests.backends import emu_library
    L._install_test_library(emu_library())
    try:
        (dataset, ds2, K), case = _gather_case()
        want = {}
        for run, hi in (('split', 30), ('rank1_empty', GATHER_CUT), ('rank0_empty', 30)):
            ev = DetectionEvaluator(dataset, ds2, num_classes=K)
            ev.add_frames(*_to({k: v[:hi] for k, v in case.items()}, torch.device('cpu')))
            assert ev.counts()['images'] > 0 and ev.summary()['AR_100'] > 0
            want[run] = _digest(ev)
        assert want['split'] != want['rank1_empty']
    finally:
        L._install_test_library(None)
    script = tmp_path / 'gather.py'
    script.write_text(GATHER_WORKER)
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
                        '--master-port', '29757', str(script), ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = ''.join((tmp_path / f'rank{rank}.txt').read_text() for rank in (0, 1))
    got = {tuple(line.split()[1:3]): line.split()[3] for line in out.splitlines() if line.startswith('DIGEST')}
    assert got == {(run, str(rank)): want[run] for run in want for rank in (0, 1)}, (got, want, r.stderr[-2000:])
    assert out.count('REFUSED') == 2 and 'NO ERROR' not in out, out[-2000:]


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_add_frames_then_recall_graph_capture():
    """reset + add_frames + rvt_coco_recall captured in ONE torch.cuda.graph and replayed on new contents: the eager tp table."""
    dev = torch.device('cuda', 0)
    c = cg.CASES['eval_gen1']
    F, K, R = 64, c['K'], min(c['max_det'], 100 * c['K'])
    cases = [cg.random_case(s, c['dataset'], c['ds2'], K, F, c['G'], c['max_det']) for s in (21, 22, 23)]
    bufs = _to(cases[0], dev)
    ev = DetectionEvaluator(c['dataset'], c['ds2'])
    ev.add_frames(*bufs)                                                   # eager warm-up: store, counters and tables allocated
    tp = torch.zeros(3, K, 40, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.reset()
        ev.add_frames(*bufs)
        tp.zero_()
        key, matched, ignored = (ev._planes[i, :F * R] for i in range(3))
        L.call('rvt_coco_recall', L.ptr(key), L.ptr(matched), L.ptr(ignored), F, R, K, L.ptr(tp), L.stream_of(tp))
    assert ev._spans == [(0, F, R)]
    for case in cases[1:]:
        for b, src in zip(bufs, _to(case, dev)):
            b.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = DetectionEvaluator(c['dataset'], c['ds2'])
        eager.add_frames(*_to(case, dev))
        assert eager.recall_counts()[2].sum() > 0
        assert np.array_equal(tp.cpu().numpy().reshape(3, K, 10, 4), eager.recall_counts())
        ev.invalidate()                                                    # the replay changed the store behind the host's back
        assert np.array_equal(ev.recall_table(), eager.recall_table()) and ev.summary() == eager.summary()
