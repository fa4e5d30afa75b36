"""Detection post-processing (score filter + batched NMS): rvt_amd.postprocess on the HIP kernel (emulator build on the CPU, gfx950
build on the GPU) against fixtures recorded from the unmodified reference `postprocess` (tests/make_golden_postprocess.py) and
against the plain-torch restatement of the semantics (tests/postprocess_ref.py, itself pinned to the same fixtures).

Bars.  Every output value is a copy of an input value or one correctly rounded fp32 operation on it, and every keep / kill decision
is the same fp32 formula in the same order as the reference's: counts, order and rows are compared for EXACT equality."""
import numpy as np
import pytest
import torch

from rvt_amd.postprocess import postprocess, postprocess_padded
from tests import casegen_postprocess as cg
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden
from tests.postprocess_ref import postprocess_ref

CASE_SETTINGS = [pytest.param(name, s, id=f'{name}-{cg.setting_id(s)}') for name in cg.CASES for s in cg.SETTINGS]


def _golden_rows(name, s):
    gold = load_golden(name)
    count, rows = gold[f'{cg.setting_id(s)}/count'], gold[f'{cg.setting_id(s)}/rows']
    return count, np.split(rows, np.cumsum(count)[:-1])


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_list(got, want_rows, what=''):
    """got: list of tensors / None; want_rows: list of [n][7] arrays (n = 0: None expected)."""
    assert len(got) == len(want_rows)
    for b, (g, w) in enumerate(zip(got, want_rows)):
        if w.shape[0] == 0:
            assert g is None, f'{what} image {b}: expected no detections, got {g.shape[0]}'
            continue
        assert g is not None and g.shape[0] == w.shape[0], f'{what} image {b}: {None if g is None else g.shape[0]} rows, expected {w.shape[0]}'
        ga = g.cpu().numpy()
        assert ga.dtype == np.float32 and ga.shape[1] == 7
        assert _same_bits(ga, np.ascontiguousarray(w, dtype=np.float32)), \
            f'{what} image {b}: first differing row {int(np.nonzero((ga != w).any(axis=1))[0][0])}'


def _check_padded(pred, got_list, det, count, aidx, max_det):
    """The padded form against the list form: same rows, zero tail, anchor_idx -1 there, rows traceable to their anchors."""
    det, count, aidx, p = det.cpu(), count.cpu(), aidx.cpu(), pred.cpu()
    assert det.shape == (pred.shape[0], max_det, 7) and aidx.shape == (pred.shape[0], max_det)
    for b, g in enumerate(got_list):
        n = 0 if g is None else g.shape[0]
        assert int(count[b]) == n
        m = min(n, max_det)
        if m:
            assert torch.equal(det[b, :m], g.cpu()[:m])
            idx = aidx[b, :m].long()
            assert int(idx.min()) >= 0 and int(idx.max()) < pred.shape[1] and idx.unique().numel() == m
            assert torch.equal(p[b, idx, 4], det[b, :m, 4])
        assert not det[b, m:].any() and bool((aidx[b, m:] == -1).all())


def _ref_rows(pred, nc, conf, thr, agn):
    return [np.zeros((0, 7), np.float32) if r is None else r.cpu().numpy() for r in postprocess_ref(pred, nc, conf, thr, agn)]


@pytest.mark.parametrize('name,s', CASE_SETTINGS)
def test_restatement_matches_reference_golden(name, s):
    """Pins tests/postprocess_ref.py to the reference (CPU only): equal counts, bit-identical rows."""
    count, rows = _golden_rows(name, s)
    got = postprocess_ref(torch.from_numpy(cg.make_prediction(name).copy()), cg.CASES[name]['nc'], *s)
    assert [0 if g is None else g.shape[0] for g in got] == count.tolist()
    for g, w in zip(got, rows):
        assert (g is None) == (w.shape[0] == 0)
        if g is not None:
            assert np.array_equal(g.numpy(), w)


@pytest.mark.parametrize('name,s', CASE_SETTINGS)
def test_postprocess_vs_reference_golden(backend, name, s):
    """The kernel against the reference's own output: counts, None pattern, row order, rows bit for bit; the padded form agrees."""
    dev = backend
    nc = cg.CASES[name]['nc']
    count, rows = _golden_rows(name, s)
    pred = torch.from_numpy(cg.make_prediction(name).copy()).to(dev)
    got = postprocess(pred, nc, *s)
    assert [0 if g is None else g.shape[0] for g in got] == count.tolist()
    _check_list(got, rows, name)
    det, cnt, aidx = postprocess_padded(pred, nc, *s)
    _check_padded(pred, got, det, cnt, aidx, pred.shape[1])


def _random_prediction(seed, B, A, nc, dev):
    """Clustered boxes with exact score ties, duplicated rows (IoU = 1, equal scores) and zero-area boxes injected."""
    r = np.random.default_rng(1000 + seed)
    K = max(1, min(12, A // 6))
    centres = r.uniform(20, 300, (B, K, 2))
    sizes = r.uniform(10, 80, (B, K, 2))
    k = r.integers(0, K, (B, A))
    bi = np.arange(B)[:, None]
    pred = np.zeros((B, A, 5 + nc), dtype=np.float32)
    pred[:, :, 0:2] = centres[bi, k] + r.normal(0, 6, (B, A, 2))
    pred[:, :, 2:4] = sizes[bi, k] * r.uniform(0.7, 1.4, (B, A, 2))
    pred[:, :, 4] = r.uniform(0, 1, (B, A))
    pred[:, :, 5:] = r.uniform(0, 1, (B, A, nc))
    for b in range(B):
        m = max(1, A // 10)
        if A >= 4:
            src, dst = r.integers(0, A, m), r.integers(0, A, m)
            pred[b, dst] = pred[b, src]                                   # duplicated rows: IoU = 1 and an exact score tie
            src, dst = r.integers(0, A, m), r.integers(0, A, m)
            pred[b, dst, 4:] = pred[b, src, 4:]                           # equal scores and classes on different boxes
            pred[b, r.integers(0, A, m), 2] = 0                           # zero-area boxes
            pred[b, r.integers(0, A, max(1, m // 4)), 2:4] = 0
            if nc > 1:
                rows = r.integers(0, A, m)
                pred[b, rows, 5 + r.integers(0, nc, m)] = pred[b, rows, 5:].max(axis=1)   # exact class ties
    return torch.from_numpy(pred).to(dev)


# the emulator runs a workgroup as fibers on one thread: the large B goes with a small A and the large A with a small B
RANDOM_SHAPES = [
    (0, 1, 81, 3), (1, 2, 1000, 2), (2, 1, 4097, 3), (3, 64, 64, 1), (4, 3, 200, 80), (5, 2, 5040, 3),
    (6, 1, 9000, 2), (7, 5, 1, 1), (8, 4, 640, 5), (9, 2, 2048, 4), (10, 1, 63, 1),
]


@pytest.mark.parametrize('seed,B,A,nc', RANDOM_SHAPES)
def test_postprocess_random_shapes_vs_restatement(backend, seed, B, A, nc):
    """Shapes without a fixture (A not a multiple of 64, one to three sort chunks, B = 1 and 64, 1 and 80 classes), random
    thresholds, exact ties / duplicates / zero-area boxes: exact equality with the restatement, class-aware and agnostic."""
    dev = backend
    r = np.random.default_rng(2000 + seed)
    pred = _random_prediction(seed, B, A, nc, dev)
    for agn in (False, True):
        conf = float(r.choice([0.0, r.uniform(0.005, 0.05), r.uniform(0.05, 0.5)]))
        thr = float(r.uniform(0.2, 0.8))
        want = _ref_rows(pred, nc, conf, thr, agn)
        got = postprocess(pred, nc, conf, thr, agn)
        _check_list(got, want, f'seed {seed} conf {conf:.4f} nms {thr:.4f} agnostic {agn}')
        max_det = max(1, A // 3)
        det, cnt, aidx = postprocess_padded(pred, nc, conf, thr, agn, max_det=max_det)
        _check_padded(pred, got, det, cnt, aidx, max_det)


def _grid_boxes(B, A, nc, dev, size=4.0, pitch=10.0):
    """Disjoint boxes on a grid, descending scores in anchor order, every anchor a candidate."""
    pred = torch.zeros(B, A, 5 + nc)
    i = torch.arange(A, dtype=torch.float32)
    pred[:, :, 0] = (i % 32) * pitch + 5
    pred[:, :, 1] = torch.div(i, 32, rounding_mode='floor') * pitch + 5
    pred[:, :, 2:4] = size
    pred[:, :, 4] = 1.0 - i / (2 * A)
    pred[:, :, 5] = 0.9
    return pred.to(dev)


def test_postprocess_edges(backend):
    dev = backend
    nc, A = 2, 300
    # an image with no candidate beside a full image
    pred = _grid_boxes(2, A, nc, dev)
    pred[0, :, 4] = 0.0
    before = pred.clone()
    got = postprocess(pred, nc, 0.1, 0.45)
    assert torch.equal(pred, before), 'the input tensor was modified'
    assert got[0] is None and got[1] is not None and got[1].shape == (A, 7)      # disjoint boxes: nothing suppressed
    det, cnt, aidx = postprocess_padded(pred, nc, 0.1, 0.45)
    assert cnt.tolist() == [0, A] and not det[0].any() and bool((aidx[0] == -1).all())
    assert aidx[1].tolist() == list(range(A))                                       # descending scores in anchor order
    _check_list(got, _ref_rows(pred, nc, 0.1, 0.45, False))
    # every anchor suppressed by one box: heavily overlapping boxes of one class, anchor 7 scores highest
    pred = _grid_boxes(1, A, nc, dev, size=50.0, pitch=0.01)
    pred[0, :, 4] *= 0.9
    pred[0, 7, 4] = 1.0
    got = postprocess(pred, nc, 0.1, 0.45)
    assert got[0].shape == (1, 7) and torch.equal(got[0][0, :4].cpu(), torch.tensor([pred[0, 7, 0] - 25, pred[0, 7, 1] - 25,
                                                                                   pred[0, 7, 0] + 25, pred[0, 7, 1] + 25]).cpu())
    det, cnt, aidx = postprocess_padded(pred, nc, 0.1, 0.45)
    assert cnt.tolist() == [1] and int(aidx[0, 0]) == 7
    # the same boxes in alternating classes: two survive class-aware, one class-agnostic
    pred[0, 1::2, 5], pred[0, 1::2, 6] = 0.1, 0.9
    assert postprocess(pred, nc, 0.1, 0.45)[0].shape[0] == 2 and postprocess(pred, nc, 0.1, 0.45, True)[0].shape[0] == 1
    # max_det smaller than the kept count: the top rows, count untruncated
    pred = _grid_boxes(2, A, nc, dev)
    full = postprocess(pred, nc, 0.1, 0.45)
    det, cnt, aidx = postprocess_padded(pred, nc, 0.1, 0.45, max_det=17)
    assert cnt.tolist() == [A, A] and det.shape == (2, 17, 7)
    for b in range(2):
        assert torch.equal(det[b], full[b][:17]) and aidx[b].tolist() == list(range(17))
    # caller-provided outputs
    out = (torch.full((2, 17, 7), 5.0, device=dev), torch.full((2,), -3, dtype=torch.int32, device=dev),
           torch.full((2, 17), 9, dtype=torch.int32, device=dev))
    d2, c2, a2 = postprocess_padded(pred, nc, 0.1, 0.45, max_det=17, out=out)
    assert d2 is out[0] and torch.equal(d2, det) and torch.equal(c2, cnt) and torch.equal(a2, aidx)
    # non-fp32 / non-contiguous input is converted, not rejected
    wide = torch.zeros(2, A, 5 + nc + 3, device=dev)
    wide[:, :, :5 + nc] = pred
    _check_list(postprocess(wide[:, :, :5 + nc], nc, 0.1, 0.45), [f.cpu().numpy() for f in full])
    _check_list(postprocess(pred.double(), nc, 0.1, 0.45), [f.cpu().numpy() for f in full])
    # outside the supported range: the library's message, before any launch
    with pytest.raises(RuntimeError, match='anchors outside the supported range'):
        postprocess(torch.zeros(1, 16385, 6, device=dev), 1, 0.1, 0.45)
    with pytest.raises(RuntimeError, match='num_classes=81 outside the supported range'):
        postprocess(torch.zeros(1, 8, 86, device=dev), 81, 0.1, 0.45)


def test_head_eval_then_postprocess(backend):
    """YOLOXHead.eval() on the head_micro maps, then postprocess: equals the restatement applied to the same detections."""
    from tests import casegen_head as cgh
    from tests.test_head import _build
    dev = backend
    m, _ = _build('head_micro', dev, torch.float32)
    m.eval()
    xs = [torch.from_numpy(a).to(dev) for a in cgh.make_inputs('head_micro')]
    with torch.no_grad():
        det, _ = m(xs)
    nc = cgh.CASES['head_micro']['nc']
    n_total = 0
    for conf, agn in ((0.01, False), (0.001, True)):
        got = postprocess(det, nc, conf, 0.45, agn)
        want = _ref_rows(det, nc, conf, 0.45, agn)
        _check_list(got, want, f'conf {conf}')
        n_total += sum(w.shape[0] for w in want)
    assert n_total > 0, 'the head_micro detections give no candidate at all: the test checks nothing'


@pytest.mark.gpu
def test_postprocess_graph_capture():
    """One launch, no host synchronisation, nothing allocated after the first call: postprocess_padded captures into a
    torch.cuda.graph on one stream and replays on new input contents at the same addresses."""
    dev = torch.device('cuda', 0)
    name, (conf, thr, agn) = 'pp_gen1', cg.SETTINGS[0]
    nc = cg.CASES[name]['nc']
    src = torch.from_numpy(cg.make_prediction(name).copy()).to(dev)
    pred = src.clone()
    B, A, _ = pred.shape
    out = (torch.empty(B, A, 7, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, A, dtype=torch.int32, device=dev))
    postprocess_padded(pred, nc, conf, thr, agn, out=out)                 # eager warm-up: workspace allocated and cached
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        postprocess_padded(pred, nc, conf, thr, agn, out=out)
    for shift in (1, 2):                                                    # new input CONTENTS at the same addresses
        pred.copy_(torch.roll(src, shifts=(shift, 17 * shift), dims=(0, 1)))
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        eager = (torch.empty_like(out[0]), torch.empty_like(out[1]), torch.empty_like(out[2]))
        postprocess_padded(pred, nc, conf, thr, agn, out=eager)
        torch.cuda.synchronize()
        assert int(got[1].min()) > 0
        for g, e in zip(got, eager):
            assert torch.equal(g, e)
