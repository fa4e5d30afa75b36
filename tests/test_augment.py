"""Spatial training augmentation (flip / zoom-in / zoom-out of event planes and box labels): rvt_amd.augment on the HIP kernels
(emulator build on the CPU, gfx950 build on the GPU) against fixtures recorded from the unmodified reference
RandomSpatialAugmentorGenX (tests/make_golden_augment.py) and against the plain-torch restatement (tests/augment_ref.py, itself
pinned to the same fixtures).

Bars.  Every output byte is a copy of an input byte or zero, and every label value is a copy or a chain of single rounded fp32
operations in the reference's order: everything is compared for EXACT equality (torch.equal / equal bits).  No tolerance."""
import warnings

import numpy as np
import pytest
import torch

from rvt_amd import augment as A
from rvt_amd.augment import RandomSpatialAugmentorGenX, SpatialAugmentState
from rvt_amd.types import DataType
from tests import casegen_augment as cg
from tests.augment_ref import labels_ref, planes_ref
from tests.backends import backend  # noqa: F401
from tests.harness import load_golden

CASE_NAMES = list(cg.CASES)


def _states(gold) -> list:
    return [SpatialAugmentState(flip=bool(r[0]), mode=int(r[1]), x0=int(r[2]), y0=int(r[3]), factor=float(r[4])) for r in gold['states']]


def _packed(name, dev=None):
    labels = cg.make_labels(name)
    return A.pack_labels([[labels[b][t] for b in range(len(labels))] for t in range(cg.T_LABELS)], device=dev)


def _same_bits(a: torch.Tensor, b) -> bool:
    a = a.cpu().numpy()
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _kernel_count(gold_count: np.ndarray, count_in: torch.Tensor) -> torch.Tensor:
    """The fixture holds -1 where the reference ends with None; the kernel reports 0 for a frame that had labels and lost them."""
    g = torch.from_numpy(gold_count)
    return torch.where((g < 0) & (count_in.cpu() > 0), torch.zeros_like(g), g)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_fixture_conditions(name):
    gold = load_golden(name)
    cg.check_states(name, gold['states'])
    assert gold['coded'].shape == (len(cg.CASES[name]['seeds']), 5) + tuple(cg.CASES[name]['hw'])


def test_fixture_conditions_overall():
    per = {}
    for name in CASE_NAMES:
        gold = load_golden(name)
        _, cin = _packed(name)
        per[name] = (gold['states'], cin.numpy(), _kernel_count(gold['count_out'], cin).numpy())
    cg.check_results(per)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_sample_states_match_reference_draws(name):
    """CPU only: the same torch RNG calls in the same order as the reference, so the same seed gives the same state."""
    gold = load_golden(name)
    c = cg.CASES[name]
    labels = cg.make_labels(name)
    got = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for b, seed in enumerate(c['seeds']):
            torch.manual_seed(seed)
            aug = RandomSpatialAugmentorGenX(c['hw'], True, cg.AUGM_CONFIG)
            got += A.sample_states(aug, [labels[b]])
    assert np.array_equal(cg.states_array(got), gold['states'])


@pytest.mark.parametrize('name', CASE_NAMES)
def test_restatement_matches_reference_golden(name):
    """Pins tests/augment_ref.py to the reference (CPU only): planes and label rows bit for bit."""
    gold = load_golden(name)
    hw = cg.CASES[name]['hw']
    st = _states(gold)
    coded = torch.from_numpy(cg.coded_planes(hw))
    ev = coded.unsqueeze(0).unsqueeze(0).repeat(1, len(st), 1, 1, 1)
    assert torch.equal(planes_ref(ev, st)[0], torch.from_numpy(gold['coded']))
    rows, count = _packed(name)
    ro, co, yo = labels_ref(rows, count, st, hw)
    assert torch.equal(co, _kernel_count(gold['count_out'], count).to(co.dtype))
    assert _same_bits(ro, gold['rows_out']) and _same_bits(yo, gold['yolox'])


@pytest.mark.parametrize('name', CASE_NAMES)
def test_planes_vs_reference_golden(backend, name):
    """The planes kernel on the coded planes equals the reference's recorded source map; on event-like planes it equals a
    gather through that map."""
    dev = backend
    gold = load_golden(name)
    hw = cg.CASES[name]['hw']
    st = _states(gold)
    B = len(st)
    it, _ = A.make_tables(st, hw, dev)
    coded = torch.from_numpy(cg.coded_planes(hw)).to(dev)
    ev = coded.unsqueeze(0).unsqueeze(0).repeat(1, B, 1, 1, 1).contiguous()
    out = A.augment_planes(ev, it)
    assert torch.equal(out[0].cpu(), torch.from_numpy(gold['coded']))
    T, C = 2, 3
    src = torch.from_numpy(cg.event_planes(name, T, C))
    m = gold['coded'].astype(np.int64)
    sx, sy, valid = torch.from_numpy(m[:, 0] | (m[:, 1] << 8)), torch.from_numpy(m[:, 2] | (m[:, 3] << 8)), torch.from_numpy(m[:, 4] == 255)
    want = torch.empty_like(src)
    for b in range(B):
        want[:, b] = src[:, b][:, :, sy[b], sx[b]] * valid[b].to(torch.uint8)
    got = A.augment_planes(src.to(dev), it)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_labels_vs_reference_golden(backend, name):
    dev = backend
    gold = load_golden(name)
    hw = cg.CASES[name]['hw']
    st = _states(gold)
    rows, count = _packed(name, dev)
    _, ft = A.make_tables(st, hw, dev)
    ro, co, yo = A.augment_labels(rows, count, ft)
    assert torch.equal(co.cpu(), _kernel_count(gold['count_out'], count))
    assert _same_bits(ro, gold['rows_out']) and _same_bits(yo, gold['yolox'])
    # the reference's labelled-frame selection: None after zoom-in, an empty label set after zoom-out
    assert torch.equal(A.labelled_frames(co, st).cpu(), torch.from_numpy(gold['count_out'] >= 0))
    ro2, co2, none = A.augment_labels(rows, count, ft, yolox=False)
    assert none is None and torch.equal(ro2, ro) and torch.equal(co2, co)


def _random_states(r, B, H, W, edges):
    out = []
    for b in range(B):
        mode = int(r.integers(0, 3))
        s = SpatialAugmentState(flip=bool(r.integers(0, 2)), mode=mode)
        if mode:
            s.factor = float(r.uniform(1.01, 1.6))
            zh, zw = s.window_hw((H, W))
            ex = edges[b % len(edges)]
            s.x0 = {'l': 0, 'r': W - zw}.get(ex[0], int(r.integers(0, W - zw + 1)))
            s.y0 = {'t': 0, 'b': H - zh}.get(ex[1], int(r.integers(0, H - zh + 1)))
        out.append(s)
    return out


def _random_labels(r, T, B, G, H, W):
    rows = np.zeros((T, B, G, 7), dtype=np.float32)
    count = r.integers(-1, G + 1, (T, B)).astype(np.int32)            # frames with count -1 and 0 included
    x = r.uniform(0, W - 3, (T, B, G))
    y = r.uniform(0, H - 3, (T, B, G))
    rows[..., 0] = r.integers(0, 1000, (T, B, G))
    rows[..., 1], rows[..., 2] = x, y
    rows[..., 3] = r.uniform(0.5, W - 1 - x)
    rows[..., 4] = r.uniform(0.5, H - 1 - y)
    rows[..., 5] = r.integers(0, 3, (T, B, G))
    rows[..., 6] = r.uniform(0, 1, (T, B, G))
    for t in range(T):
        for b in range(B):
            rows[t, b, max(count[t, b], 0):] = 0
    return torch.from_numpy(rows), torch.from_numpy(count)


# (seed, T, B, C, H, W, G): W % 16 != 0 (byte path), W % 16 == 0 (16-byte path), B = 1, G = 1, W across the 256-column LDS skew,
# the largest supported W on the 16-byte path and the widest row on the byte path
RANDOM_SHAPES = [(0, 2, 3, 2, 17, 23, 3), (1, 1, 4, 3, 40, 64, 5), (2, 3, 1, 2, 24, 48, 1), (3, 1, 5, 1, 9, 304, 4),
                 (4, 2, 6, 2, 33, 528, 2), (5, 1, 2, 20, 20, 100, 6), (6, 1, 4, 1, 70, 16, 1), (7, 1, 3, 1, 3, 2048, 2),
                 (8, 2, 2, 1, 5, 2047, 1)]


@pytest.mark.parametrize('seed,T,B,C,H,W,G', RANDOM_SHAPES)
def test_random_shapes_vs_restatement(backend, seed, T, B, C, H, W, G):
    """Shapes without a fixture, a zoom window touching every edge, frames with count 0 and -1, the stacked tensor and a list of
    T separately allocated tensors: exact equality with the restatement."""
    dev = backend
    r = np.random.default_rng(3000 + seed)
    st = _random_states(r, B, H, W, edges=('lt', 'rb', 'lb', 'rt', '..'))
    ev = torch.from_numpy(r.integers(0, 256, (T, B, C, H, W)).astype(np.uint8))
    rows, count = _random_labels(r, T, B, G, H, W)
    want_ev = planes_ref(ev, st)
    want = labels_ref(rows, count, st, (H, W))
    ev_out, ro, co, yo = A.augment_sequence(ev.to(dev), rows.to(dev), count.to(dev), st)
    assert torch.equal(ev_out.cpu(), want_ev)
    assert torch.equal(co.cpu(), want[1]) and _same_bits(ro, want[0]) and _same_bits(yo, want[2])
    parts = [ev[t].clone().to(dev) for t in range(T)]                  # separately allocated, never stacked
    ev_list, *_ = A.augment_sequence(parts, rows.to(dev), count.to(dev), st)
    assert torch.equal(ev_list.cpu(), want_ev)


def test_factor_one_and_identity(backend):
    dev = backend
    r = np.random.default_rng(7)
    ev = torch.from_numpy(r.integers(0, 11, (1, 2, 2, 12, 32)).astype(np.uint8)).to(dev)
    rows, count = _random_labels(r, 1, 2, 3, 12, 32)
    st = [SpatialAugmentState(), SpatialAugmentState(flip=True)]
    ev_out, ro, co, _ = A.augment_sequence(ev, rows.to(dev), count.to(dev), st)
    assert torch.equal(ev_out[:, 0], ev[:, 0]) and torch.equal(ev_out[:, 1], torch.flip(ev[:, 1], dims=[-1]))
    assert torch.equal(ro[:, 0].cpu(), rows[:, 0]) and torch.equal(co.cpu(), count)
    # a factor of exactly 1 is mode 0: the augmentor never produces a zoom state with it, and the tables reject one
    with pytest.raises(ValueError, match='factor'):
        A.make_tables([SpatialAugmentState(mode=1, factor=1.0)] * 2, (12, 32), dev)
    aug = RandomSpatialAugmentorGenX((12, 32), True, dict(prob_hflip=0, rotate=dict(prob=0, max_angle_deg=0),
                                                          zoom=dict(prob=1, zoom_out=dict(weight=1, factor=dict(min=1, max=1)))))
    assert aug.draw([None]) == SpatialAugmentState()


def test_rejected_inputs(backend):
    dev = backend
    st = [SpatialAugmentState(mode=2, factor=1.25, x0=1, y0=1)]
    it, ft = A.make_tables(st, (16, 32), dev)
    ev = torch.zeros(1, 1, 2, 16, 32, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match='overlap'):
        A.augment_planes(ev, it, out=ev)
    with pytest.raises(ValueError, match='outside the 16x32 frame'):
        A.make_tables([SpatialAugmentState(mode=1, factor=1.25, x0=20, y0=0)], (16, 32), dev)
    with pytest.raises(TypeError, match='uint8'):
        A.augment_planes(ev.float(), it)
    with pytest.raises(TypeError, match='float32'):
        A.augment_labels(torch.zeros(1, 1, 2, 7, dtype=torch.float64, device=dev), torch.zeros(1, 1, dtype=torch.int32, device=dev), ft)
    with pytest.raises(RuntimeError, match='W=4096 outside the supported range'):
        A.augment_planes(torch.zeros(1, 1, 1, 1, 4096, dtype=torch.uint8, device=dev), it)
    cfg = dict(cg.AUGM_CONFIG, rotate=dict(prob=0.5, min_angle_deg=2, max_angle_deg=6))
    with pytest.raises(NotImplementedError, match='rotate.prob'):
        RandomSpatialAugmentorGenX((16, 32), True, cfg)
    with pytest.raises(AssertionError, match='zoom_in_weight'):
        RandomSpatialAugmentorGenX((16, 32), False, cg.AUGM_CONFIG)
    aug = RandomSpatialAugmentorGenX((16, 32), True, cg.AUGM_CONFIG)
    with pytest.raises(NotImplementedError, match='IMAGE'):
        aug({DataType.EV_REPR: [ev[0, 0]], DataType.OBJLABELS_SEQ: [None], DataType.IMAGE: [ev[0, 0]]})


def test_call_one_sequence(backend):
    """The reference's __call__ form on one sequence equals the batched form with the same draw."""
    dev = backend
    name = 'augment_odd'
    c = cg.CASES[name]
    labels = cg.make_labels(name)[1]
    ev = [torch.from_numpy(cg.event_planes(name, 1, 2)[0, 1]).to(dev) for _ in range(cg.T_LABELS)]
    torch.manual_seed(c['seeds'][1])
    aug = RandomSpatialAugmentorGenX(c['hw'], True, cg.AUGM_CONFIG)
    out = aug({DataType.EV_REPR: ev, DataType.OBJLABELS_SEQ: [None if a is None else torch.from_numpy(a) for a in labels]})
    torch.manual_seed(c['seeds'][1])
    st = A.sample_states(RandomSpatialAugmentorGenX(c['hw'], True, cg.AUGM_CONFIG), [labels])
    assert st[0].mode == 1
    rows, count = A.pack_labels([[a] for a in labels], device=dev)
    ev_b, ro, co, _ = A.augment_sequence([e.unsqueeze(0) for e in ev], rows, count, st)
    for t in range(cg.T_LABELS):
        assert torch.equal(out[DataType.EV_REPR][t], ev_b[t, 0])
        n = int(co[t, 0])
        assert (out[DataType.OBJLABELS_SEQ][t] is None) == (n <= 0)
        if n > 0:
            assert torch.equal(out[DataType.OBJLABELS_SEQ][t], ro[t, 0, :n])


def test_augment_then_stem(backend):
    """The augmented uint8 planes are the layout the backbone takes: forward_sequence runs on them."""
    from tests import casegen
    from tests.test_backbone import build_model
    dev = backend
    m = build_model('micro', dev, torch.float32)
    T, B, (H, W) = 2, 1, casegen.CASES['micro']['hw']
    ev = torch.from_numpy(np.random.default_rng(5).integers(0, 11, (T, B, 20, H, W)).astype(np.uint8)).to(dev)
    st = [SpatialAugmentState(flip=True, mode=1, factor=1.3, x0=3, y0=5)]
    it, _ = A.make_tables(st, (H, W), dev)
    out = A.augment_planes(ev, it)
    assert torch.equal(out.cpu(), planes_ref(ev.cpu(), st))
    with torch.no_grad():
        feats, _ = m.forward_sequence(out)
    assert all(torch.isfinite(f.float()).all() for f in feats.values())


@pytest.mark.gpu
def test_augment_graph_capture():
    """Planes + labels captured as one linear chain into a graph; replayed after the parameter tables were rewritten in place,
    the outputs equal the eager result for the new parameters."""
    dev = torch.device('cuda', 0)
    name = 'augment_gen1'
    gold = load_golden(name)
    hw = cg.CASES[name]['hw']
    st = _states(gold)
    B = len(st)
    ev = torch.from_numpy(cg.event_planes(name, 2, 4)).to(dev)
    rows, count = _packed(name, dev)
    it, ft = A.make_tables(st, hw, dev)
    ev_out = torch.empty_like(ev)
    lab_out = (torch.empty_like(rows), torch.empty_like(count), torch.empty(*rows.shape[:3], 5, device=dev))
    A.augment_planes(ev, it, out=ev_out)
    A.augment_labels(rows, count, ft, out=lab_out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.augment_planes(ev, it, out=ev_out)
        A.augment_labels(rows, count, ft, out=lab_out)
    for shift in (1, 3):
        st2 = st[shift:] + st[:shift]
        A.write_tables(st2, hw, it, ft)
        ev_out.fill_(7)
        for t in lab_out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = [ev_out.clone()] + [t.clone() for t in lab_out]
        it2, ft2 = A.make_tables(st2, hw, dev)
        eager = [A.augment_planes(ev, it2)] + list(A.augment_labels(rows, count, ft2))
        torch.cuda.synchronize()
        assert not torch.equal(got[0], ev)
        for g, e in zip(got, eager):
            assert torch.equal(g, e)
