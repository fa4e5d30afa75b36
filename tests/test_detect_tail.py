"""The fused detection tail (rvt_yolox_detect: decode + score filter + NMS in one launch, csrc/nms.hpp) against the two launches it
replaces: rvt_amd.head.decode into the [B][A][5 + nc] fp32 tensor, then rvt_amd.postprocess.postprocess_padded.

Bar.  The fused kernel evaluates the decode kernel's expressions (same translation unit, same flags) and then runs the same
sort / NMS code on the same bits, so det, count and anchor_idx are compared with torch.equal: no tolerance anywhere."""
import numpy as np
import pytest
import torch

from rvt_amd.head import decode
from rvt_amd.postprocess import detect_padded, postprocess_padded
from tests.backends import backend  # noqa: F401

STRIDES = (8, 16, 32)
NMS_THRE = 0.45
MID_CONF = 0.3


def _pad8(n):
    return (n + 7) // 8 * 8


def _make_maps(seed, B, hws, nc, dtype, dev):
    """Per-level [reg|obj|pad] (ld 8) and [cls|pad] (ld pad8(nc)) maps: centres within a cell or two of the grid point, extents 2 - 5
    strides (neighbouring boxes overlap), objectness / class logits around 0 with the lower classes favoured (so that a class holds
    several overlapping boxes even at nc = 80).  The padding columns carry noise: reading one shows."""
    g = torch.Generator().manual_seed(seed)
    maps = []
    for (H, W) in hws:
        ro = torch.randn(B, H, W, 8, generator=g)
        ro[..., 2:4] = torch.log(2.0 + 3.0 * torch.rand(B, H, W, 2, generator=g))
        ro[..., 4] = 1.5 * torch.randn(B, H, W, generator=g)
        cl = 1.5 * torch.randn(B, H, W, _pad8(nc), generator=g)
        cl[..., :nc] -= 0.1 * torch.arange(nc, dtype=torch.float32)
        maps += [ro.to(dtype).to(dev), cl.to(dtype).to(dev)]
    return maps


def _two_step(maps, hws, nc, conf, agn, max_det=None):
    pred = decode(maps, hws, STRIDES[:len(hws)], nc)
    det, cnt, aidx = postprocess_padded(pred, nc, conf, NMS_THRE, agn, max_det=max_det)
    return pred, det.clone(), cnt.clone(), aidx.clone()


def _assert_same(got, want, what):
    for name, g, w in zip(('det', 'count', 'anchor_idx'), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        if name == 'det':                                  # bit for bit: -0.0 and 0.0 must not pass for each other
            assert torch.equal(g.cpu().view(torch.int32), w.cpu().view(torch.int32)), (what, name)
        else:
            assert torch.equal(g, w), (what, name)


# (id, seed, B, level shapes, nc): the smallest shapes at which each path of the kernel can go wrong
SHAPES = [
    ('a51_under_one_block', 1, 3, ((5, 7), (3, 4), (2, 2)), 3),
    ('a315_blocks_nc1', 2, 2, ((12, 20), (6, 10), (3, 5)), 1),
    ('a315_blocks_nc80', 3, 2, ((12, 20), (6, 10), (3, 5)), 80),
    ('a5460_two_sort_chunks', 4, 1, ((52, 80), (26, 40), (13, 20)), 2),
    ('one_level_b64', 5, 64, ((8, 8),), 2),
]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name,seed,B,hws,nc', SHAPES, ids=[s[0] for s in SHAPES])
def test_detect_equals_decode_then_postprocess(backend, name, seed, B, hws, nc, dtype):
    dev = backend
    maps = _make_maps(seed, B, hws, nc, dtype, dev)
    A = sum(h * w for h, w in hws)
    strides = STRIDES[:len(hws)]
    for agn in (False, True):
        for conf, max_det in ((0.0, None), (MID_CONF, None), (0.05, 3)):
            what = f'{name} agnostic {agn} conf {conf} max_det {max_det}'
            pred, det, cnt, aidx = _two_step(maps, hws, nc, conf, agn, max_det)
            # the two-step route alone must make this a test: detections in every image, and NMS that suppresses something
            cand = ((pred[..., 4] * pred[..., 5:].max(-1).values) >= conf).sum(1).to(torch.int32)
            assert int(cnt.min()) > 0, what
            assert bool((cnt < cand).any()), f'{what}: nothing suppressed in any image'
            if conf == 0.0:
                assert cand.tolist() == [A] * B, what
            if max_det is not None:
                assert int(cnt.max()) > max_det, f'{what}: max_det is not below the kept count'
            got = detect_padded(maps, hws, strides, nc, conf, NMS_THRE, agn, max_det=max_det)
            _assert_same(got, (det, cnt, aidx), what)


def test_detect_class_tie_after_sigmoid(backend):
    """Two class logits that differ but round to the same fp32 sigmoid: the class max must run over the sigmoid values, where the
    lower class wins the tie, as it does in the decoded tensor - a max over the logits would pick the higher class."""
    dev = backend
    one = np.float32(1.0)
    x = next(k for k in range(1, 60) if one / (one + np.float32(np.exp(np.float32(-k)))) == one)    # 1 + exp(-x) rounds to 1
    lo, hi = float(x + 2), float(x + 5)                 # well inside the saturated range of any expf: both sigmoids are exactly 1
    hws, nc = ((2, 2),), 3
    for dtype in (torch.float32, torch.bfloat16):
        ro = torch.zeros(1, 2, 2, 8)
        ro[..., 2:4] = -1.0                             # small disjoint boxes: nothing suppressed
        ro[..., 4] = 1.0
        cl = torch.zeros(1, 2, 2, 8)
        cl[..., 0], cl[..., 1], cl[..., 2] = -3.0, lo, hi
        cl[0, 1, 1, 1], cl[0, 1, 1, 2] = hi, lo         # and the other way round: still class 1
        maps = [ro.to(dtype).to(dev), cl.to(dtype).to(dev)]
        assert float(maps[1][0, 0, 0, 1]) != float(maps[1][0, 0, 0, 2])
        pred, det, cnt, aidx = _two_step(maps, hws, nc, 0.1, False)
        assert torch.equal(pred[..., 6], pred[..., 7]) and bool((pred[..., 6] == 1.0).all()), 'the sigmoids do not tie'
        assert cnt.tolist() == [4] and det[0, :, 6].tolist() == [1.0] * 4
        got = detect_padded(maps, hws, STRIDES[:1], nc, 0.1, NMS_THRE, False)
        _assert_same(got, (det, cnt, aidx), f'class tie {dtype}')


def test_detect_rejects_unsupported(backend):
    """Outside the supported range: the library's message, and nothing is launched (the caller's outputs keep their contents)."""
    dev = backend

    def zeros(hws, nc):
        return [t for h, w in hws for t in (torch.zeros(1, h, w, 8, device=dev), torch.zeros(1, h, w, _pad8(nc), device=dev))]

    def out(A):
        return (torch.full((1, A, 7), 5.0, device=dev), torch.full((1,), -3, dtype=torch.int32, device=dev),
                torch.full((1, A), 9, dtype=torch.int32, device=dev))

    for hws, nc, msg in ((((1, 16385),), 1, 'A=16385 anchors outside the supported range'),
                         (((2, 4),), 81, 'num_classes=81 outside the supported range'),
                         (((1, 1),) * 9, 1, '9 levels outside the supported range')):
        A = sum(h * w for h, w in hws)
        o = out(A)
        with pytest.raises(RuntimeError, match=msg):
            detect_padded(zeros(hws, nc), hws, (8,) * len(hws), nc, 0.1, NMS_THRE, out=o)
        assert bool((o[0] == 5.0).all()) and o[1].tolist() == [-3] and bool((o[2] == 9).all())


def test_head_detect_padded_equals_forward_then_postprocess(backend):
    """YOLOXHead.detect_padded on the head_micro inputs against postprocess_padded(head(xs)[0]): bit-identical."""
    from tests import casegen_head as cgh
    from tests.test_head import _build
    dev = backend
    m, _ = _build('head_micro', dev, torch.float32)
    m.eval()
    xs = [torch.from_numpy(a).to(dev) for a in cgh.make_inputs('head_micro')]
    nc = cgh.CASES['head_micro']['nc']
    with torch.no_grad():
        pred, _ = m(xs)
    n_total = 0
    for conf, agn in ((0.01, False), (0.001, True)):
        want = tuple(t.clone() for t in postprocess_padded(pred, nc, conf, 0.45, agn))
        got = m.detect_padded(xs, conf, 0.45, agn)
        _assert_same(got, want, f'conf {conf}')
        n_total += int(want[1].sum())
        again = m.detect_padded(xs, conf, 0.45, agn)                        # cached per shape: the same tensors, nothing new
        assert all(a.data_ptr() == g.data_ptr() for a, g in zip(again, got))
    assert n_total > 0, 'the head_micro detections give no candidate at all: the test checks nothing'


@pytest.mark.gpu
def test_detect_graph_capture():
    """One launch, no host synchronisation, nothing allocated after the first call: detect_padded captures into a torch.cuda.graph
    and replays on new map contents at the same addresses."""
    dev = torch.device('cuda', 0)
    hws, nc, B = ((12, 20), (6, 10), (3, 5)), 3, 4
    A = sum(h * w for h, w in hws)
    src = _make_maps(7, B, hws, nc, torch.bfloat16, dev)
    maps = [t.clone() for t in src]
    out = (torch.empty(B, A, 7, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, A, dtype=torch.int32, device=dev))
    detect_padded(maps, hws, STRIDES, nc, MID_CONF, NMS_THRE, out=out)      # eager warm-up: workspace allocated and cached
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        detect_padded(maps, hws, STRIDES, nc, MID_CONF, NMS_THRE, out=out)
    for shift in (1, 2):                                                    # new map CONTENTS at the same addresses
        for t, s in zip(maps, src):
            t.copy_(torch.roll(s, shifts=(shift, shift), dims=(0, 2)))
        for t in out:
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        eager = (torch.empty_like(out[0]), torch.empty_like(out[1]), torch.empty_like(out[2]))
        detect_padded(maps, hws, STRIDES, nc, MID_CONF, NMS_THRE, out=eager)
        torch.cuda.synchronize()
        assert int(got[1].min()) > 0
        _assert_same(got, eager, f'shift {shift}')
        _assert_same(got, _two_step(maps, hws, nc, MID_CONF, False)[1:], f'shift {shift} two-step')


def test_detect_launch_is_priced(backend):
    """opmodel.py prices the launch from its recorded arguments: the maps read once, the outputs, the workspace written and read."""
    import opmodel
    from rvt_amd import _lib
    dev = backend
    hws, nc, B = ((5, 7), (3, 4), (2, 2)), 3, 3
    maps = _make_maps(1, B, hws, nc, torch.bfloat16, dev)
    calls, orig = [], _lib.call

    def rec(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    _lib.call = rec
    try:
        detect_padded(maps, hws, STRIDES, nc, MID_CONF, NMS_THRE, max_det=10)
    finally:
        _lib.call = orig
    assert [n for n, _ in calls] == ['rvt_yolox_detect']
    name, args = calls[0]
    A = 51
    fl, by = opmodel.model(name, args)
    assert fl == 0.0 and by == B * A * (8 + 8) * 2 + B * 10 * 7 * 4 + B * 4 + B * 10 * 4 + 2 * 52 * B * A
    assert opmodel.executed(name, args) == 12.0 * B * A * (A - 1) / 2 + 3.0 * B * A * (1 + nc)
