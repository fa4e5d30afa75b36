"""The weight-cache protocol every module of the detector offers (invalidate_weight_cache, weight_caches), the two-pass arena builder
behind ModelWeights and ConvPack, and GraphedStep's check of the protocol.  CPU emulator only: nothing here is a kernel matter."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rvt_amd
from rvt_amd import _lib, weights
from tests import casegen_dropin, casegen_fpn, casegen_head
from tests.test_fpn import _build as build_fpn
from tests.test_head import _build as build_head


@pytest.fixture
def emu():
    from tests.backends import emu_library
    _lib._install_test_library(emu_library())
    yield torch.device('cpu')
    _lib._install_test_library(None)


@pytest.mark.parametrize('which', ['typed', 'fp32'])
@pytest.mark.parametrize('more', [1, -1])
def test_two_pass_builder_refuses_passes_that_disagree(which, more):
    def fill(tab, arT, ar32):
        arT.take(3, 7)
        ar32.take(128)
        arena = arT if which == 'typed' else ar32
        arena.take(64 + ((tab is not None) == (more > 0)))       # the view pass asks for one element more (less) than the sizing pass
        return 'filled'
    with pytest.raises(RuntimeError, match='sizing pass'):
        weights.build_arenas(torch.float32, torch.device('cpu'), fill)


def test_two_pass_builder_hands_back_what_fill_built():
    seen = []

    def fill(tab, arT, ar32):
        a, b = arT.take(3, 5), ar32.take(7)
        seen.append((tab, a, b))
        return a, b
    bufT, buf32, tab, (a, b) = weights.build_arenas(torch.bfloat16, torch.device('cpu'), fill, zero32=True)
    assert seen[0] == (None, None, None) and seen[1][0] is tab and len(seen) == 2
    assert bufT.dtype == torch.bfloat16 and buf32.dtype == torch.float32 and not bool(buf32.any())
    assert a.data_ptr() == bufT.data_ptr() and tuple(a.shape) == (3, 5) and b.data_ptr() == buf32.data_ptr() and tab.dev is not None


def _check_stale_then_fresh(run, build, write):
    """An eval forward after a write through .data is stale; after invalidate_weight_cache() it is a freshly built module's."""
    m = build()
    before = run(m)
    write(m)
    stale = run(m)
    assert all(torch.equal(a, b) for a, b in zip(before, stale)), 'a write through .data does not move _version: the caches cannot see it'
    m.invalidate_weight_cache()
    after = run(m)
    fresh = build()
    write(fresh)
    want = run(fresh)
    assert all(torch.equal(a, b) for a, b in zip(after, want))
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    return m


def test_fpn_invalidate_weight_cache_after_a_data_write(emu):
    xs = {s: torch.from_numpy(a) for s, a in casegen_fpn.make_inputs('fpn_micro').items()}

    def run(m):
        with torch.no_grad():
            return [o.clone() for o in m(xs)]
    m = _check_stale_then_fresh(run, lambda: build_fpn('fpn_micro', emu, torch.float32)[0].eval(),
                                lambda m: m.C3_p3.conv1.conv.weight.data.mul_(0.5))
    held = m.weight_caches()
    assert any(t is m._pack.bufT for t in held) and any(t is m._pack.buf32 for t in held) and any(t is m._pack.table for t in held)
    assert all(any(t is c._pk.fin for t in held) for c in m._pack.convs)


def test_head_invalidate_weight_cache_after_a_data_write(emu):
    xs = [torch.from_numpy(a) for a in casegen_head.make_inputs('head_micro')]

    def run(m):
        with torch.no_grad():
            return [m(xs)[0].clone()]

    def write(m):
        m.stems[0].bn.running_mean.data.add_(0.5)
        m.cls_preds[1].bias.data.add_(1.0)
    m = _check_stale_then_fresh(run, lambda: build_head('head_micro', emu, torch.float32)[0].eval(), write)
    held = m.weight_caches()
    assert any(t is m._pack.bufT for t in held) and len(held) > 3 + len(m._pack.convs)       # ... and the padded prediction weights


def test_detector_invalidate_weight_cache_reaches_its_three_parts(emu):
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', casegen_dropin.GOLDEN + '.npz'))
    ints = {n[4:]: gold[n] for n in gold.files if n.startswith('int:')}
    x = F.pad(casegen_dropin.make_inputs()[0].float(), [0, 6, 0, 4])

    def build():
        m = rvt_amd.YoloXDetector(casegen_dropin.model_cfg())
        m.load_state_dict(casegen_dropin.seeded_state(m.state_dict(), ints), strict=True)
        return m.eval()

    def run(m):
        with torch.no_grad():
            det, _, states = m(x)
        return [det.clone()] + [h.clone() for h, _ in states]
    for part, write in (('backbone', lambda m: next(m.backbone.parameters()).data.mul_(0.5)),
                        ('fpn', lambda m: m.fpn.lateral_conv0.conv.weight.data.mul_(0.5)),
                        ('yolox_head', lambda m: m.yolox_head.stems[0].bn.running_mean.data.add_(0.5))):
        m = _check_stale_then_fresh(run, build, write)
        assert len(m.weight_caches()) == sum(len(p.weight_caches()) for p in (m.backbone, m.fpn, m.yolox_head)), part
        assert m.backbone.weight_caches() == [m.backbone._mw_cache]


def test_graphed_step_refuses_a_model_without_the_protocol_before_running_anything():
    from rvt_amd.graph import GraphedStep
    calls = []
    with pytest.raises(TypeError, match='invalidate_weight_cache'):
        GraphedStep(lambda: calls.append(1), models=(object(),))
    assert not calls
    for cls in (rvt_amd.RNNDetector, rvt_amd.YoloXDetector, rvt_amd.fpn.YOLOPAFPN, rvt_amd.head.YOLOXHead):
        assert callable(getattr(cls, 'invalidate_weight_cache', None)) and callable(getattr(cls, 'weight_caches', None)), cls
