"""rvt_amd.YoloXDetector, the native detector class: the reference's module layout and call contract
(models/detection/yolox_extension/models/detector.py:18-72) without the reference.

The first test repeats the checks of tests/test_host.py::test_dropin_through_reference_registry_and_detector, with that test's
tolerances, on the native class: the fixture tests/golden/dropin_detector.npz was recorded from the reference's own YoloXDetector
(oracle/make_golden_dropin.py) with the seeded weights and inputs of tests/casegen_dropin.py.  Neither the reference nor omegaconf
is needed, so it runs on the GPU as well as on the emulator."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rvt_amd
from rvt_amd.postprocess import postprocess_padded
from tests import casegen_dropin as cg
from tests.backends import backend  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', cg.GOLDEN + '.npz'))


def _detector(dev, gold, dtype=torch.float32):
    m = rvt_amd.YoloXDetector(cg.model_cfg(), compute_dtype=dtype)
    ints = {n[4:]: gold[n] for n in gold.files if n.startswith('int:')}
    missing = m.load_state_dict(cg.seeded_state(m.state_dict(), ints), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return m.to(dev)


def _rel(a, ref):
    ref = torch.from_numpy(np.asarray(ref))
    assert tuple(a.shape) == tuple(ref.shape), (tuple(a.shape), tuple(ref.shape))
    return (a.detach().float().cpu() - ref).abs().max().item() / ref.abs().max().item()


def test_detector_matches_reference_golden(backend):
    dev = backend
    gold = _gold()
    names = [str(n) for n in gold['names']]
    shapes = [str(s) for s in gold['shapes']]
    assert len(names) == 424
    for cfg in (cg.model_cfg(), cg.model_cfg('mi355x'), rvt_amd.AttrDict(cg.model_cfg())):     # impl / compile keys are ignored
        sd = rvt_amd.YoloXDetector(cfg).state_dict()
        assert list(sd) == names, 'state_dict names / order differ from the reference detector'
        assert [','.join(map(str, t.shape)) for t in sd.values()] == shapes, 'state_dict shapes differ from the reference detector'
    ours = _detector(dev, gold).eval()
    assert [type(m).__module__.split('.')[0] for m in (ours.backbone, ours.fpn, ours.yolox_head)] == ['rvt_amd'] * 3

    xs = cg.make_inputs()
    st = None
    with torch.no_grad():
        for t in range(xs.shape[0]):
            fo, st = ours.forward_backbone(F.pad(xs[t].float(), [0, 6, 0, 4]).to(dev), st)     # modules/detection.py:133-134
            assert sorted(fo) == [1, 2, 3, 4]
            for s in fo:
                err = _rel(fo[s], gold[f'feat_t{t}_s{s}'])
                assert err < 1e-3, (t, s, err)
        for i, (h, c) in enumerate(st):
            assert _rel(h, gold[f'h{i}']) < 1e-3 and _rel(c, gold[f'c{i}']) <= 1e-3, i
        out, losses = ours.forward_detect(backbone_features=fo)
        assert losses is None and _rel(out, gold['detections']) <= 2e-3
    # training mode on the reference's own last-step features: SimOTA losses and the gradient into the backbone features
    ours.train()
    fo_g = {s: torch.from_numpy(gold[f'feat_t{xs.shape[0] - 1}_s{s}']).clone().to(dev).requires_grad_(True) for s in (1, 2, 3, 4)}
    _, loss = ours.forward_detect(backbone_features=fo_g, targets=cg.make_targets().to(dev))
    assert sorted(loss) == sorted(n[5:] for n in gold.files if n.startswith('loss:'))
    for k in ('loss', 'iou_loss', 'conf_loss', 'cls_loss', 'num_fg'):
        a, b = float(loss[k].detach()), float(gold['loss:' + k])
        assert abs(a - b) <= 2e-3 * max(abs(b), 1e-6), (k, a, b)
    loss['loss'].backward()
    for s in (2, 3, 4):
        err = _rel(fo_g[s].grad, gold[f'feat_grad_s{s}'])
        assert err < 2e-3, (s, err)


def test_detector_forward_contract(backend):
    dev = backend
    gold = _gold()
    m = _detector(dev, gold).eval()
    xs = cg.make_inputs().to(dev)
    nc = 3
    with torch.no_grad():
        out, losses, st0 = m(xs[0], None, retrieve_detections=False)
        assert out is None and losses is None and len(st0) == 4 and all(len(p) == 2 for p in st0)
        out, losses, st1 = m(xs[1], st0)
        assert losses is None and out.dim() == 3 and out.shape[0] == 2 and out.shape[2] == 5 + nc
    # detect: the same step ending in the fused tail - the rows of postprocess_padded(forward), the states of forward
    n_cand = 0
    for conf, agn, max_det in ((0.0, False, None), (0.02, True, None), (0.0, False, 4)):
        want = tuple(t.clone() for t in postprocess_padded(out, nc, conf, 0.45, agn, max_det=max_det))
        (det, cnt, aidx), st = m.detect(xs[1], st0, conf, 0.45, agn, max_det=max_det)
        assert torch.equal(det.view(torch.int32), want[0].view(torch.int32)) and torch.equal(cnt, want[1]) and torch.equal(aidx, want[2])
        for (h, c), (hw, cw) in zip(st, st1):
            assert torch.equal(h, hw) and torch.equal(c, cw) and h.stride() == hw.stride()
        n_cand += int(cnt.sum())
    assert n_cand > 0, 'no detection at all: the comparison checks nothing'
    # the sequence form is the backbone's
    with torch.no_grad():
        feats, st_seq = m.forward_sequence(xs[:2], None)
    for (h, c), (hw, cw) in zip(st_seq, st1):
        assert torch.equal(h, hw) and torch.equal(c, cw)
    assert sorted(feats) == [1, 2, 3, 4] and feats[1].shape[:2] == (2, 2)
    # the reference's guards: training mode needs targets; no targets without detections
    m.train()
    with pytest.raises(AssertionError):
        m(xs[0].float())
    with pytest.raises(AssertionError):
        m(xs[0].float(), None, retrieve_detections=False, targets=cg.make_targets().to(dev))
    with pytest.raises(AssertionError):
        m.detect(xs[0], None, 0.1, 0.45)
