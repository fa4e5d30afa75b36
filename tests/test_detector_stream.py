"""rvt_amd.graph.GraphedDetectorStream: one streaming detection step (masked state reset, backbone, PAFPN, head maps, decode + score
filter + NMS, state carry) replayed as ONE hipGraph launch, against the eager YoloXDetector.detect loop.  Both routes issue the
same kernels on the same bits, so det, count and anchor_idx are compared with torch.equal."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CONF, NMS = 0.1, 0.45
NC, B = 2, 3


def _detector(dev):
    """RVT-Tiny / Gen1, bf16, random weights; LayerScale O(1) so the features depend on the frames, and head biases that make
    every step a detection problem: objectness / class logits around 0 (scores around 0.25, far above CONF) and extents of three
    strides, so neighbouring boxes overlap (IoU 0.5 between grid neighbours) and NMS has boxes to suppress."""
    import rvt_amd
    cfg = {'backbone': rvt_amd.backbone_config('tiny', 'gen1'),
           'fpn': {'name': 'PAFPN', 'depth': 0.33, 'in_stages': [2, 3, 4], 'depthwise': False, 'act': 'silu'},
           'head': {'name': 'YoloX', 'depthwise': False, 'act': 'silu', 'num_classes': NC}}
    torch.manual_seed(0)
    m = rvt_amd.YoloXDetector(cfg, compute_dtype=torch.bfloat16)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith('gamma'):
                p.fill_(0.5)
        for conv in list(m.yolox_head.obj_preds) + list(m.yolox_head.cls_preds):
            conv.bias.zero_()
        for conv in m.yolox_head.reg_preds:
            conv.bias[2:4] = math.log(3.0)
    return m.to(dev).eval()


def _frames(dev, n=5):
    g = torch.Generator(device=dev).manual_seed(1)
    return [torch.randint(0, 11, (B, 20, 240, 304), generator=g, dtype=torch.uint8, device=dev) for _ in range(n)]


def test_detector_stream_graph_matches_eager():
    from rvt_amd.graph import GraphedDetectorStream
    from rvt_amd.postprocess import postprocess_padded
    from rvt_amd.states import RNNStates
    dev = torch.device('cuda', 0)
    m = _detector(dev)
    frames = _frames(dev)
    is_first = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    want = []
    st = None
    for i, f in enumerate(frames):
        if i == 3:                                          # sequence boundary of sample 1: its state restarts from zeros
            st = RNNStates.recursive_reset(st, is_first.bool())
        with torch.no_grad():
            pred = m(f, st)[0]
        (det, cnt, aidx), st = m.detect(f, st, CONF, NMS)
        cand = ((pred[..., 4] * pred[..., 5:].max(-1).values) >= CONF).sum(1)
        print(f'step {i}: candidates {cand.tolist()} kept {cnt.tolist()}')
        assert int(cnt.min()) > 0 and bool((cnt < cand).all()), (i, cnt.tolist(), cand.tolist())
        two = postprocess_padded(pred, NC, CONF, NMS)
        assert torch.equal(det, two[0]) and torch.equal(cnt, two[1]) and torch.equal(aidx, two[2]), i
        want.append((det.clone(), cnt.clone(), aidx.clone()))
    assert not torch.equal(want[3][0][1], want[2][0][1])
    gs = GraphedDetectorStream(m, frames[0], CONF, NMS)
    assert gs.reset_mask.dtype == torch.uint8 and tuple(gs.reset_mask.shape) == (B,) and gs.frame_buffer.dtype == torch.uint8
    for i, f in enumerate(frames):
        if i == 3:
            gs.reset_mask.copy_(is_first)
        got = gs(f)
        torch.cuda.synchronize()
        assert not gs.reset_mask.any(), 'the captured step must clear the mask'
        for name, g, w in zip(('det', 'count', 'anchor_idx'), got, want[i]):
            assert torch.equal(g, w), (i, name)
    gs.reset()                                              # all states back to zero: the first steps again
    for i in range(2):
        got = gs(frames[i])
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want[i])), i
    gs.close()


def test_detector_stream_producer_writes_input():
    from rvt_amd.graph import GraphedDetectorStream
    dev = torch.device('cuda', 0)
    m = _detector(dev)
    frames = _frames(dev, 3)
    gs = GraphedDetectorStream(m, frames[0], CONF, NMS, max_det=100)
    copied = []
    for f in frames:
        copied.append(tuple(t.clone() for t in gs(f)))
    assert int(copied[-1][1].min()) > 0 and copied[-1][0].shape == (B, 100, 7)
    gs.reset()
    for f, want in zip(frames, copied):
        gs.frame_buffer.zero_()
        gs.frame_buffer.add_(f)                             # a producer writes the graph's input in place: no frame copy by the stream
        got = gs()
        torch.cuda.synchronize()
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    gs.close()


def test_detector_stream_guards():
    from rvt_amd.graph import GraphedDetectorStream
    dev = torch.device('cuda', 0)
    m = _detector(dev)
    frame = _frames(dev, 1)[0]
    gs = GraphedDetectorStream(m, frame, CONF, NMS)
    with pytest.raises(ValueError, match='frame must be'):
        gs(frame[:2])
    with pytest.raises(ValueError, match='frame must be'):
        gs(frame.float())
    with pytest.raises(ValueError, match='frame must be'):
        gs(frame[:, :, :, :300])
    gs(frame)
    torch.cuda.synchronize()
    gs.close()
    with pytest.raises(RuntimeError, match='closed'):
        gs(frame)
    with pytest.raises(RuntimeError, match='closed'):
        gs()
