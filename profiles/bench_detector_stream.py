"""Timing of the streaming detection step on one MI355X: the fused detection tail (rvt_yolox_detect) and the whole step as one
hipGraph replay (rvt_amd.graph.GraphedDetectorStream), each against what it replaces, interleaved on the same device in one process.

Shapes: RVT-Base at 1 Mpx (384 x 640 model resolution, 3 classes, 5040 anchors) and RVT-Tiny on Gen1 (256 x 320, 2 classes, 1680
anchors), bf16, B = 64 and B = 1; PAFPN depth 0.67 as the reference's model config.  Random weights; LayerScale 0.5, objectness /
class biases 0 and extents of three strides so that the head's maps give overlapping boxes, and conf_thre set to the 97th percentile
of the scores of the first step: about 3 % of the anchors are candidates, the density the score filter leaves in deployment.

  (a) the tail alone, on the maps of one step: decode (one launch per level, the [B][A][5 + nc] fp32 tensor written) +
      postprocess_padded, against detect_padded (one launch).  Device events around each call, the two variants alternating.
  (b) the whole step, frame to kept boxes: the eager YoloXDetector.detect loop, GraphedDetectorStream called with a frame (one
      frame copy + one graph launch) and called without (a producer wrote frame_buffer: one graph launch).  A streaming consumer
      needs the boxes of step t before it feeds step t + 1, so each step is timed with a host clock from the call to the end of a
      device synchronise; the three variants alternate step by step, each carrying its own recurrent state.
The variants are checked for identical output before anything is timed.  p50 / p99 over --steps samples per variant.

Usage: python profiles/bench_detector_stream.py [--steps 200] [--out FILE]"""
import argparse
import datetime
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rvt_amd  # noqa: E402
from rvt_amd.graph import GraphedDetectorStream  # noqa: E402
from rvt_amd.head import decode  # noqa: E402
from rvt_amd.postprocess import detect_padded, postprocess_padded  # noqa: E402

ROWS = (('base_1mpx', 'base', 'gen4', (360, 640), 3), ('tiny_gen1', 'tiny', 'gen1', (240, 304), 2))
BATCHES = (64, 1)
NMS_THRE = 0.45


def build_detector(size, dataset, nc, dev):
    cfg = {'backbone': rvt_amd.backbone_config(size, dataset),
           'fpn': {'name': 'PAFPN', 'depth': 0.67, 'in_stages': [2, 3, 4], 'depthwise': False, 'act': 'silu'},
           'head': {'name': 'YoloX', 'depthwise': False, 'act': 'silu', 'num_classes': nc}}
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


def pct(ts):
    a = np.asarray(ts)
    return float(np.percentile(a, 50)), float(np.percentile(a, 99))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def bench_row(name, size, dataset, hw, nc, B, steps, dev):
    m = build_detector(size, dataset, nc, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    frames = [torch.randint(0, 11, (B, 20, *hw), generator=g, dtype=torch.uint8, device=dev) for _ in range(8)]
    head = m.yolox_head
    with torch.no_grad():
        feats, _ = m.forward_backbone(frames[0])
        maps, hws = head._pred_maps(m.fpn(feats))
        maps = [t.contiguous() for t in maps]
        pred = decode(maps, hws, head.strides, nc)
        score = pred[..., 4] * pred[..., 5:].max(-1).values
        conf = float(np.quantile(score.float().cpu().numpy(), 0.97))
    A = pred.shape[1]

    # ---- (a) the tail alone ----------------------------------------------------------------------------------------------
    two_step = lambda: postprocess_padded(decode(maps, hws, head.strides, nc), nc, conf, NMS_THRE)      # noqa: E731
    fused = lambda: detect_padded(maps, hws, head.strides, nc, conf, NMS_THRE)                            # noqa: E731
    want = tuple(t.clone() for t in two_step())
    assert same(fused(), want), f'{name} B={B}: the fused tail differs from decode + postprocess_padded'
    ncand, kept = float((score >= conf).sum()) / B, float(want[1].sum()) / B
    for _ in range(10):
        two_step()
        fused()
    torch.cuda.synchronize()
    t_two, t_fused = [], []
    for _ in range(steps):
        t_two.append(event_ms(two_step))
        t_fused.append(event_ms(fused))

    # ---- (b) the whole step ----------------------------------------------------------------------------------------------
    gs = GraphedDetectorStream(m, frames[0], conf, NMS_THRE)
    st = None
    for i in range(4):                                                       # same output, states carried, before any timing
        dets, st = m.detect(frames[i], st, conf, NMS_THRE)
        assert same(gs(frames[i]), dets), f'{name} B={B}: graph replay differs from the eager step {i}'
    gs2 = GraphedDetectorStream(m, frames[0], conf, NMS_THRE)               # the producer's stream: its own state and buffers
    state = {'st': None}

    def eager(f):
        _, state['st'] = m.detect(f, state['st'], conf, NMS_THRE)

    t_eager, t_copy, t_nocopy = [], [], []
    for i in range(steps + 5):
        f = frames[i % len(frames)]
        gs2.frame_buffer.copy_(f)                                            # the producer's write, outside the timed window
        torch.cuda.synchronize()
        a, b, c = host_ms(lambda: eager(f)), host_ms(lambda: gs(f)), host_ms(lambda: gs2())
        if i >= 5:
            t_eager.append(a)
            t_copy.append(b)
            t_nocopy.append(c)
    gs.close()
    gs2.close()
    res = [pct(t) for t in (t_two, t_fused, t_eager, t_copy, t_nocopy)]
    return (f'{name:9s} {B:3d} {A:5d} {conf:9.4f} {ncand:9.1f} {kept:7.1f} | ' +
            ' | '.join(f'{p50:8.3f} {p99:8.3f}' for p50, p99 in res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--rows', default=None, help='comma-separated subset of ' + ','.join(r[0] for r in ROWS))
    ap.add_argument('--batches', default=None, help='comma-separated batch sizes (default 64,1)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    rvt_amd.tuning.production()
    rows = [r for r in ROWS if args.rows is None or r[0] in args.rows.split(',')]
    batches = BATCHES if args.batches is None else tuple(int(b) for b in args.batches.split(','))
    lines = [f'# streaming detection step on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}, bf16',
             f'# p50 p99 in ms over {args.steps} samples per variant, variants alternating in one process',
             '# tail: device events around the call; step: host clock from the call to the end of a device synchronise',
             '# case        B     A conf_thre  cand/img kept/img | tail: decode+postprocess | tail: fused detect | step: eager detect '
             '| step: graph + frame copy | step: graph, producer wrote the frame']
    for name, size, dataset, hw, nc in rows:
        for B in batches:
            lines.append(bench_row(name, size, dataset, hw, nc, B, args.steps, dev))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
