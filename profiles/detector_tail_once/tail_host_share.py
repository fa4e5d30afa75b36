"""Host share of the detector tail on one MI355X: PAFPN + YOLOX head at RVT-Base widths on K labelled 1 Mpx frames (the tail of
profiles/bench_detector_step.py without the backbone), bf16.  Per training step (forward + SimOTA losses + backward) and per eval
`detect_padded` call: wall time with a device synchronise, and the host's enqueue time alone (the clock stops before the synchronise).
Usage: python profiles/detector_tail_once/tail_host_share.py [K, default 96] [steps, default 20]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rvt_amd import fpn as F_, head as H_  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 96
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev, dt = torch.device('cuda', 0), torch.bfloat16
dims, strides, hw = (128, 256, 512), (8, 16, 32), (384, 640)
torch.manual_seed(0)
neck = F_.YOLOPAFPN(depth=0.67, in_channels=dims, compute_dtype=dt).to(dev)
head = H_.YOLOXHead(num_classes=3, strides=strides, in_channels=dims, compute_dtype=dt).to(dev)
feats = {s: torch.randn(K, hw[0] // st, hw[1] // st, c, device=dev).to(dt).permute(0, 3, 1, 2) for s, c, st in zip((2, 3, 4), dims, strides)}
feats8 = {s: f[:8] for s, f in feats.items()}                  # the eval call: a streaming batch of 8 frames
g = torch.Generator().manual_seed(0)
labels = torch.zeros(K, 16, 5)
for b in range(K):
    n = int(torch.randint(1, 17, (1,), generator=g))
    r = torch.rand(n, 5, generator=g)
    labels[b, :n] = torch.stack([(r[:, 0] * 3).floor(), 20 + r[:, 1] * 600, 20 + r[:, 2] * 344, 16 + r[:, 3] * 200, 16 + r[:, 4] * 150], 1)
labels = labels.to(dev)


def train_step():
    head(neck(feats), labels)[1]['loss'].backward()
    for p in params:
        p.grad = None


def detect():
    with torch.no_grad():
        head.detect_padded(neck(feats8), 0.1, 0.45)


def measure(fn, steps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    host = wall = 0.0
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        host += t1 - t0
        wall += time.perf_counter() - t0
    return round(host / steps * 1e3, 3), round(wall / steps * 1e3, 3)


params = list(neck.parameters()) + list(head.parameters())
neck.train(), head.train()
th, tw = measure(train_step, steps)
neck.eval(), head.eval()
eh, ew = measure(detect, 20 * steps)               # (a ~1 ms call: as long a window as the training steps')
print(json.dumps({'what': 'detector tail alone: PAFPN + YOLOX head, RVT-Base widths, K labelled 1 Mpx frames, bf16', 'K': K,
                  'train_host_ms': th, 'train_wall_ms': tw, 'eval_host_ms': eh, 'eval_wall_ms': ew}), flush=True)
