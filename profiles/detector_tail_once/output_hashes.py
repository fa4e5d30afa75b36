"""Throw-away check of the detector-tail refactor: SHA-256 of the outputs, the losses and every parameter gradient of one training step
and one eval forward of `fpn_micro`, `head_micro` and the drop-in detector of tests/casegen_dropin.py, fp32 and bf16, so that the
outputs of two checkouts can be compared bit for bit.  Run from a checkout's root on the emulator:
    python profiles/detector_tail_once/output_hashes.py [--full] > hashes.txt"""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.getcwd())
import rvt_amd  # noqa: E402
from rvt_amd import _lib, tuning  # noqa: E402
from tests import casegen_dropin, casegen_fpn, casegen_head  # noqa: E402
from tests.backends import emu_library  # noqa: E402
from tests.test_fpn import _build as build_fpn  # noqa: E402
from tests.test_head import _build as build_head  # noqa: E402

_lib._install_test_library(emu_library())
tuning.use(**tuning.TEST_GEOMETRY)
dev = torch.device('cpu')


FULL = '--full' in sys.argv             # one line per tensor (1 436 lines); default: one digest per (case, dtype, phase, kind of tensor)
GROUPS = {}


def sha(title, t):
    t = t.detach()
    raw = (t.float() if t.dtype == torch.bfloat16 else t).contiguous().numpy().tobytes()
    line = f'{title} {t.dtype} {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}'
    if FULL:
        print(line)
    key = ' '.join(title.split()[:3] + [title.split()[3].rstrip('0123456789')])
    n, h = GROUPS.setdefault(key, [0, hashlib.sha256()])
    GROUPS[key][0] = n + 1
    h.update(line.encode() + b'\n')


def state(title, m):
    for n, p in m.named_parameters():
        sha(f'{title} grad {n}', p.grad)
    for n, b in m.named_buffers():
        sha(f'{title} buffer {n}', b)


for dtype in (torch.float32, torch.bfloat16):
    # ---- PAFPN
    m, _ = build_fpn('fpn_micro', dev, dtype)
    xs = {s: torch.from_numpy(a).to(dev) for s, a in casegen_fpn.make_inputs('fpn_micro').items()}
    cots = [torch.from_numpy(a).to(dev) for a in casegen_fpn.make_cotangents('fpn_micro')]
    m.train()
    xg = {s: x.clone().requires_grad_(True) for s, x in xs.items()}
    outs = m(xg)
    sum((o.float() * ct).sum() for o, ct in zip(outs, cots)).backward()
    for i, o in enumerate(outs):
        sha(f'fpn_micro {dtype} train out{i}', o)
    for s, x in xg.items():
        sha(f'fpn_micro {dtype} train dx{s}', x.grad)
    state(f'fpn_micro {dtype} train', m)
    m.eval()
    with torch.no_grad():
        for i, o in enumerate(m(xs)):
            sha(f'fpn_micro {dtype} eval out{i}', o)
    # ---- YOLOX head
    m, _ = build_head('head_micro', dev, dtype)
    xs = [torch.from_numpy(a).to(dev) for a in casegen_head.make_inputs('head_micro')]
    labels = torch.from_numpy(casegen_head.make_labels('head_micro', casegen_head.CASES['head_micro'])).to(dev)
    m.train()
    xg = [x.clone().requires_grad_(True) for x in xs]
    det, losses = m(xg, labels)
    losses['loss'].backward()
    sha(f'head_micro {dtype} train detections', det)
    for k, v in losses.items():
        sha(f'head_micro {dtype} train loss {k}', torch.as_tensor(v))
    for i, x in enumerate(xg):
        sha(f'head_micro {dtype} train dx{i}', x.grad)
    state(f'head_micro {dtype} train', m)
    m.eval()
    with torch.no_grad():
        sha(f'head_micro {dtype} eval detections', m(xs)[0])
        for n, t in zip(('det', 'count', 'anchor_idx'), m.detect_padded(xs, 0.1, 0.45)):
            sha(f'head_micro {dtype} eval detect_padded {n}', t)
    # ---- drop-in detector: three streaming steps, the loss on the last
    gold = np.load(os.path.join('tests', 'golden', casegen_dropin.GOLDEN + '.npz'))
    m = rvt_amd.YoloXDetector(casegen_dropin.model_cfg(), compute_dtype=dtype)
    m.load_state_dict(casegen_dropin.seeded_state(m.state_dict(), {n[4:]: gold[n] for n in gold.files if n.startswith('int:')}), strict=True)
    m = m.to(dev)
    frames = [F.pad(x.float(), [0, 6, 0, 4]).to(dev) for x in casegen_dropin.make_inputs()]
    targets = casegen_dropin.make_targets().to(dev)
    m.train()
    st = None
    for x in frames[:-1]:
        _, _, st = m(x, st, retrieve_detections=False)
    det, losses, st = m(frames[-1], st, targets=targets)
    losses['loss'].backward()
    sha(f'dropin {dtype} train detections', det)
    for k, v in losses.items():
        sha(f'dropin {dtype} train loss {k}', torch.as_tensor(v))
    for i, (h, c) in enumerate(st):
        sha(f'dropin {dtype} train h{i}', h)
        sha(f'dropin {dtype} train c{i}', c)
    state(f'dropin {dtype} train', m)
    m.eval()
    with torch.no_grad():
        st = None
        for x in frames:
            det, _, st = m(x, st)
        sha(f'dropin {dtype} eval detections', det)
        dets, _ = m.detect(frames[0], None, 0.1, 0.45)
        for n, t in zip(('det', 'count', 'anchor_idx'), dets):
            sha(f'dropin {dtype} eval detect {n}', t)

if not FULL:
    for key, (n, h) in GROUPS.items():
        print(f'{key}: {n} tensors {h.hexdigest()}')
