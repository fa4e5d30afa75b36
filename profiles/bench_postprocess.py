"""Timing of the on-device detection post-processing (rvt_amd.postprocess.postprocess_padded: score filter + batched NMS, one
launch per batch) on one MI355X, against what a user had before it: the plain-torch restatement tests/postprocess_ref.py run on the
same cuda tensors (per-image loop, boolean-mask indexing, all-pairs IoU matrix on the device, greedy pass on the host).  For scale,
the eval-mode YOLOX head forward (towers + decode, RVT-Base widths, bf16) at the same batch and resolution.

Inputs: the tests' clustered prediction tensors (tests/casegen_postprocess.py) tiled to the batch size, at three candidate densities
per case: about 1 % of the anchors (conf_thre = the 99th percentile of the scores), the fixtures' density (conf_thre = 0.1) and
100 % (conf_thre = 0: every anchor a candidate, the worst case).  nms_thre = 0.45, per-class NMS.
The kernel path and the head are timed with device events over >= 50 calls after a warm-up; the restatement synchronises with the
host inside every call, so it is timed with a host clock around synchronised calls, over a handful of calls (it takes seconds).
The two paths are checked for identical output on every row before anything is timed.

Usage: python profiles/bench_postprocess.py [--calls 50] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rvt_amd import head as H_  # noqa: E402
from rvt_amd.postprocess import postprocess_padded  # noqa: E402
from tests import casegen_postprocess as cg  # noqa: E402
from tests.postprocess_ref import postprocess_ref  # noqa: E402

ROWS = (('pp_1mpx', 24), ('pp_1mpx', 64), ('pp_gen1', 64))
NMS_THRE = 0.45


def event_median_ms(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def host_median_ms(fn, budget_s=6.0, min_calls=3):
    fn()
    torch.cuda.synchronize()
    ts, t_end = [], time.perf_counter() + budget_s
    while len(ts) < min_calls or (time.perf_counter() < t_end and len(ts) < 50):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), len(ts)


def head_forward_ms(name, B, calls, dev):
    c = cg.CASES[name]
    dims = (128, 256, 512)                                                   # RVT-Base stage widths 2..4
    head = H_.YOLOXHead(num_classes=c['nc'], strides=c['strides'], in_channels=dims, compute_dtype=torch.bfloat16).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn(B, ch, h, w, device=dev, generator=g).to(torch.bfloat16) for ch, (h, w) in zip(dims, c['hws'])]
    with torch.no_grad():
        return event_median_ms(lambda: head(xs), calls)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# detection post-processing on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# kernel / head: median of {args.calls} event-timed calls (min..max in brackets); restatement: median of n host-timed synchronised calls',
             '# case      B     A  density  conf_thre  candidates/img  kept/img | hip ms [min..max]        | restatement ms (n) | ratio | eval head fwd ms']
    for name, B in ROWS:
        c = cg.CASES[name]
        base = torch.from_numpy(cg.make_prediction(name).copy())
        pred = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1)[:B].contiguous().to(dev)
        A, nc = pred.shape[1], c['nc']
        score = pred[:, :, 4] * pred[:, :, 5:].max(dim=2).values
        head_ms = head_forward_ms(name, B, args.calls, dev)
        for label, conf in (('1%', float(np.quantile(score.cpu().numpy(), 0.99))), ('fixture', 0.1), ('100%', 0.0)):
            det, count, _ = postprocess_padded(pred, nc, conf, NMS_THRE)
            want = postprocess_ref(pred, nc, conf, NMS_THRE)
            torch.cuda.synchronize()
            for b, w in enumerate(want):                                      # same output before any timing
                n = 0 if w is None else w.shape[0]
                assert int(count[b]) == n and (n == 0 or torch.equal(det[b, :n], w)), f'{name} B={B} {label}: image {b} differs'
            ncand = float((score >= conf).sum()) / B
            kept = float(count.sum()) / B
            med, lo, hi = event_median_ms(lambda: postprocess_padded(pred, nc, conf, NMS_THRE), args.calls)
            ref_ms, n_ref = host_median_ms(lambda: postprocess_ref(pred, nc, conf, NMS_THRE))
            lines.append(f'{name:8s} {B:3d} {A:5d}  {label:7s}  {conf:9.4f}  {ncand:14.1f}  {kept:8.1f} | {med:7.3f} [{lo:.3f}..{hi:.3f}] | '
                         f'{ref_ms:10.2f} ({n_ref:2d})    | {ref_ms / med:6.1f}x | {head_ms:7.3f}')
            print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
