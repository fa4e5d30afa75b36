"""Timing of the on-device detection evaluation (rvt_amd.evaluation.DetectionEvaluator) on one MI355X.

  1. The match launch (`add_frames`) for a validation batch - 1 Mpx, 24 frames and Gen1, 64 frames - beside `postprocess_padded`
     on the same tensors in the same run: the tests' clustered prediction tensors (tests/casegen_postprocess.py) tiled to the batch
     size, conf_thre 0.1, nms_thre 0.45, max_det 256; the labels are the frame's first detections moved by a few pixels.
     Both are timed with device events over --calls calls after a warm-up.
  2. `evaluate()` (key sort, the accumulate kernels, the recall kernel, the one read-back) for a split-sized store: 20 000 and 200 000 frames of
     synthetic detections (tests/casegen_evaluation.py, 2 000 distinct frames repeated), host clock around the synchronising call;
     beside it `rvt_coco_accumulate` and `rvt_coco_recall` alone on the same stores, event-timed.
  3. The numpy restatement (tests/cocoeval_ref.py) on the same 20 000 frames on this box's host cores, once; its six metrics are
     compared with the device's before anything is reported.

Usage: python profiles/bench_evaluation.py [--calls 50] [--frames 20000,200000] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rvt_amd.evaluation import METRICS, DetectionEvaluator  # noqa: E402
from rvt_amd.postprocess import postprocess_padded  # noqa: E402
from tests import casegen_evaluation as cge  # noqa: E402
from tests import casegen_postprocess as cgp  # noqa: E402
from tests import cocoeval_ref  # noqa: E402

ROWS = (('pp_1mpx', 24, 'gen4'), ('pp_gen1', 64, 'gen1'))
MAX_DET, G = 256, 16
STORE = dict(dataset='gen4', ds2=True, K=3, G=8, max_det=48, base=2000)


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


def batch_rows(name, B, dataset, calls, dev):
    c = cgp.CASES[name]
    base = torch.from_numpy(cgp.make_prediction(name).copy())
    pred = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1)[:B].contiguous().to(dev)
    nc = c['nc']
    det, count, _ = postprocess_padded(pred, nc, 0.1, 0.45, max_det=MAX_DET)
    det, count = det.clone(), count.clone()
    rows = torch.zeros(B, G, 7, device=dev)
    rows[:, :, 1:3] = det[:, :G, 0:2] + 3.0
    rows[:, :, 3:5] = det[:, :G, 2:4] - det[:, :G, 0:2]
    rows[:, :, 5] = det[:, :G, 6]
    lcount = count.clamp(max=G)
    t_us = torch.full((B,), 1000000, dtype=torch.int64, device=dev)
    ev = DetectionEvaluator(dataset, False, num_classes=nc)
    ev.reserve((calls + 6) * B * min(MAX_DET, 100 * nc), device=dev)
    pp = event_median_ms(lambda: postprocess_padded(pred, nc, 0.1, 0.45, max_det=MAX_DET), calls)
    mt = event_median_ms(lambda: ev.add_frames(det, count, rows, lcount, t_us), calls)
    one = DetectionEvaluator(dataset, False, num_classes=nc)
    one.add_frames(det, count, rows, lcount, t_us)
    cts, m = one.counts(), one.evaluate()
    return (f'{name:8s} {B:3d} {pred.shape[1]:5d} {nc:2d} {float(count.float().mean()):9.1f} {int(cts["records"].sum()) / B:9.1f} '
            f'{int(cts["npig"][:, 0].sum()) / B:7.1f} | {pp[0]:7.3f} [{pp[1]:.3f}..{pp[2]:.3f}] | {mt[0]:7.3f} [{mt[1]:.3f}..{mt[2]:.3f}] | '
            f'{mt[0] / pp[0]:5.2f} | AP {m["AP"]:.4f} truncated {m["truncated_frames"]}')


def store_case():
    s = STORE
    return cge.random_case(77, s['dataset'], s['ds2'], s['K'], s['base'], s['G'], s['max_det'])


def fill(ev, case, frames, dev):
    bufs = tuple(torch.from_numpy(case[k]).to(dev) for k in ('det', 'count', 'rows', 'lcount', 't_us'))
    for _ in range(frames // STORE['base']):
        ev.add_frames(*bufs)


def evaluate_ms(ev, reps=5):
    ts = []
    for _ in range(reps + 1):
        ev.invalidate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.evaluate()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:]), out


def kernels_ms(ev, calls):
    """Event-timed medians of the two table kernels on the store as it stands: rvt_coco_accumulate on a permutation sorted once
    outside the timing, and the rvt_coco_recall launches of the store's spans (with the zeroing of their table)."""
    from rvt_amd import _lib as L
    from rvt_amd.evaluation import N_COUNTERS
    K, n = ev.num_classes, ev.slots
    key, matched, ignored = (ev._planes[i, :n] for i in range(3))
    perm = torch.sort(key, stable=True)[1]
    ws = torch.empty(max(int(L.get_lib().rvt_coco_accumulate_ws_bytes(n, K)), 1), dtype=torch.uint8, device=key.device)
    out = torch.empty(10 * 101 * K * 4 + N_COUNTERS, dtype=torch.float64, device=key.device)
    acc = event_median_ms(lambda: L.call('rvt_coco_accumulate', L.ptr(perm), L.ptr(matched), L.ptr(ignored), n, K, L.ptr(ev._counters),
                                         L.ptr(ev._thr[10:]), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_of(out)), calls)
    rec = event_median_ms(ev._recall_tp, calls)
    return acc, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--frames', default='20000,200000')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# detection evaluation on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# 1. one validation batch, max_det {MAX_DET}, G {G}: median of {args.calls} event-timed calls [min..max]',
             '# case      B     A nc  kept/img  records/img gt/img | postprocess_padded ms     | add_frames (match) ms     | ratio |']
    for name, B, dataset in ROWS:
        lines.append(batch_rows(name, B, dataset, args.calls, dev))
        print(lines[-1], flush=True)
    s = STORE
    case = store_case()
    lines += [f'# 2. evaluate() on a store of N frames ({s["base"]} distinct synthetic frames repeated, {s["K"]} classes, max_det {s["max_det"]}): '
              'median of 5 host-timed calls [min..max], sort + accumulate + recall + read-back',
              '#   frames    slots  records | evaluate ms               | AP']
    first, kernel_lines = None, []
    for n in [int(v) for v in args.frames.split(',')]:
        ev = DetectionEvaluator(s['dataset'], s['ds2'])
        fill(ev, case, n, dev)
        med, lo, hi, out = evaluate_ms(ev)
        lines.append(f'{ev.frames:10d} {ev.slots:8d} {int(ev.counts()["records"].sum()):8d} | {med:8.2f} [{lo:.2f}..{hi:.2f}] | {out["AP"]:.6f}')
        print(lines[-1], flush=True)
        acc, rec = kernels_ms(ev, args.calls)
        kernel_lines.append(f'{ev.frames:10d} {ev.slots:8d} | {acc[0]:7.3f} [{acc[1]:.3f}..{acc[2]:.3f}] | {rec[0]:7.3f} [{rec[1]:.3f}..{rec[2]:.3f}] | '
                            f'AR_100 {ev.summary()["AR_100"]:.6f}')
        print(kernel_lines[-1], flush=True)
        if first is None:
            first = (ev.frames, out)
        del ev
    lines += [f'# 2b. the table kernels alone on the same stores: median of {args.calls} event-timed calls [min..max]; evaluate() above runs both',
              '#   frames    slots | rvt_coco_accumulate ms     | rvt_coco_recall (+ zeroing its table) ms |'] + kernel_lines
    n, dev_out = first
    frames = cge.to_frames(case) * (n // s['base'])
    t0 = time.perf_counter()
    want = cocoeval_ref.evaluate_frames(frames, s['dataset'], s['ds2'], s['K'])
    ref_s = time.perf_counter() - t0
    for k in METRICS:
        assert abs(want['metrics'][k] - dev_out[k]) <= 1e-9, f'{k}: restatement {want["metrics"][k]!r}, device {dev_out[k]!r}'
    lines += [f'# 3. numpy restatement (tests/cocoeval_ref.py) on the same {n} frames, host, one run; its six metrics equal the device\'s to 1e-9',
              f'{n:10d} frames | {ref_s * 1e3:10.0f} ms']
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
