"""Timing of the on-device spatial augmentation (rvt_amd.augment: rvt_augment_planes, rvt_augment_labels) on one MI355X.

Planes: the headline shape (T = 21, B = 24, 20 x 360 x 640) and Gen1 (T = 21, B = 8, 20 x 240 x 304), every sample in one mode
(none, flip, zoom-in, zoom-out, each zoom also flipped) and a mix drawn with the shipped probabilities.  Beside each figure, two
references measured in the same process on the same device tensors:
  (a) restatement: tests/augment_ref.planes_ref, the reference's torch ops (flip, interpolate nearest-exact, zero canvas) sample
      by sample on the device;
  (b) copy: out.copy_(in) of the same tensor, the floor for one read plus one write of every byte.
GB/s = (bytes written + bytes read by the model of opmodel.py) / time; the microarchitecture guide's measured copy rate is
6290 GB/s.  Labels: the kernel against the per-frame torch loop (tests/augment_ref.labels_ref) on device tensors.
Kernel and copy: median of device-event-timed calls after a warm-up; the restatement and the label loop synchronise with the host
(.tolist(), Python loop), so they are timed with a host clock around synchronised calls.  Outputs are checked equal before timing.

Usage: python profiles/bench_augment.py [--calls 30] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opmodel  # noqa: E402
from rvt_amd import augment as A  # noqa: E402
from tests import casegen_augment as cg  # noqa: E402
from tests.augment_ref import labels_ref, planes_ref  # noqa: E402

SHAPES = (('1mpx', 21, 24, 20, 360, 640), ('gen1', 21, 8, 20, 240, 304))
HBM_COPY_GBS = 6290.0


def event_median_ms(fn, calls, warmup=3):
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


def host_median_ms(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def uniform_states(B, H, W, flip, mode, factor):
    out = []
    for b in range(B):
        s = A.SpatialAugmentState(flip=flip, mode=mode, factor=factor if mode else 1.0)
        if mode:
            zh, zw = s.window_hw((H, W))
            s.x0, s.y0 = (b * 37) % (W - zw + 1), (b * 17) % (H - zh + 1)
        out.append(s)
    return out


def mixed_states(B, H, W, labels):
    torch.manual_seed(1234)
    aug = A.RandomSpatialAugmentorGenX((H, W), True, cg.AUGM_CONFIG)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return A.sample_states(aug, labels)


def random_labels(r, T, B, G, H, W):
    rows = np.zeros((T, B, G, 7), dtype=np.float32)
    count = np.where(r.random((T, B)) < 0.3, -1, r.integers(1, G + 1, (T, B))).astype(np.int32)
    x, y = r.uniform(0, W - 4, (T, B, G)), r.uniform(0, H - 4, (T, B, G))
    rows[..., 1], rows[..., 2] = x, y
    rows[..., 3], rows[..., 4] = r.uniform(1, np.minimum(W - 1 - x, W / 3)), r.uniform(1, np.minimum(H - 1 - y, H / 3))
    rows[..., 5], rows[..., 6] = r.integers(0, 3, (T, B, G)), 1.0
    for t in range(T):
        for b in range(B):
            rows[t, b, max(count[t, b], 0):] = 0
    return rows, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# spatial augmentation on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# hip / copy: median of {args.calls} event-timed calls [min..max]; restatement / label loop: median of 5 host-timed synchronised calls',
             f'# GB/s = modelled bytes (opmodel.py: source window read + every output byte written) / hip time; measured HBM copy rate {HBM_COPY_GBS:.0f} GB/s',
             '# planes  T  B   C   H   W  states      MB moved | hip ms [min..max]       GB/s  %copy-rate | copy_ ms  hip/copy | restatement ms  restatement/hip']
    r = np.random.default_rng(0)
    for name, T, B, C, H, W in SHAPES:
        ev = torch.from_numpy(r.integers(0, 11, (T, B, C, H, W)).astype(np.uint8)).to(dev)
        out = torch.empty_like(ev)
        G = 8
        rows_np, count_np = random_labels(r, T, B, G, H, W)
        labels = [[rows_np[t, b, :count_np[t, b]] if count_np[t, b] > 0 else None for t in range(T)] for b in range(B)]
        copy_ms = event_median_ms(lambda: out.copy_(ev), args.calls)[0]
        sets = [('none', uniform_states(B, H, W, False, 0, 1.0)), ('flip', uniform_states(B, H, W, True, 0, 1.0)),
                ('zoom-in 1.25', uniform_states(B, H, W, False, 1, 1.25)), ('flip+in 1.25', uniform_states(B, H, W, True, 1, 1.25)),
                ('zoom-out 1.1', uniform_states(B, H, W, False, 2, 1.1)), ('flip+out 1.1', uniform_states(B, H, W, True, 2, 1.1)),
                ('shipped mix', mixed_states(B, H, W, labels))]
        for label, st in sets:
            it, ft = A.make_tables(st, (H, W), dev)
            A.augment_planes(ev, it, out=out)
            assert torch.equal(out, planes_ref(ev, st)), f'{name} {label}: kernel and restatement differ'
            med, lo, hi = event_median_ms(lambda: A.augment_planes(ev, it, out=out), args.calls)
            ref_ms = host_median_ms(lambda: planes_ref(ev, st))
            nbytes = opmodel.augment_planes_bytes(T * B, C, H, W, [(s.mode,) + s.window_hw((H, W)) for s in st])
            gbs = nbytes / med / 1e6
            lines.append(f'{name:6s} {T:3d} {B:2d} {C:3d} {H:3d} {W:3d}  {label:12s} {nbytes / 1e6:8.1f} | {med:7.3f} [{lo:.3f}..{hi:.3f}] {gbs:7.0f} '
                         f'{100 * gbs / HBM_COPY_GBS:5.1f}%     | {copy_ms:7.3f}  {med / copy_ms:6.2f}x | {ref_ms:10.2f}     {ref_ms / med:8.1f}x')
            print(lines[-1], flush=True)
        # labels: the shipped mix
        st = sets[-1][1]
        _, ft = A.make_tables(st, (H, W), dev)
        rows, count = torch.from_numpy(rows_np).to(dev), torch.from_numpy(count_np).to(dev)
        lab_out = (torch.empty_like(rows), torch.empty_like(count), torch.empty(T, B, G, 5, device=dev))
        A.augment_labels(rows, count, ft, out=lab_out)
        want = labels_ref(rows, count, st, (H, W))
        assert all(torch.equal(g, w) for g, w in zip(lab_out, want)), f'{name}: label kernel and loop differ'
        med, lo, hi = event_median_ms(lambda: A.augment_labels(rows, count, ft, out=lab_out), args.calls)
        ref_ms = host_median_ms(lambda: labels_ref(rows, count, st, (H, W)), n=3)
        lines.append(f'# labels {name}: {T * B} frames, G = {G}, {int((count_np > 0).sum())} labelled, shipped mix | hip {med:.4f} ms [{lo:.4f}..{hi:.4f}] | '
                     f'per-frame torch loop on the device {ref_ms:.1f} ms | {ref_ms / med:.0f}x')
        print(lines[-1], flush=True)
        del ev, out
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
