"""Timing of the on-device event-sequence builder (rvt_amd.representations.EventSequenceBuilder: rvt_event_sequence) on one MI355X.

The 1 Mpx sensor (720 x 1280 -> 20 x 360 x 640, 50 ms windows) at the streaming shape (B 64, T 1) and a training-sized shape
(B 24, T 21), each at a sparse and a dense event rate, streams generated on the device (int16 x, y, p and int64 t: 14 B / event).
Beside each figure the route the parent commit offers, built from the same device tensors in the same process: torch.searchsorted,
then per window StackedHistogram.construct at full resolution (its int64 conversion included: that is its interface) and
torch.nn.functional.interpolate(scale_factor=0.5, mode='nearest-exact').  The two outputs are checked equal before timing.

  hip ms      median of event-timed build_from_table calls (table and output already on the device) [min..max]
  build ms    median of host-timed synchronised build() calls (table built and copied to the device per call)
  per-window  median of host-timed synchronised runs of the parent route (it synchronises with the host for the bounds)
  MB          modelled bytes: events of all windows read once (14 B each) + one scratch round trip (4 B written and 4 B read per
              cell) + planes written (1 B per cell); GB/s = MB / hip ms
  Wc row      hip ms for each number of scratch images in flight; the default is marked with *

Usage: python profiles/bench_evseq.py [--calls 20] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rvt_amd import representations as R  # noqa: E402

H, W, BINS, CUTOFF, STEP_US = 720, 1280, 10, 10, 50_000
SHAPES = (('stream', 64, 1), ('train', 24, 21))
RATES = (('sparse', 100_000), ('dense', 1_000_000))            # events per 50 ms window: 2 and 20 Mev/s
WCS = (2, 4, 8, 16, 32, 64)


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


def host_median_ms(fn, n=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def make_stream(n, T, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(0, W, (n,), generator=g, device=dev, dtype=torch.int16)
    y = torch.randint(0, H, (n,), generator=g, device=dev, dtype=torch.int16)
    p = torch.randint(0, 2, (n,), generator=g, device=dev, dtype=torch.int16)
    t = torch.sort(torch.randint(0, STEP_US * T, (n,), generator=g, device=dev)).values + 1_000_000
    return x, y, p, t


def per_window_route(rep, streams, ts_end, out):
    for b, (x, y, p, t) in enumerate(streams):
        end = torch.searchsorted(t, ts_end, right=True).tolist()
        start = torch.searchsorted(t, ts_end - STEP_US, right=False).tolist()
        for w, (i0, i1) in enumerate(zip(start, end)):
            full = rep.construct(x[i0:i1], y[i0:i1], p[i0:i1], t[i0:i1])
            out[w, b].copy_(torch.nn.functional.interpolate(full[None], scale_factor=0.5, mode='nearest-exact')[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# event-sequence builder on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# 1 Mpx sensor {H} x {W} -> 20 x {H // 2} x {W // 2}, 50 ms windows, int16 x / y / p + int64 t; hip: median of {args.calls} event-timed '
             'calls [min..max]; build / per-window: median of 3 host-timed synchronised runs',
             '# MB = events read once (14 B) + scratch round trip (8 B / cell) + planes written (1 B / cell); GB/s = MB / hip ms',
             '# shape   B  T  rate    Mev/window |       MB | hip ms [min..max]        GB/s | build ms | per-window ms  per-window/hip']
    rep = R.StackedHistogram(BINS, H, W, CUTOFF, True)
    for shape, B, T in SHAPES:
        for rate, per_window in RATES:
            streams = [make_stream(per_window * T, T, 100 * B + b, dev) for b in range(B)]
            ts_end = 1_000_000 + STEP_US * torch.arange(1, T + 1, device=dev)
            eb = R.EventSequenceBuilder(BINS, H, W, CUTOFF, True, downsample_by_2=True, window_us=STEP_US)
            out = torch.empty((T, B) + eb.get_shape(), dtype=torch.uint8, device=dev)
            bnd = torch.empty(B, T, 2, dtype=torch.int64, device=dev)
            table = eb.make_table(streams, ts_end)
            eb.build_from_table(table, out, bnd)
            want = per_window_route(rep, streams, ts_end, torch.empty_like(out))
            assert torch.equal(out, want), f'{shape} {rate}: the builder and the per-window route differ'
            events = int((bnd[..., 1] - bnd[..., 0]).sum())
            cells = out.numel()
            mb = (14 * events + 9 * cells) / 1e6
            med, lo, hi = event_median_ms(lambda: eb.build_from_table(table, out, bnd), args.calls)
            build_ms = host_median_ms(lambda: eb.build(streams, ts_end, out=out, bounds_out=bnd))
            ref_ms = host_median_ms(lambda: per_window_route(rep, streams, ts_end, want))
            lines.append(f'{shape:7s} {B:3d} {T:2d}  {rate:6s} {events / (B * T) / 1e6:10.3f} | {mb:8.1f} | {med:7.3f} [{lo:.3f}..{hi:.3f}] {mb / med:7.0f} | '
                         f'{build_ms:8.3f} | {ref_ms:10.2f}   {ref_ms / med:8.1f}x')
            print(lines[-1], flush=True)
            row = []
            for wc in WCS:
                if wc > B * T:
                    continue
                e2 = R.EventSequenceBuilder(BINS, H, W, CUTOFF, True, downsample_by_2=True, window_us=STEP_US, max_windows_in_flight=wc)
                o2, _ = e2.build_from_table(table, out, bnd)
                assert torch.equal(o2, want)
                m2 = event_median_ms(lambda: e2.build_from_table(table, out, bnd), max(5, args.calls // 2))[0]
                row.append(f'{wc}{"*" if wc == R.DEFAULT_WINDOWS_IN_FLIGHT else ""}: {m2:.3f}')
                del e2
            lines.append(f'#   windows in flight (hip ms): ' + '   '.join(row))
            print(lines[-1], flush=True)
            del streams, table, out, want, eb
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
