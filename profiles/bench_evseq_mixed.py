"""Timing of the mixed-density event-sequence builder (rvt_amd.representations.EventSequenceBuilder(representation='mixed_density'):
rvt_event_sequence_mixed) on one MI355X.

The 1 Mpx sensor (720 x 1280 -> int8 10 x 360 x 640, 50 ms windows, cutoff 32 as the reference's mixeddensity_stack.yaml) at the
streaming shape (B 64, T 1) and a training-sized shape (B 24, T 21), each at a sparse and a dense event rate, streams generated on
the device (int16 x, y, p and int64 t: 14 B / event).  Beside each figure, from the same device tensors in the same process:
  * the stacked-histogram builder of the parent commit (uint8 20 x 360 x 640: twice the cells), and
  * a torch restatement of the reference's per-window route: torch.searchsorted, then per window the reference's arithmetic
    (data/utils/representations.py:185-217) at full resolution with the bin read off torch.frexp, put_(accumulate=True) into an
    int32 image, cumsum over the bins, the int8 cast, the clamp, and the odd pixels [:, 1::2, 1::2] (= downsample_ev_repr).
The mixed builder's output is checked equal to the restatement before timing.

  mixed ms    median of event-timed build_from_table calls (table and output already on the device) [min..max]
  hist ms     the same for the stacked-histogram builder
  torch ms    median of host-timed synchronised runs of the restatement (it synchronises with the host for the bounds)
  MB          modelled bytes of the mixed build: events of all windows read once (14 B each) + one scratch round trip (4 B written
              and 4 B read per cell) + planes written (1 B per cell); GB/s = MB / mixed ms

Usage: python profiles/bench_evseq_mixed.py [--calls 20] [--out FILE]"""
import argparse
import datetime
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from profiles.bench_evseq import BINS, H, RATES, SHAPES, STEP_US, W, event_median_ms, host_median_ms, make_stream  # noqa: E402
from rvt_amd import representations as R  # noqa: E402

CUTOFF_MIXED, CUTOFF_HIST = 32, 10


def torch_window(x, y, p, t):
    img = torch.zeros(BINS * H * W, dtype=torch.int32, device=t.device)
    if t.numel():
        tn = (t - t[0]) / torch.clamp(t[-1] - t[0], min=1)                       # int64 / int64 -> float32, as the reference
        tn = torch.clamp(tn, min=1e-6, max=1 - 1e-6)
        b = torch.clamp(BINS + torch.frexp(tn)[1] - 1, min=0).long()             # floor(BINS - log(tn) / log(1/2)), exactly
        img.put_(x.long() + W * y.long() + H * W * b, (p * 2 - 1).to(torch.int32), accumulate=True)
    full = torch.cumsum(img.view(BINS, H, W), 0, dtype=torch.int32).to(torch.int8)   # the int8 accumulator's wrap
    return torch.clamp(full, min=-CUTOFF_MIXED, max=CUTOFF_MIXED)[:, 1::2, 1::2]


def torch_route(streams, ts_end, out):
    for b, (x, y, p, t) in enumerate(streams):
        end = torch.searchsorted(t, ts_end, right=True).tolist()
        start = torch.searchsorted(t, ts_end - STEP_US, right=False).tolist()
        for w, (i0, i1) in enumerate(zip(start, end)):
            out[w, b].copy_(torch_window(x[i0:i1], y[i0:i1], p[i0:i1], t[i0:i1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# mixed-density event-sequence builder on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# 1 Mpx sensor {H} x {W} -> int8 {BINS} x {H // 2} x {W // 2} (stacked histogram: uint8 {2 * BINS} x {H // 2} x {W // 2}), 50 ms windows, '
             f'int16 x / y / p + int64 t; mixed / hist: median of {args.calls} event-timed calls [min..max]; torch: median of 3 host-timed synchronised runs',
             '# MB = events read once (14 B) + scratch round trip (8 B / cell) + planes written (1 B / cell) of the mixed build; GB/s = MB / mixed ms',
             '# shape   B  T  rate    Mev/window |       MB | mixed ms [min..max]      GB/s | hist ms [min..max]       hist/mixed | torch ms  torch/mixed']
    for shape, B, T in SHAPES:
        for rate, per_window in RATES:
            streams = [make_stream(per_window * T, T, 100 * B + b, dev) for b in range(B)]
            ts_end = 1_000_000 + STEP_US * torch.arange(1, T + 1, device=dev)
            eb = R.EventSequenceBuilder(BINS, H, W, CUTOFF_MIXED, downsample_by_2=True, window_us=STEP_US, representation='mixed_density')
            hb = R.EventSequenceBuilder(BINS, H, W, CUTOFF_HIST, True, downsample_by_2=True, window_us=STEP_US)
            out = torch.empty((T, B) + eb.get_shape(), dtype=torch.int8, device=dev)
            hout = torch.empty((T, B) + hb.get_shape(), dtype=torch.uint8, device=dev)
            bnd = torch.empty(B, T, 2, dtype=torch.int64, device=dev)
            table = eb.make_table(streams, ts_end)
            eb.build_from_table(table, out, bnd)
            want = torch_route(streams, ts_end, torch.empty_like(out))
            assert torch.equal(out, want), f'{shape} {rate}: the builder and the torch restatement differ'
            events = int((bnd[..., 1] - bnd[..., 0]).sum())
            mb = (14 * events + 9 * out.numel()) / 1e6
            med, lo, hi = event_median_ms(lambda: eb.build_from_table(table, out, bnd), args.calls)
            hmed, hlo, hhi = event_median_ms(lambda: hb.build_from_table(table, hout, bnd), args.calls)
            ref_ms = host_median_ms(lambda: torch_route(streams, ts_end, want))
            lines.append(f'{shape:7s} {B:3d} {T:2d}  {rate:6s} {events / (B * T) / 1e6:10.3f} | {mb:8.1f} | {med:7.3f} [{lo:.3f}..{hi:.3f}] {mb / med:7.0f} | '
                         f'{hmed:7.3f} [{hlo:.3f}..{hhi:.3f}] {hmed / med:8.2f}x | {ref_ms:8.2f} {ref_ms / med:8.1f}x')
            print(lines[-1], flush=True)
            del streams, table, out, hout, want, eb, hb
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
