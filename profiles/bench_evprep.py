"""Timing of the event preparation kernels (rvt_amd/csrc/evprep.hpp: rvt_event_time_repair, rvt_event_decode_dat) on one MI355X.

Per stream 2^24 and 2^27 events, B = 1 and B = 24 streams, generated on the device.  Three operations:
  repair         rvt_event_time_repair in place on int64 timestamps; 'steps': 2.5 % of the events stepped back (few stores),
                 'flat': a spike in front, so every timestamp is rewritten.  Each launch reads 8 B/event and the second stores up
                 to 8: 16 to 24 B/event move; the model counts 16
  decode         rvt_event_decode_dat, repair off: one launch, 8 B read and 14 B written per event
  decode+repair  the same with the repair in the pass: records read twice, stream written once, the modelled 30 B/event
Beside each figure, on the same device tensors in the same process:
  torch          torch.cummax (+ clamp to 0) per stream for the repair; the torch bit operations (& >> to int16 / int64) for the
                 decode; both for decode+repair
  copy           Tensor.copy_ of a buffer of half the modelled bytes (read once, written once)
Timestamps are restored before every timed repair call (outside the timed region).  GB/s = modelled bytes / kernel ms.

Usage: python profiles/bench_evprep.py [--calls 10] [--out FILE] [--max-log2 27]"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rvt_amd import representations as R  # noqa: E402
from rvt_amd.recordings import DatDecoder  # noqa: E402

W, H = 1280, 720
MODEL_BYTES = {'repair': 16, 'decode': 22, 'decode+repair': 30}


def event_median_ms(fn, calls, prep=None, warmup=2):
    ts = []
    for k in range(warmup + calls):
        if prep is not None:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def make_times(n, seed, dev, flat):
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.cumsum(torch.randint(0, 30, (n,), generator=g, device=dev, dtype=torch.int32), 0, dtype=torch.int64) % (2 ** 32 - 4096)
    t = torch.sort(t).values
    if flat:
        t[0] = 2 ** 32 - 1
    else:
        idx = torch.randint(1, n, (n // 40,), generator=g, device=dev)
        t[idx] -= torch.randint(1, 2000, (n // 40,), generator=g, device=dev)
        t.clamp_(min=0)
    return t


def make_records(t, seed):
    g = torch.Generator(device=t.device).manual_seed(seed)
    n = t.numel()
    w = (torch.randint(0, W, (n,), generator=g, device=t.device) | (torch.randint(0, H, (n,), generator=g, device=t.device) << 14)
         | (torch.randint(0, 16, (n,), generator=g, device=t.device) << 28))
    return t | (w << 32)                                  # little-endian {uint32 t; int32 w} as one int64


def torch_decode(rec, repair):
    t = rec & 0xffffffff
    w = rec >> 32
    x, y, p = (w & 16383).to(torch.int16), ((w >> 14) & 16383).to(torch.int16), ((w >> 28) & 1).to(torch.int16)
    if repair:
        t = torch.cummax(t, 0).values.clamp_(min=0)
    return x, y, p, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--max-log2', type=int, default=27)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# event preparation on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} event-timed calls [min..max]; modelled bytes per event: ' + ', '.join(f'{k} {v}' for k, v in MODEL_BYTES.items()),
             '# op             data   B  log2(n) |  kernel ms [min..max]        GB/s |  torch ms   torch/kernel |  copy ms   copy GB/s']

    def report(op, data, B, lg, n, ker, tor, cop):
        gb = MODEL_BYTES[op] * n * B / 1e6
        lines.append(f'{op:14s} {data:5s} {B:3d}  {lg:5d}   | {ker[0]:9.3f} [{ker[1]:.3f}..{ker[2]:.3f}] {gb / ker[0]:8.0f} | {tor[0]:9.3f}   {tor[0] / ker[0]:8.1f}x    | '
                     f'{cop[0]:8.3f}   {gb / cop[0]:8.0f}')
        print(lines[-1], flush=True)

    for lg in sorted({24, args.max_log2}):
        n = 2 ** lg
        for B in (1, 24):
            # ---- repair alone
            for data, flat in (('steps', False), ('flat', True)):
                orig = [make_times(n, 7 * b + lg, dev, flat) for b in range(B)]
                work = [t.clone() for t in orig]
                coord = torch.empty(n, dtype=torch.int16, device=dev)          # not read by the repair
                streams = [(coord, coord, coord, t) for t in work]
                table = R.EventSequenceBuilder(1, 1, 1, window_us=1).make_table(streams, torch.zeros(1, dtype=torch.int64, device=dev))
                ws = torch.empty(R.prep_ws_elems(B), dtype=torch.int64, device=dev)

                def restore():
                    for a, o in zip(work, orig):
                        a.copy_(o)
                R.repair_time(table, ws=ws)
                want = torch.cummax(orig[0], 0).values.clamp_(min=0)
                assert torch.equal(work[0], want), 'the repair and torch.cummax differ'
                del want
                ker = event_median_ms(lambda: R.repair_time(table, ws=ws), args.calls, restore)
                tor = event_median_ms(lambda: [torch.cummax(o, 0).values.clamp_(min=0) for o in orig], max(3, args.calls // 3))
                cop = event_median_ms(lambda: [a.copy_(o) for a, o in zip(work, orig)], args.calls)
                report('repair', data, B, lg, n, ker, tor, cop)
                del orig, work, streams, table
                torch.cuda.empty_cache()
            # ---- decode, without and with the repair in the pass
            recs = [make_records(make_times(n, 11 * b + lg, dev, False), 13 * b + lg) for b in range(B)]
            for op, repair in (('decode', False), ('decode+repair', True)):
                dec = DatDecoder(B, n, dev, repair=repair)
                dec.decode(recs)
                x, y, p, t = torch_decode(recs[0], repair)
                assert all(torch.equal(a, b) for a, b in zip(dec.streams[0], (x, y, p, t))), 'the decode and the torch route differ'
                del x, y, p, t
                ker = event_median_ms(dec.decode_in_place, args.calls, dec.reset)
                tor = event_median_ms(lambda: [torch_decode(r, repair) for r in recs], max(3, args.calls // 3))
                half = MODEL_BYTES[op] * n // 2
                src = torch.empty(half, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                cop = event_median_ms(lambda: [dst.copy_(src) for _ in range(B)], args.calls)
                report(op, 'steps', B, lg, n, ker, tor, cop)
                del dec, src, dst
                torch.cuda.empty_cache()
            del recs
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
