"""Timing of the two ways host-resident frame stores reach the device in the epoch loader (rvt_amd.loader.BatchLoader,
resident='host') on one MI355X: staging='copy' (frames collected on the host into a pinned set, four copy_ calls: the yardstick)
against staging='gather' (one table row per frame, one rvt_frames_gather launch that reads the pinned stores itself).

Shapes: the 1 Mpx training shape (T = 21, B = 24, 20 x 360 x 640) and Gen1 (T = 21, B = 8, 20 x 240 x 304); 1 / 5 / 20 % uniformly
random non-zero bytes; 16 pinned stores of 2 T windows; RANDOM training batches (T consecutive windows per sample).  One process, the
two routes alternating step by step over the same batches, median [min..max] of --calls steps.  Per case:
  (1) host wall time of BatchLoader._plan (index, draw, label packing, staging start);
  (2) time from the start of _plan until the staging set's `ready` event has happened;
  (3) one gather launch alone on the batch's table against one pinned copy_ of the same number of bytes (event-timed), as GB/s of the
      packed bytes moved once;
  (4) a fixed main-stream sequence (unpack_frames + augment_planes at the shape) alone, and while the staging of the next batch runs
      on the side stream.
max_blocks: (2) with the gather's grid capped at 8 .. 256 workgroups; the best cap is measured three more times, the spread of those
three medians is the noise, and the default is the smallest cap whose median lies within that spread of the best (the largest such
cap over the cases).  staging=None resolves to 'gather' only if at every shape and fill (1) is lower than 'copy' by more than the
spread and (2) is not higher than 'copy' by more than the spread; otherwise 'copy' stays.

Usage: python profiles/bench_frames_gather.py [--calls 20] [--out FILE]
       --rehearse runs the same code at a toy size on the CPU emulator build (tests/emu): it checks the script, its times mean nothing."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_framecache import alternate, random_planes, timed_ms  # noqa: E402
from rvt_amd import augment as A, framecache as fc  # noqa: E402
from rvt_amd.loader import BatchLoader, SequenceStore  # noqa: E402
from rvt_amd.types import DatasetSamplingMode, Mode  # noqa: E402
from tests import casegen_augment as cg  # noqa: E402

SHAPES = (('1mpx', 21, 24, 20, 360, 640), ('gen1', 21, 8, 20, 240, 304))
SHARES = (0.01, 0.05, 0.20)
GRIDS = (8, 16, 32, 64, 128, 256)
N_STORES = 16
RND = DatasetSamplingMode.RANDOM


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(m):
    return f'{m[0]:8.3f} [{m[1]:.3f}..{m[2]:.3f}]'


def build_stores(T, C, H, W, share, dev):
    r = np.random.default_rng(1)
    n_win = 2 * T
    stores = []
    for k in range(N_STORES):
        x = random_planes(n_win, 1, C, H, W, share, dev, seed=100 * k + int(1000 * share))
        frames = fc.pack_frames(x.reshape(n_win, C, H, W)).to('cpu').trim()
        o2r = np.arange(T - 1, n_win, 2, dtype=np.int64)
        rows = [np.array([(f, W / 8 + i + r.uniform(0, W / 2), H / 8 + r.uniform(0, H / 2), W / 4, H / 4, i % 3, 1.0) for i in range(1 + f % 3)],
                         dtype=np.float32) for f in range(len(o2r))]
        stores.append(SequenceStore(frames, o2r, rows))
        del x
    return stores


def plan_step(ld, samples, on_gpu):
    """One _plan into the loader's next staging set: (host ms, ms until ready, the plan)."""
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = ld._plan(RND, samples)
    t1 = time.perf_counter()
    if plan['packed'].ready is not None:
        plan['packed'].ready.synchronize()
    t2 = time.perf_counter()
    ld.parts[RND]['flip'] ^= 1                                  # what _launch does: the next plan goes to the other set
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, plan


def case(name, T, B, C, H, W, share, calls, dev, on_gpu, lines):
    E = C * H * W
    augm = dict(random=cg.AUGM_CONFIG, stream=dict(cg.AUGM_CONFIG, zoom=dict(prob=0.8, zoom_out=dict(weight=1, factor=dict(min=1, max=1.2)))))
    stores = build_stores(T, C, H, W, share, dev)
    lds = {s: BatchLoader(stores, B, T, RND, Mode.TRAIN, augm_config=augm, dataset_hw=(H, W), device=dev, resident='host', seed=0, staging=s)
           for s in ('copy', 'gather')}
    batches = []
    while len(batches) < calls + 4:
        lds['copy'].epoch += 1
        batches += list(lds['copy']._random_batches(B))
    torch.manual_seed(0)
    head = f'{name:5s} {T:3d} {B:2d} {C:3d} {H:3d} {W:3d} {100 * share:4.0f}%'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # ---- (1), (2): the two routes alternating over the same batches
        ts = {s: ([], []) for s in lds}
        for i, samples in enumerate(batches[:calls + 2]):
            for s, ld in lds.items():
                host, ready, plan = plan_step(ld, samples, on_gpu)
                if i >= 2:                                      # the first use of either staging set allocates nothing but touches new pages
                    ts[s][0].append(host)
                    ts[s][1].append(ready)
        n = int(plan['index'].max()) + 1                      # (local index: the frames the last batch names)
        nnz = int(plan['packed'].dev.value_base[n])
        nbytes = fc.packed_nbytes(n, E, nnz)
        res = {s: (med(ts[s][0]), med(ts[s][1])) for s in lds}
        lines.append(f'{head} | {n} frames {nbytes / 1e6:7.1f} MB | (1) plan host ms: copy {fmt(res["copy"][0])}  gather {fmt(res["gather"][0])} | '
                     f'(2) plan -> ready ms: copy {fmt(res["copy"][1])}  gather {fmt(res["gather"][1])}')
        print(lines[-1], flush=True)

        # ---- max_blocks sweep of (2)
        g = lds['gather']
        sweep = {}
        for blocks in GRIDS:
            g.gather_blocks = blocks
            sweep[blocks] = statistics.median(plan_step(g, batches[i % len(batches)], on_gpu)[1] for i in range(calls))
        best = min(sweep, key=sweep.get)
        g.gather_blocks = best
        again = [statistics.median(plan_step(g, batches[i % len(batches)], on_gpu)[1] for i in range(calls)) for _ in range(3)]
        spread = max(again) - min(again)
        choice = min(b for b in GRIDS if sweep[b] <= sweep[best] + spread)
        g.gather_blocks = 0
        lines.append(f'{head} | max_blocks sweep of (2), median ms: ' + '  '.join(f'{b}: {sweep[b]:.3f}' for b in GRIDS) +
                     f' | best {best} again x3: ' + ' '.join(f'{a:.3f}' for a in again) + f' spread {spread:.3f} -> smallest within: {choice}')
        print(lines[-1], flush=True)

        # ---- (3): the launch alone against a pinned copy_ of the same number of bytes
        st = plan_step(g, batches[0], on_gpu)[2]['packed']
        n = int(torch.from_numpy(g._global_index(batches[0])).unique().numel())
        nbytes = fc.packed_nbytes(n, E, int(st.dev.value_base[n]))
        src = torch.zeros(nbytes, dtype=torch.uint8)
        src = src.pin_memory() if on_gpu else src
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        res3 = alternate({'gather': lambda: g.gatherer.launch(st.table_dev, n, st.dev), 'copy_': lambda: dst.copy_(src, non_blocking=True)},
                         calls, on_gpu)
        lines.append(f'{head} | (3) {n} frames {nbytes / 1e6:.1f} MB: gather launch {fmt(res3["gather"])} ms {nbytes / res3["gather"][0] / 1e6:6.1f} GB/s | pinned copy_ '
                     f'{fmt(res3["copy_"])} ms {nbytes / res3["copy_"][0] / 1e6:6.1f} GB/s')
        print(lines[-1], flush=True)
        del src, dst

        # ---- (4): a fixed main-stream sequence alone and beside the staging of the next batch
        out4 = {}
        for s, ld in lds.items():
            p = ld.parts[RND]
            p['flip'] = 0
            _, _, plan0 = plan_step(ld, batches[0], on_gpu)      # set 0 holds batch 0 and is only read from here on; flip is 1
            index_dev = torch.from_numpy(plan0['index']).to(dev)
            ev = p['bufs'][0].ev

            def seq():
                fc.unpack_frames(plan0['packed'].dev, index_dev, out=p['dense'])
                A.augment_planes(p['dense'].view(torch.uint8), p['it'], out=ev.view(torch.uint8))
            alone = alternate({'seq': seq}, calls, on_gpu)['seq']
            beside = []
            for i in range(calls):
                p['flip'] = 1
                if on_gpu:
                    torch.cuda.synchronize()
                ld._plan(RND, batches[1 + i % (len(batches) - 1)])               # the staging is on the side stream when this returns
                beside.append(timed_ms(seq, on_gpu))
            if on_gpu:
                torch.cuda.synchronize()
            out4[s] = (alone, med(beside))
        lines.append(f'{head} | (4) unpack + augment ms: ' + ' | '.join(
            f'{s}: alone {fmt(a)} beside staging {fmt(b)} x{b[0] / a[0]:.2f}' for s, (a, b) in out4.items()))
        print(lines[-1], flush=True)
    del lds, stores
    return res, spread, choice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--rehearse', action='store_true')
    ap.add_argument('--only', default=None, help='one shape name')
    args = ap.parse_args()
    on_gpu = not args.rehearse
    if on_gpu:
        assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
        dev, where, shapes = torch.device('cuda', 0), torch.cuda.get_device_name(0), SHAPES
    else:
        from rvt_amd import _lib
        from tests.backends import emu_library
        _lib._install_test_library(emu_library())
        dev, where, shapes = torch.device('cpu'), 'the CPU emulator (REHEARSAL: times mean nothing)', (('toy', 3, 3, 2, 24, 48),)
    lines = [f'# staging of host-resident frame stores on {where}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# {N_STORES} pinned stores of 2 T windows, RANDOM training batches; median [min..max] of {args.calls} steps, the routes alternating step by step',
             '# shape   T  B   C   H   W fill | what']
    verdict, choices = True, []
    for name, T, B, C, H, W in shapes:
        if args.only and name != args.only:
            continue
        for share in SHARES:
            res, spread, choice = case(name, T, B, C, H, W, share, args.calls, dev, on_gpu, lines)
            choices.append(choice)
            ok1 = res['gather'][0][0] < res['copy'][0][0] - spread
            ok2 = res['gather'][1][0] <= res['copy'][1][0] + spread
            verdict = verdict and ok1 and ok2
            lines.append(f'# {name} {100 * share:.0f}%: (1) lower than copy by more than the spread {spread:.3f}: {ok1}; (2) not higher than copy by more than it: {ok2}')
            print(lines[-1], flush=True)
            if on_gpu:
                torch.cuda.empty_cache()
    lines.append(f'# default max_blocks by the rule above: {max(choices)} (per case: {choices})')
    lines.append(f"# staging=None by the rule above: {'gather' if verdict else 'copy'}")
    print('\n'.join(lines[-2:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
