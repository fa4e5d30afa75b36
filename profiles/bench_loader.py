"""Timing of the epoch loader's device work and host work (rvt_amd.loader, rvt_amd.framecache.unpack_augment) on one MI355X.

1. unpack_augment (one launch) against unpack_frames + augment_planes (two launches, a dense tensor between them: the yardstick,
   unchanged by the fused launch).  Shapes: the 1 Mpx training shape (T = 21, B = 24, 20 x 360 x 640) and Gen1 (T = 21, B = 8,
   20 x 240 x 304); 1 / 5 / 20 % uniformly random non-zero bytes (the inputs of profiles/bench_framecache.py); a permuted index;
   the shipped-probability augmentation mix of profiles/bench_augment.py, and pure identity.  The variants alternate call by call
   in one process, timed by device events; median [min..max] of the alternating samples.  The outputs are checked equal first.
   The loader's default route (fused=None) follows the 1 Mpx, 5 %, mix row: fused unless its median exceeds the two-launch median
   by more than the spread (max - min) of the two-launch samples.
2. Host time of one BatchLoader step (index, draw, tables; for resident='host' the staging gather and the copy as well) at the
   same two shapes, 5 % frames, RANDOM training batches, both residencies: wall time of a whole step, and of its host part alone.

Usage: python profiles/bench_loader.py [--calls 20] [--out FILE] [--skip-host]
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

import opmodel  # noqa: E402
from bench_augment import mixed_states, random_labels  # noqa: E402
from bench_framecache import alternate, random_planes  # noqa: E402
from rvt_amd import augment as A, framecache as fc  # noqa: E402
from rvt_amd.loader import BatchLoader, SequenceStore  # noqa: E402
from rvt_amd.types import DatasetSamplingMode, Mode  # noqa: E402
from tests import casegen_augment as cg  # noqa: E402

SHAPES = (('1mpx', 21, 24, 20, 360, 640), ('gen1', 21, 8, 20, 240, 304))
SHARES = (0.01, 0.05, 0.20)


def kernel_rows(shapes, calls, dev, on_gpu, lines):
    r = np.random.default_rng(0)
    verdict = None
    for name, T, B, C, H, W in shapes:
        F, E = T * B, C * H * W
        rows_np, count_np = random_labels(r, T, B, 8, H, W)
        labels = [[rows_np[t, b, :count_np[t, b]] if count_np[t, b] > 0 else None for t in range(T)] for b in range(B)]
        mixes = {'mix': mixed_states(B, H, W, labels), 'identity': [A.SpatialAugmentState() for _ in range(B)]}
        for share in SHARES:
            x = random_planes(T, B, C, H, W, share, dev, seed=int(1000 * share) + F)
            nnz = int((x != 0).sum())
            packed = fc.pack_frames(x, capacity=nnz)
            assert packed.check().nnz() == nnz
            del x
            index = torch.randperm(F, device=dev).reshape(T, B)
            dense, out1, out2 = (torch.empty((T, B, C, H, W), dtype=torch.uint8, device=dev) for _ in range(3))
            for what, states in mixes.items():
                it, _ = A.make_tables(states, (H, W), dev)

                def two():
                    fc.unpack_frames(packed, index, out=dense)
                    A.augment_planes(dense, it, out=out2)
                fc.unpack_augment(packed, index, it, out=out1)
                two()
                assert torch.equal(out1, out2), f'{name} {share} {what}: the two routes differ'
                res = alternate({'fused': lambda: fc.unpack_augment(packed, index, it, out=out1), 'two': two,
                                 'unpack': lambda: fc.unpack_frames(packed, index, out=dense),
                                 'augment': lambda: A.augment_planes(dense, it, out=out2)}, calls, on_gpu)
                fu, tw, up, au = (res[k] for k in ('fused', 'two', 'unpack', 'augment'))
                gbs = opmodel.frames_unpack_augment_bytes(F, E, nnz, B) / fu[0] / 1e6
                lines.append(f'{name:5s} {T:3d} {B:2d} {C:3d} {H:3d} {W:3d}  {100 * nnz / (F * E):4.1f}%  {what:8s} | fused {fu[0]:7.3f} [{fu[1]:.3f}..{fu[2]:.3f}] {gbs:6.0f} GB/s | '
                             f'two launches {tw[0]:7.3f} [{tw[1]:.3f}..{tw[2]:.3f}] (unpack {up[0]:.3f} + augment {au[0]:.3f}) | fused / two {fu[0] / tw[0]:5.2f}')
                print(lines[-1], flush=True)
                if name == '1mpx' and share == 0.05 and what == 'mix':
                    verdict = (fu[0], tw[0], tw[2] - tw[1])
            del packed, dense, out1, out2
    if verdict is not None:
        fu, tw, spread = verdict
        keep = fu <= tw + spread
        lines.append(f'# default route (1mpx, 5 %, mix): fused {fu:.3f} ms, two launches {tw:.3f} ms, spread {spread:.3f} ms -> '
                     f'{"fused" if keep else "two launches"} by the rule above')
        print(lines[-1], flush=True)


def host_rows(shapes, dev, on_gpu, lines, steps=6):
    lines.append('# one BatchLoader step, RANDOM training batches, 5 % frames: wall ms of a whole step (launches and the label read-back included), '
                 'and of its host part alone (index, draw, label packing; host residency: + staging gather and copy start)')
    augm = dict(random=cg.AUGM_CONFIG, stream=dict(cg.AUGM_CONFIG, zoom=dict(prob=0.8, zoom_out=dict(weight=1, factor=dict(min=1, max=1.2)))))
    for name, T, B, C, H, W in shapes:
        n_win, n_store = 2 * T, max(2, (B + 1) // 2)               # enough windows for B different samples without a 2.3 GB host copy per store
        r = np.random.default_rng(1)
        stores = []
        for k in range(n_store):
            x = random_planes(n_win, 1, C, H, W, 0.05, dev, seed=k)
            frames = fc.pack_frames(x.reshape(n_win, C, H, W)).to('cpu').trim()
            o2r = np.arange(T - 1, n_win, 2, dtype=np.int64)
            rows = [np.array([(f, W / 8 + i + r.uniform(0, W / 2), H / 8 + r.uniform(0, H / 2), W / 4, H / 4, i % 3, 1.0) for i in range(1 + f % 3)],
                             dtype=np.float32) for f in range(len(o2r))]
            stores.append(SequenceStore(frames, o2r, rows))
            del x
        for resident in ('device', 'host'):
            ld = BatchLoader(stores, B, T, DatasetSamplingMode.RANDOM, Mode.TRAIN, augm_config=augm, dataset_hw=(H, W), device=dev,
                             resident=resident, seed=0)
            host_ms, step_ms = [], []
            torch.manual_seed(0)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for _ in range(steps):
                    ld.epoch += 1
                    for samples in ld._random_batches(B):
                        t0 = time.perf_counter()
                        plan = ld._plan(DatasetSamplingMode.RANDOM, samples)
                        t1 = time.perf_counter()
                        ld._launch(plan, False)
                        if on_gpu:
                            torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        host_ms.append((t1 - t0) * 1e3)
                        step_ms.append((t2 - t0) * 1e3)
            host_ms, step_ms = host_ms[1:], step_ms[1:]             # the first step allocates
            lines.append(f'{name:5s} {T:3d} {B:2d} {C:3d} {H:3d} {W:3d}  resident={resident:6s} | host part {statistics.median(host_ms):7.3f} '
                         f'[{min(host_ms):.3f}..{max(host_ms):.3f}] | whole step {statistics.median(step_ms):7.3f} [{min(step_ms):.3f}..{max(step_ms):.3f}] '
                         f'over {len(step_ms)} steps')
            print(lines[-1], flush=True)
            del ld


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--rehearse', action='store_true')
    args = ap.parse_args()
    on_gpu = not args.rehearse
    if on_gpu:
        assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
        dev, where, shapes = torch.device('cuda', 0), torch.cuda.get_device_name(0), SHAPES
    else:
        from rvt_amd import _lib
        from tests.backends import emu_library
        _lib._install_test_library(emu_library())
        dev, where, shapes = torch.device('cpu'), 'the CPU emulator (REHEARSAL: times mean nothing)', (('toy', 2, 3, 2, 24, 48),)
    lines = [f'# epoch loader on {where}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} event-timed calls [min..max] in ms, the variants alternating call by call in one process; permuted (T, B) index',
             '# GB/s = modelled bytes (opmodel.frames_unpack_augment_bytes with the measured nnz) / fused time',
             '# shape   T  B   C   H   W  share  states   | one launch | unpack_frames + augment_planes | ratio']
    kernel_rows(shapes, args.calls, dev, on_gpu, lines)
    if not args.skip_host:
        host_rows(shapes, dev, on_gpu, lines)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
