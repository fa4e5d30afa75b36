"""Timing of the sparse frame cache (rvt_amd.framecache: rvt_frames_pack, rvt_frames_unpack) on one MI355X.

Shapes: the 1 Mpx training shape (T = 21, B = 24, 20 x 360 x 640) and Gen1 (T = 21, B = 8, 20 x 240 x 304), uniformly random
non-zero bytes at shares of 1 %, 5 % and 20 %.  Per shape and share, in one process, the variants alternating call by call:
  pack     pack_frames into preallocated arrays (four launches)
  unpack   unpack_frames of every frame through a permuted (T, B) index (one launch)
  copy     out.copy_(x) of the dense tensor: one read plus one write of every byte, the yardstick of the augmentation and
           event-prep benches
  h2d      the dense tensor from pinned host memory to the device
  packed   the packed arrays from pinned host memory to the device (four copies) followed by the unpack: what replaces h2d
GB/s = the bytes of opmodel.frames_pack_bytes / frames_unpack_bytes (with the measured nnz) over the time.  Median of
device-event-timed calls after a warm-up, [min..max].  The round trip is checked equal before timing.

Usage: python profiles/bench_framecache.py [--calls 20] [--out FILE]
       --rehearse runs the same code at a toy size on the CPU emulator build (tests/emu): it checks the script, its times mean nothing."""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opmodel  # noqa: E402
from rvt_amd import framecache as fc  # noqa: E402

SHAPES = (('1mpx', 21, 24, 20, 360, 640), ('gen1', 21, 8, 20, 240, 304))
SHARES = (0.01, 0.05, 0.20)


def timed_ms(fn, on_gpu):
    if on_gpu:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, calls, on_gpu, warmup=2):
    """{name: (median, min, max) ms}; one call of every variant per round, so that drift hits all of them alike."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    if on_gpu:
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(calls):
        for k, fn in variants.items():
            ts[k].append(timed_ms(fn, on_gpu))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def random_planes(T, B, C, H, W, share, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty(T, B, C, H, W, dtype=torch.uint8, device=dev)
    for t in range(T):                                          # step by step: the fp32 draw of a whole 2.3 GB tensor would be 9 GB
        keep = torch.rand(B, C, H, W, device=dev, generator=g) < share
        x[t] = torch.randint(1, 11, (B, C, H, W), device=dev, generator=g, dtype=torch.uint8) * keep
    return x


def host_pinned(t, on_gpu):
    h = t.cpu()
    return h.pin_memory() if on_gpu else h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
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
        dev, where, shapes = torch.device('cpu'), 'the CPU emulator (REHEARSAL: times mean nothing)', (('toy', 2, 3, 2, 24, 33),)
    lines = [f'# sparse frame cache on {where}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} event-timed calls [min..max], the variants alternating call by call in one process',
             '# GB/s = modelled bytes (opmodel.py: frames_pack_bytes / frames_unpack_bytes with the measured nnz) / time; copy_ moves 2 x dense bytes',
             '# shape   T  B   C   H   W  share  dense MB  packed MB  ratio | pack ms [min..max]     GB/s | unpack ms [min..max]   GB/s  unpack/copy | '
             'copy_ ms   GB/s | h2d dense ms  GB/s | h2d packed + unpack ms  vs dense']
    for name, T, B, C, H, W in shapes:
        F, E = T * B, C * H * W
        for share in SHARES:
            x = random_planes(T, B, C, H, W, share, dev, seed=int(1000 * share) + F)
            nnz = int((x != 0).sum())
            packed = fc.pack_frames(x, capacity=nnz)
            assert packed.check().nnz() == nnz
            index = torch.randperm(F, device=dev).reshape(T, B)
            out = torch.empty_like(x)
            fc.unpack_frames(packed, index, out=out)
            assert torch.equal(out, x.reshape((F,) + tuple(x.shape[2:]))[index.reshape(-1)].reshape(x.shape)), f'{name} {share}: round trip differs'
            packed.check()
            dst = torch.empty_like(x)
            hx = host_pinned(x, on_gpu)
            hp = fc.PackedFrames(packed.frame_shape, packed.dtype, *(host_pinned(t, on_gpu) for t in
                                                                      (packed.masks, packed.seg_offset, packed.value_base, packed.values, packed.status)))
            staged = fc.pack_frames(x, capacity=nnz)            # device arrays the packed transfer lands in

            def h2d_packed():
                for d, s in ((staged.masks, hp.masks), (staged.seg_offset, hp.seg_offset), (staged.value_base, hp.value_base),
                             (staged.values, hp.values)):
                    d.copy_(s, non_blocking=True)
                fc.unpack_frames(staged, index, out=out)

            res = alternate({'pack': lambda: fc.pack_frames(x, out=packed), 'unpack': lambda: fc.unpack_frames(packed, index, out=out),
                             'copy': lambda: dst.copy_(x), 'h2d': lambda: dst.copy_(hx, non_blocking=True), 'packed': h2d_packed},
                            args.calls, on_gpu)
            assert torch.equal(out, x.reshape((F,) + tuple(x.shape[2:]))[index.reshape(-1)].reshape(x.shape))
            dense, small = F * E, packed.nbytes
            pk, up, cp, hd, hpk = (res[k] for k in ('pack', 'unpack', 'copy', 'h2d', 'packed'))
            pack_gbs = opmodel.frames_pack_bytes(F, E, nnz) / pk[0] / 1e6
            unpack_gbs = opmodel.frames_unpack_bytes(F, E, nnz) / up[0] / 1e6
            lines.append(f'{name:6s} {T:3d} {B:2d} {C:3d} {H:3d} {W:3d}  {100 * nnz / dense:4.1f}%  {dense / 1e6:8.1f}  {small / 1e6:9.1f}  {dense / small:5.2f} | '
                         f'{pk[0]:7.3f} [{pk[1]:.3f}..{pk[2]:.3f}] {pack_gbs:6.0f} | {up[0]:7.3f} [{up[1]:.3f}..{up[2]:.3f}] {unpack_gbs:6.0f}  {up[0] / cp[0]:9.2f}x | '
                         f'{cp[0]:7.3f} {2 * dense / cp[0] / 1e6:6.0f} | {hd[0]:9.3f} {dense / hd[0] / 1e6:7.1f} | {hpk[0]:12.3f}  {hd[0] / hpk[0]:12.2f}x')
            print(lines[-1], flush=True)
            del x, out, dst, hx, hp, staged, packed
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
