"""Frame cache format version 2 (masks only for non-empty 64-byte groups: rvt_frames_pack2 / _unpack2 / _gather2) against version 1
measured in the same run, on one MI355X.  Version 1's code is the parent's, so it is the yardstick; nothing here changes a default.

Shapes: the 1 Mpx training shape (T = 21, B = 24, 20 x 360 x 640) and Gen1 (T = 21, B = 8, 20 x 240 x 304).  Fills: uniformly
random non-zero bytes at 1 / 5 / 20 %, and "blobs": a 64-byte group is live with probability 0.1 or 0.3 and a byte of a live group
non-zero with probability 0.15.  The group occupancy of real recordings is NOT measured in this repository: the uniform fills are
version 2's worst case at a given density (every byte falls into a group of its own), the blobs stand for clustered data.
Per shape and fill, in one process, version 1 and version 2 alternating call by call:
  size     the store of both versions; asserted equal to packed_nbytes / packed_nbytes2
  pack     pack_frames into preallocated arrays (four launches each)
  unpack   unpack_frames of every frame through a permuted (T, B) index (one launch each)
  copy     out.copy_(x) of the dense tensor: one read plus one write of every byte
  h2d      the packed arrays from pinned host memory to the device followed by the unpack
  gather   the frames of a permuted index fetched from a pinned store by FrameGather: host wall time of table + copy + launch, and
           wall time until the staged set is ready (a synchronise behind the launch)
Median of device-event-timed calls (gather: host clock) after a warm-up, [min..max].  Both round trips are checked before timing.

Usage: python profiles/bench_framecache2.py [--calls 20] [--out FILE] [--only SHAPE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_framecache import alternate, host_pinned, random_planes  # noqa: E402
from rvt_amd import framecache as fc  # noqa: E402

SHAPES = (('1mpx', 21, 24, 20, 360, 640), ('gen1', 21, 8, 20, 240, 304))
FILLS = (('u1', None, 0.01), ('u5', None, 0.05), ('u20', None, 0.20), ('blob10', 0.1, 0.15), ('blob30', 0.3, 0.15))


def blob_planes(T, B, C, H, W, live, share, dev, seed):
    """A group of 64 consecutive bytes of a frame is live with probability `live`; a byte of a live group is non-zero with `share`."""
    g = torch.Generator(device=dev).manual_seed(seed)
    E = C * H * W
    Gf = (E + 63) // 64
    x = torch.empty(T, B, C, H, W, dtype=torch.uint8, device=dev)
    for t in range(T):                                          # step by step, like random_planes
        groups = (torch.rand(B, Gf, device=dev, generator=g) < live).repeat_interleave(64, dim=1)[:, :E].reshape(B, C, H, W)
        keep = groups & (torch.rand(B, C, H, W, device=dev, generator=g) < share)
        x[t] = torch.randint(1, 11, (B, C, H, W), device=dev, generator=g, dtype=torch.uint8) * keep
    return x


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(m):
    return f'{m[0]:7.3f} [{m[1]:.3f}..{m[2]:.3f}]'


def gather_times(host_store, index_np, calls, dev, on_gpu):
    """(host ms, ms until ready) of gathering the frames of index_np from a pinned store into a preallocated device set."""
    g = fc.FrameGather([host_store], dev)
    n = index_np.size
    out = g.empty(n, host_store.nnz(), host_store.ngroups()) if g.version == 2 else g.empty(n, host_store.nnz())
    table_dev = torch.zeros(n * g.cols, dtype=torch.int64, device=dev)
    host_ms, ready_ms = [], []
    for i in range(calls + 2):
        if on_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.gather(index_np, out, table_dev=table_dev)
        t1 = time.perf_counter()
        if on_gpu:
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            host_ms.append((t1 - t0) * 1e3)
            ready_ms.append((t2 - t0) * 1e3)
    out.check()
    return med(host_ms), med(ready_ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None, help='one shape name')
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
    lines = [f'# frame cache format 2 against format 1 on {where}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} calls [min..max], version 1 and version 2 alternating call by call in one process; v1 is the yardstick',
             '# fills: uN = N % uniformly random non-zero bytes; blobNN = NN % of the 64-byte groups live, 15 % of a live group\'s bytes non-zero',
             '# the group occupancy of real recordings is not measured in this repository',
             '# shape   T  B fill    nnz%  live groups% | what']
    for name, T, B, C, H, W in shapes:
        if args.only and name != args.only:
            continue
        F, E = T * B, C * H * W
        Gf = fc.geometry(E)[0]
        for fill, live, share in FILLS:
            seed = int(1000 * share) + F + (0 if live is None else int(100 * live))
            x = random_planes(T, B, C, H, W, share, dev, seed) if live is None else blob_planes(T, B, C, H, W, live, share, dev, seed)
            p1 = fc.pack_frames(x).trim()
            p2 = fc.pack_frames(x, version=2).trim()
            nnz, ng = p2.nnz(), p2.ngroups()
            assert p1.nnz() == nnz == int((x != 0).sum())
            assert p1.nbytes == fc.packed_nbytes(F, E, nnz) and p2.nbytes == fc.packed_nbytes2(F, E, ng, nnz)
            index = torch.randperm(F, device=dev).reshape(T, B)
            want = x.reshape((F,) + tuple(x.shape[2:]))[index.reshape(-1)].reshape(x.shape)
            out = torch.empty_like(x)
            for p in (p1, p2):
                out.fill_(0xA5)
                fc.unpack_frames(p, index, out=out)
                assert torch.equal(out, want), f'{name} {fill}: round trip differs'
                p.check()
            del want
            head = f'{name:5s} {T:3d} {B:2d} {fill:7s} {100 * nnz / (F * E):5.2f}  {100 * ng / (F * Gf):6.2f}'
            dense = F * E
            lines.append(f'{head} | size MB: dense {dense / 1e6:.1f}  v1 {p1.nbytes / 1e6:.2f}  v2 {p2.nbytes / 1e6:.2f}  v1/v2 {p1.nbytes / p2.nbytes:.3f} '
                         f'| per frame KB: v1 {p1.nbytes / F / 1e3:.1f}  v2 {p2.nbytes / F / 1e3:.1f}')
            print(lines[-1], flush=True)
            dst = torch.empty_like(x)
            h1 = fc.PackedFrames(p1.frame_shape, p1.dtype, *(host_pinned(t, on_gpu) for t in (p1.masks, p1.seg_offset, p1.value_base, p1.values, p1.status)))
            h2 = fc.PackedFrames2(p2.frame_shape, p2.dtype, *(host_pinned(t, on_gpu) for t in p2._arrays()))
            s1, s2 = fc.pack_frames(x, capacity=nnz), fc.pack_frames(x, capacity=nnz, mask_capacity=ng, version=2)   # where the transfers land

            def h2d(staged, host, keys):
                for k in keys:
                    getattr(staged, k).copy_(getattr(host, k), non_blocking=True)
                fc.unpack_frames(staged, index, out=out)

            res = alternate({'pack1': lambda: fc.pack_frames(x, out=p1), 'pack2': lambda: fc.pack_frames(x, out=p2),
                             'unpack1': lambda: fc.unpack_frames(p1, index, out=out), 'unpack2': lambda: fc.unpack_frames(p2, index, out=out),
                             'copy': lambda: dst.copy_(x),
                             'h2d1': lambda: h2d(s1, h1, ('masks', 'seg_offset', 'value_base', 'values')),
                             'h2d2': lambda: h2d(s2, h2, ('group_mask', 'seg_offset', 'grp_offset', 'value_base', 'mask_base', 'masks', 'values'))},
                            args.calls, on_gpu)
            lines.append(f'{head} | pack ms: v1 {fmt(res["pack1"])}  v2 {fmt(res["pack2"])}  v2/v1 {res["pack2"][0] / res["pack1"][0]:.2f} '
                         f'| unpack ms: v1 {fmt(res["unpack1"])}  v2 {fmt(res["unpack2"])}  v2/v1 {res["unpack2"][0] / res["unpack1"][0]:.2f} '
                         f'| copy_ ms {fmt(res["copy"])}')
            print(lines[-1], flush=True)
            lines.append(f'{head} | pinned h2d + unpack ms: v1 {fmt(res["h2d1"])}  v2 {fmt(res["h2d2"])}  v2/v1 {res["h2d2"][0] / res["h2d1"][0]:.2f}')
            print(lines[-1], flush=True)
            del dst, s1, s2
            idx = index.reshape(-1).cpu().numpy()
            g1 = gather_times(h1, idx, args.calls, dev, on_gpu)
            g2 = gather_times(h2, idx, args.calls, dev, on_gpu)
            for got, p in ((g1[2], p1), (g2[2], p2)):
                fc.unpack_frames(got, out=out.reshape((F,) + tuple(x.shape[2:])))
                assert torch.equal(out, x.reshape((F,) + tuple(x.shape[2:]))[index.reshape(-1)].reshape(x.shape)), f'{name} {fill}: gather differs'
            lines.append(f'{head} | gather of {F} frames from a pinned store: host ms v1 {fmt(g1[0])}  v2 {fmt(g2[0])} '
                         f'| until ready ms v1 {fmt(g1[1])}  v2 {fmt(g2[1])}  v2/v1 {g2[1][0] / g1[1][0]:.2f}')
            print(lines[-1], flush=True)
            del x, out, p1, p2, h1, h2, g1, g2
            if on_gpu:
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
