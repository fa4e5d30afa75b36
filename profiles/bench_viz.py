"""Timing of the on-device detection preview (rvt_amd.viz: rvt_render_preview) on one MI355X.

Shapes: B = 64 frames of 20 x 360 x 640 (the 64-stream detector's frame buffer at 1 Mpx half scale) with two panels at scale 1 and
scale 2, and 8 frames of 20 x 240 x 304 (Gen1) with two panels at scale 4.  Every frame carries 12 detections and 6 labels.  Beside
each figure, two comparisons measured in the same process on the same device tensors:
  (a) pinned copy: host.copy_(planes, non_blocking=True) into pinned host memory, what a host-side renderer needs before it can
      draw anything (the detections and the image upload not counted);
  (b) torch base image: the grey / white / black image alone made with torch ops on the device (sum of each half of the channels
      in int32, sign, an index into three grey levels, expanded to RGB), no boxes, no tags, scale 1.
The three variants alternate call by call, so clock and thermal drift fall on all of them alike; each figure is the median of the
event-timed calls of its variant.  GB/s = modelled bytes (opmodel.render_preview_bytes: planes read once, image written once) /
time.  The kernel's output is checked against the numpy restatement (tests/viz_ref.py) on a small frame before anything is timed.
No time is asserted.

Usage: python profiles/bench_viz.py [--calls 20] [--out profiles/viz_bench.txt]"""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opmodel  # noqa: E402
from rvt_amd import viz  # noqa: E402
from tests import viz_ref  # noqa: E402

CASES = (('1mpx', 64, 20, 360, 640, 1, 'gen4'), ('1mpx', 64, 20, 360, 640, 2, 'gen4'), ('gen1', 8, 20, 240, 304, 4, 'gen1'))
N_DET, N_LAB = 12, 6


def boxes(r, F, n, H, W, classes):
    x, y = r.uniform(0, 0.8 * W, (F, n)), r.uniform(0, 0.8 * H, (F, n))
    w, h = r.uniform(4, W / 4, (F, n)), r.uniform(4, H / 4, (F, n))
    det = np.stack([x, y, x + w, y + h, r.random((F, n)), r.random((F, n)), r.integers(0, classes, (F, n))], axis=-1).astype(np.float32)
    lab = np.stack([np.zeros((F, n)), x, y, w, h, r.integers(0, classes, (F, n)), np.ones((F, n))], axis=-1).astype(np.float32)
    return det, lab


def torch_base_image(planes, levels):
    C = planes.shape[1]
    d = planes[:, C // 2:].sum(dim=1, dtype=torch.int32) - planes[:, :C // 2].sum(dim=1, dtype=torch.int32)
    return levels[torch.sign(d).long() + 1].unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()


def alternate(fns, calls, warmup=3):
    """Median / min / max ms of each callable, one call of each in turn per round."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def check_small(dev):
    r = np.random.default_rng(1)
    x = (r.integers(0, 5, (2, 20, 24, 48)) * (r.random((2, 20, 24, 48)) < 0.3)).astype(np.uint8)
    det, lab = boxes(r, 2, 3, 24, 48, 2)
    cd, cl = np.array([3, 2], dtype=np.int32), np.array([-1, 3], dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    got = viz.render_preview(t(x), t(det), t(cd), t(lab[:, :3]), t(cl), scale=2).cpu().numpy()
    want, _ = viz_ref.render(x, [(det, cd, 0), (lab[:, :3], cl, 1)], np.array(viz.PALETTES['gen1'], dtype=np.uint8),
                             viz.name_table(viz.LABELMAPS['gen1']), viz.glyph_table(), scale=2)
    assert np.array_equal(got, want.reshape(got.shape)), 'kernel and restatement differ'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'viz_bench.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    check_small(dev)
    lines = [f'# detection preview on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} event-timed calls [min..max], the three variants alternating call by call; {N_DET} detections + {N_LAB} labels per frame, two panels, tags on',
             '# GB/s = modelled bytes (opmodel.py: planes read once + image written once) / hip time',
             '# shape   F   C   H   W  s   MB planes  MB image | hip ms [min..max]       GB/s | pinned copy_ of the planes ms  copy/hip | torch base image ms (s = 1, no boxes)  torch/hip']
    r = np.random.default_rng(0)
    levels = torch.tensor([0, 127, 255], dtype=torch.uint8, device=dev)
    for name, F, C, H, W, s, dataset in CASES:
        planes = torch.from_numpy((r.integers(0, 6, (F, C, H, W)) * (r.random((F, C, H, W)) < 0.1)).astype(np.uint8)).to(dev)
        det_np, lab_np = boxes(r, F, N_DET, H, W, len(viz.LABELMAPS[dataset]))
        det, lab = torch.from_numpy(det_np).to(dev), torch.from_numpy(lab_np[:, :N_LAB].copy()).to(dev)
        cd = torch.full((F,), N_DET, dtype=torch.int32, device=dev)
        cl = torch.full((F,), N_LAB, dtype=torch.int32, device=dev)
        out = torch.empty(F, 2 * H * s, W * s, 3, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        host = torch.empty(planes.shape, dtype=torch.uint8, pin_memory=True)
        assert torch.equal(torch_base_image(planes, levels), viz.ev_repr_to_img(planes)), 'torch base image and kernel differ'
        (hip, lo, hi), (cp, _, _), (tb, _, _) = alternate(
            [lambda: viz.render_preview(planes, det, cd, lab, cl, dataset=dataset, scale=s, out=out, status=status),
             lambda: host.copy_(planes, non_blocking=True),
             lambda: torch_base_image(planes, levels)], args.calls)
        nbytes = opmodel.render_preview_bytes(F, C, H, W, 2, s)
        lines.append(f'{name:6s} {F:3d} {C:3d} {H:3d} {W:3d} {s:2d} {planes.numel() / 1e6:10.1f} {out.numel() / 1e6:9.1f} | {hip:7.3f} [{lo:.3f}..{hi:.3f}] '
                     f'{nbytes / hip / 1e6:7.0f} | {cp:28.3f} {cp / hip:8.1f}x | {tb:37.3f} {tb / hip:9.1f}x')
        print(lines[-1], flush=True)
        del planes, out, host
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
