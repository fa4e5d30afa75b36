"""Timing of the on-device optimizer step (rvt_amd.optim.AdamW: rvt_optim_step = value clip + AdamW + OneCycleLR in one launch) on
one MI355X, on the parameter sets of the two shipped detectors (backbone + YOLOX PAFPN + head): RVT-Base 1 Mpx and RVT-Tiny Gen1,
random fp32 gradients in separately allocated tensors (what autograd leaves in .grad), the shipped training configuration
(config/general.yaml: lr 2e-4, weight_decay 0, clip 1.0 by value, OneCycle over 400 000 steps).  Beside each figure, measured in
the same process on the same device:
  (a) torch: clip_grad_value_ (foreach) + torch.optim.AdamW(fused=True, capturable=True).step() + OneCycleLR.step() on a copy of
      the parameters with gradients of the same contents - the three pieces a user assembles today;
  (b) copy: dst.copy_(src) of 14 bytes per parameter, i.e. 28 bytes per parameter moved, the floor for this traffic.
Traffic model: the step reads p, g, exp_avg, exp_avg_sq (16 bytes) and writes p, exp_avg, exp_avg_sq (12 bytes): 28 bytes per
parameter; GB/s = 28 * parameters / time.  "graphed": the same step captured in a hipGraph and replayed, i.e. without the host's
share (walking the parameter list, one library call).  All of them: median of device-event-timed calls on one stream after a warm-up (the events
bracket everything a call enqueues, so host time the device has to wait for is inside the figure).

Usage: python profiles/bench_optim.py [--calls 50] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from rvt_amd import fpn as F_, head as H_  # noqa: E402
from rvt_amd.optim import from_train_config  # noqa: E402

BYTES_PER_PARAM = 28
TRAIN_CFG = dict(learning_rate=2e-4, weight_decay=0, gradient_clip_val=1.0,
                 lr_scheduler=dict(use=True, total_steps=400000, pct_start=0.005, div_factor=25, final_div_factor=10000))


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


def detector_params(workload, dev):
    wl = dict(bench.WORKLOADS[workload])
    model = bench.build_model(wl, torch.bfloat16, dev)
    dims, strides = model.get_stage_dims((2, 3, 4)), model.get_strides((2, 3, 4))
    neck = F_.YOLOPAFPN(depth=0.67, in_channels=dims, compute_dtype=torch.bfloat16).to(dev)
    head = H_.YOLOXHead(num_classes=3, strides=strides, in_channels=dims, compute_dtype=torch.bfloat16).to(dev)
    return [p.detach().clone() for m in (model, neck, head) for p in m.parameters()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# optimizer step on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median of {args.calls} event-timed calls [min..max] on one stream; model: {BYTES_PER_PARAM} bytes per parameter (16 read + 12 written)',
             '# torch = clip_grad_value_ + AdamW(fused=True, capturable=True).step() + OneCycleLR.step();  copy = copy_ of 14 bytes per parameter (28 moved)',
             '# params set      tensors  parameters  MB moved | hip ms [min..max]        GB/s | graphed ms  GB/s | torch ms [min..max]      hip/torch | copy_ ms    GB/s  hip/copy | max |hip - torch| after 1 step']
    for name, workload in (('base_1mpx', 'base_1mpx'), ('tiny_gen1', 'tiny_gen1')):
        base = detector_params(workload, dev)
        n = sum(p.numel() for p in base)
        g = torch.Generator(device=dev).manual_seed(0)
        grads = [torch.randn(p.shape, device=dev, generator=g) * (3.0 if i % 2 else 1e-3) for i, p in enumerate(base)]
        ours = [p.clone().requires_grad_() for p in base]
        theirs = [p.clone().requires_grad_() for p in base]
        for p, q, gr in zip(ours, theirs, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt = from_train_config(ours, TRAIN_CFG)
        topt = torch.optim.AdamW(theirs, lr=TRAIN_CFG['learning_rate'], weight_decay=TRAIN_CFG['weight_decay'], fused=True, capturable=True)
        sp = TRAIN_CFG['lr_scheduler']
        sched = torch.optim.lr_scheduler.OneCycleLR(topt, max_lr=TRAIN_CFG['learning_rate'], total_steps=sp['total_steps'],
                                                    pct_start=sp['pct_start'], div_factor=sp['div_factor'],
                                                    final_div_factor=opt.schedule.torch_final_div_factor, cycle_momentum=False,
                                                    anneal_strategy='linear')

        def torch_step():
            torch.nn.utils.clip_grad_value_(theirs, TRAIN_CFG['gradient_clip_val'])
            topt.step()
            sched.step()
        opt.step()
        torch_step()
        torch.cuda.synchronize()
        diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(ours, theirs))
        src = torch.empty(n * BYTES_PER_PARAM // 2, dtype=torch.uint8, device=dev).random_()
        dst = torch.empty_like(src)
        hip = event_median_ms(opt.step, args.calls)
        graph = torch.cuda.CUDAGraph()                        # the same step replayed from a hipGraph: the device time alone
        with torch.cuda.graph(graph):
            opt.step()
        rep = event_median_ms(graph.replay, args.calls)
        tor = event_median_ms(torch_step, args.calls)
        cop = event_median_ms(lambda: dst.copy_(src), args.calls)
        nbytes = n * BYTES_PER_PARAM
        lines.append(f'{name:16s} {len(base):8d} {n:11d} {nbytes / 1e6:9.1f} | {hip[0]:7.3f} [{hip[1]:.3f}..{hip[2]:.3f}] {nbytes / hip[0] / 1e6:7.0f} | {rep[0]:7.3f} {nbytes / rep[0] / 1e6:7.0f} | '
                     f'{tor[0]:7.3f} [{tor[1]:.3f}..{tor[2]:.3f}]  {hip[0] / tor[0]:6.2f}x | {cop[0]:7.3f} {nbytes / cop[0] / 1e6:7.0f}  {hip[0] / cop[0]:6.2f}x | {diff:.2e}')
        print(lines[-1], flush=True)
        del base, grads, ours, theirs, opt, topt, src, dst, graph
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
