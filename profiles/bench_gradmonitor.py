"""Timing of the gradient monitor (rvt_amd.optim.GradMonitor: rvt_grad_stats = per-tensor gradient statistics + the non-finite
verdict, two launches) and of the step that obeys it (rvt_optim_step_guarded) on one MI355X, on the parameter sets of the two
shipped detectors (RVT-Base 1 Mpx, RVT-Tiny Gen1; profiles/bench_optim.py builds them), random fp32 gradients in separately
allocated tensors, the shipped training configuration.  Four candidates ALTERNATE in one process, one call each per round, so that
whatever else the device is doing falls on all of them alike:
  observe   GradMonitor.observe(): rvt_grad_stats over the optimizer's chunk table (8 bytes read per element + the partial rows)
  step      AdamW.step() with no monitor: rvt_optim_step (28 bytes per element)
  guarded   AdamW.step() with a monitor and a clean verdict: rvt_optim_step_guarded (the same traffic + 8 bytes per workgroup)
  torch     torch._foreach_norm over the same gradients + the norm of the stacked norms + isfinite of it, left on the device
            (no .item()): what a user writes today for "global norm + is it finite"; it has no per-tensor mean, maximum or count
Each figure: median [min..max] of device-event-timed calls after a warm-up; the events bracket everything a call enqueues, so host
time the device has to wait for is inside it.  GB/s = opmodel's bytes of the call over the median.

Usage: python profiles/bench_gradmonitor.py [--rounds 50] [--out FILE]"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import opmodel  # noqa: E402
from bench_optim import TRAIN_CFG, detector_params  # noqa: E402
from rvt_amd.optim import from_train_config  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, rounds, warmup=5):
    """{name: (median, min, max) ms}: one call of every candidate per round, in the given order."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'# gradient monitor on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__}',
             f'# median [min..max] ms of {args.rounds} event-timed calls per candidate, the candidates alternating call by call in one process',
             '# observe = rvt_grad_stats (2 launches); step = rvt_optim_step; guarded = rvt_optim_step_guarded with a clean verdict;',
             '# torch = _foreach_norm + norm of the stack + isfinite, no host read.  GB/s over the modelled bytes (opmodel.grad_stats_bytes / optim_step_bytes)',
             '# params set      tensors  parameters chunks | observe ms [min..max]   MB    GB/s | step ms [min..max]      GB/s | guarded ms [min..max]   guarded/step | torch ms [min..max]     observe/torch | graphed observe ms  GB/s']
    for name in ('base_1mpx', 'tiny_gen1'):
        base = detector_params(name, dev)
        n = sum(p.numel() for p in base)
        g = torch.Generator(device=dev).manual_seed(0)
        grads = [torch.randn(p.shape, device=dev, generator=g) * (3.0 if i % 2 else 1e-3) for i, p in enumerate(base)]
        plain = [p.clone().requires_grad_() for p in base]
        watched = [p.clone().requires_grad_() for p in base]
        for p, q, gr in zip(plain, watched, grads):
            p.grad, q.grad = gr.clone(), gr.clone()
        opt_plain, opt_guard = from_train_config(plain, TRAIN_CFG), from_train_config(watched, TRAIN_CFG)
        mon = opt_guard.attach_monitor([(f'p{i}', p) for i, p in enumerate(watched)], ring=64, skip_nonfinite=True)
        loss = torch.ones((), device=dev)
        tg = [q.grad for q in watched]

        def torch_stats():
            norms = torch._foreach_norm(tg)
            return torch.isfinite(torch.linalg.vector_norm(torch.stack(norms)))
        fns = {'observe': lambda: mon.observe(scalars=(loss,)), 'step': opt_plain.step, 'guarded': opt_guard.step, 'torch': torch_stats}
        t = alternate(fns, args.rounds)
        assert mon.skipped_steps() == 0 and mon.read()[0]['nonfinite'] == 0
        graph = torch.cuda.CUDAGraph()                        # the observation replayed from a hipGraph: the device time alone
        with torch.cuda.graph(graph):
            mon.observe(scalars=(loss,))
        rep = alternate({'graphed': graph.replay}, args.rounds)['graphed']
        n_chunks, n_tensors = len(opt_guard._chunks), len(mon._rows)
        ob, sb = opmodel.grad_stats_bytes(n, n_chunks, n_tensors), opmodel.optim_step_bytes(n, n_chunks)
        o, s, gd, to = t['observe'], t['step'], t['guarded'], t['torch']
        lines.append(f'{name:16s} {len(base):8d} {n:11d} {n_chunks:6d} | {o[0]:7.3f} [{o[1]:.3f}..{o[2]:.3f}] {ob / 1e6:6.1f} {ob / o[0] / 1e6:7.0f} | '
                     f'{s[0]:7.3f} [{s[1]:.3f}..{s[2]:.3f}] {sb / s[0] / 1e6:7.0f} | {gd[0]:7.3f} [{gd[1]:.3f}..{gd[2]:.3f}]  {gd[0] / s[0]:6.3f}x | '
                     f'{to[0]:7.3f} [{to[1]:.3f}..{to[2]:.3f}]  {o[0] / to[0]:6.2f}x | {rep[0]:7.3f} {ob / rep[0] / 1e6:7.0f}')
        print(lines[-1], flush=True)
        del base, grads, plain, watched, opt_plain, opt_guard, mon, graph, tg
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
