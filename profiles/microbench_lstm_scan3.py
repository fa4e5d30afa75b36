"""Wide-stage ConvLSTM: one scan launch (csrc/lstm_scan3.hpp) against the per-step kernels it replaces, at the shapes of
RVT-Base stage 3 (M = 23040 tokens per step, C = 256, T = 21), RVT-Tiny stage 4 (M = 640) and, at C = 128, RVT-Base stage 2
(M = 92160) and RVT-Tiny stage 3 (M = 640 / 2560 at B = 2 / 8 on Gen1, 7680 at 1 Mpx).  Five timings per entry: median [min - max]."""
import sys, os, statistics, torch
sys.path.insert(0, os.getcwd())
from rvt_amd import ops, tuning
dev, dt = torch.device('cuda', 0), torch.bfloat16
def timeit(fn, n=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n
def five(fn):
    return [timeit(fn) for _ in range(5)]
med = statistics.median
fmt = lambda t: f'{med(t):.3f} [{min(t):.3f} - {max(t):.3f}]'
rnd = lambda *s: torch.randn(*s, device=dev).to(dt)
T = 21
for M, C in ((23040, 256), (640, 256), (92160, 128), (640, 128), (2560, 128), (7680, 128)):
    x = rnd(T, M, C)
    w = rnd(4 * C, 2 * C) * 0.05
    b = torch.zeros(4 * C, device=dev)
    wp, wtp = ops.lstm_scan3_pack(w)
    dH, dc_last = rnd(T, M, C), torch.randn(M, C, device=dev)
    dx, dz = torch.empty(T, M, C, device=dev, dtype=dt), torch.empty(T, M, 4 * C, device=dev, dtype=dt)
    dh0, dc0 = torch.empty(M, C, device=dev, dtype=dt), torch.empty(M, C, device=dev)
    c_last = torch.empty(M, C, device=dev)
    for rb in (1, 2):
        with tuning.override(lstm_scan3_rb256=rb, lstm_scan3_rb128=rb):
            rows = ops.lstm_scan3_rows(C, M)
            Hall = torch.zeros(T + 1, M, C, device=dev, dtype=dt)
            Cs, gs = torch.empty(T, rows, C, device=dev, dtype=dt), torch.empty(T, rows, 4 * C, device=dev, dtype=dt)
            tf = five(lambda: ops.lstm_scan3_fwd(x, Hall, None, c_last, Cs, wp, b, gs))
            tn = five(lambda: ops.lstm_scan3_fwd(x, Hall, None, c_last, None, wp, b, None))
            tb = five(lambda: ops.lstm_scan3_bwd(gs, Cs, None, dH, dc_last, wtp, dx, dz, dh0, dc0))
            print(f'M={M} C={C} rb={rb}: scan3 fwd {fmt(tf)} ms  no-grad {fmt(tn)}  bwd {fmt(tb)} ms', flush=True)
            if rb == 1: s3_train, s3_nograd = med(tf) + med(tb), med(tn)
    tp = timeit(lambda: ops.lstm_scan3_pack(w))
    # the per-step kernels
    xs, hs, cs_ = rnd(M, C), rnd(M, C), torch.randn(M, C, device=dev)
    perm_w = rnd(4 * C, 2 * C) * 0.05
    ho, co, go = torch.empty(M, C, device=dev, dtype=dt), torch.empty(M, C, device=dev), torch.empty(M, 4 * C, device=dev, dtype=dt)
    dzs, wt = rnd(M, 4 * C), rnd(2 * C, 4 * C) * 0.05
    dxs, dhs = torch.empty(M, C, device=dev, dtype=dt), torch.empty(M, C, device=dev, dtype=dt)
    dhin, dcr = rnd(M, C), torch.randn(M, C, device=dev)
    t1 = timeit(lambda: ops.lstm_fwd(xs, hs, cs_, perm_w, b, ho, co, go))
    t2 = timeit(lambda: ops.lstm_dgrad(dzs, wt, dxs, dhs))
    t3 = timeit(lambda: ops.lstm_gates_bwd(dhin, dhs, dcr, go, co, cs_, dzs))
    print(f'M={M} C={C}: pack {tp * 1e3:.1f} us;  per-step route x{T}: fwd {T * t1:.3f} ms, bwd {T * (t2 + t3):.3f} ms', flush=True)
    if C == 128:        # the register-resident-weight scan of lstm_scan.hpp (what stage 2 of RVT-Base ran before)
        Hall = torch.zeros(T + 1, M, C, device=dev, dtype=dt)
        Cs, gs = torch.empty(T, M, C, device=dev, dtype=dt), torch.empty(T, M, 4 * C, device=dev, dtype=dt)
        tf = five(lambda: ops.lstm_scan_fwd(x, Hall, None, c_last, Cs, w, b, gates_out=gs))
        tn = five(lambda: ops.lstm_scan_fwd(x, Hall, None, c_last, None, w, b, gates_out=None))
        tb = five(lambda: ops.lstm_scan_bwd(x, Hall, Cs, None, dH, dc_last, w, w.t().contiguous(), b, dx, dz, dh0, dc0, gates=gs))
        print(f'M={M} C={C}: lstm_scan.hpp (weights in registers, saved gates): fwd {fmt(tf)} ms  no-grad {fmt(tn)}  bwd {fmt(tb)} ms', flush=True)
        # the gate: scan3 at rb = 1 may exceed lstm_scan.hpp by no more than the min-max spread of lstm_scan.hpp's own timings
        train = [f + r for f, r in zip(tf, tb)]
        for what, s3, r, ts in (('fwd + bwd', s3_train, med(tf) + med(tb), train), ('no-grad fwd', s3_nograd, med(tn), tn)):
            spread = max(ts) - min(ts)
            print(f'M={M} C={C} gate {what}: scan3 rb=1 {s3:.3f}  lstm_scan.hpp {r:.3f}  delta {s3 - r:+.3f}  spread {spread:.3f}  '
                  f'{"PASS" if s3 <= r + spread else "FAIL"}', flush=True)
