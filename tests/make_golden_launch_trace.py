"""Launch traces of the backbone's Python host loop: which entry points of include/rvt_hip.h a step calls, in which order,
with which integer / float arguments and which pointers NULL.  A refactor of the host code must leave every trace unchanged.

    python -m tests.make_golden_launch_trace --backend emu        (CPU emulator build of the kernel sources)
    python -m tests.make_golden_launch_trace --backend hip        (MI355X, production route)

rewrites the cases of that backend in tests/golden/launch_trace.json (per case: launch count, {name: count} histogram, SHA-256
of the canonical sequence).  The recorder only wraps `rvt_amd._lib.call` and reads the header's prototypes (`_header.PROTOS`), so it
runs unchanged on any revision that derives its binding from the header; the golden is recorded on the revision BEFORE a change and tests/test_launch_trace.py replays it on the one after.
The host loop is forced (route_stage_driver = route_stage_driver_train = 0): the C-side drivers issue their launches inside one
library call, and tests/test_stage_driver.py ties them to the host loop bit for bit.

The detector tail (PAFPN, YOLOX head) has cases of its own, `--suite tail`, in tests/golden/tail_launch_trace.json: the tail's Python
decides nothing by backend, so one golden, recorded on the emulator, serves the emulator cases and the MI355X ones
(tests/test_tail_launch_trace.py).

One normalisation: `rb`, the tile factor rvt_lstm_scan3_fwd / _bwd take (absent when the golden was recorded: the library read it
from the tuning record), is found by its parameter name, taken out of the tuple and returned separately."""
import argparse
import ctypes
import hashlib
import json
import os

import torch

from rvt_amd import RNNDetector, _header, _lib, backbone_config, tuning
from tests import casegen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_trace.json')
MODES = ('train', 'nograd', 'stream')
HOST_LOOP = dict(route_stage_driver=0, route_stage_driver_train=0)
SCAN3 = ('rvt_lstm_scan3_fwd', 'rvt_lstm_scan3_bwd')

# ---- emulator cases: (casegen name, dtype) x tuning on top of TEST_GEOMETRY x mode ----
EMU_MODELS = [('micro', 'f32'), ('micro', 'bf16'), ('micro_mask', 'f32'), ('micro_dws_xh', 'f32'), ('micro_dws_hidden', 'f32'),
              ('micro_dh24', 'f32')]
EMU_TUNINGS = {'test_geometry': {}, 'fused_mlp': dict(route_fused_mlp=1),
               'op_by_op': dict(route_lstm_scan=0, route_fused_mlp=0, route_attn_block=0)}
# ---- MI355X cases on the production route: (size, dataset, dtype, T, B, extra tuning) x mode ----
OP_BY_OP = dict(route_fused_mlp=0, route_mlp_bwd_fused=0, route_attn_block=0, route_lstm_scan=0, route_lstm_scan_wgrad=0, lstm_scan3=0,
                mlp_stream=0, ln_linear=0, mlp_chain=0, dgrad_ln=0, route_conv_dgrad4=0, conv_wgrad_tn=0, attn_staged=0, stem=0,
                ppgemm=0)                                # = tests/test_production_route.py::OP_BY_OP (asserted by the test)
HIP_MODELS = {'base_b2': ('base', 'gen4', 'bf16', 3, 2, {}), 'base_b8': ('base', 'gen4', 'bf16', 3, 8, {}),
              'tiny_gen1_b8': ('tiny', 'gen1', 'bf16', 3, 8, {}), 'base_f32_b1': ('base', 'gen4', 'f32', 2, 1, {}),
              'base_b2_op_by_op': ('base', 'gen4', 'bf16', 3, 2, OP_BY_OP)}
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def emu_cases():
    return [(f'emu/{n}/{d}/{t}/{m}', n, d, t, m) for n, d in EMU_MODELS for t in EMU_TUNINGS for m in MODES]


def hip_cases():
    return [(f'hip/{k}/{m}', k, m) for k in HIP_MODELS for m in MODES]


def canonical(name, args):
    """(entry of the canonical sequence, rb or None)."""
    proto = _header.PROTOS[name]
    assert len(proto.argtypes) == len(args), (name, len(proto.argtypes), len(args))
    out, rb = [name], None
    for ty, arg, a in zip(proto.argtypes, proto.argnames, args):
        if name in SCAN3 and arg == 'rb':
            rb = int(a)
        elif isinstance(a, ctypes.Array):               # a host-side table (the head's level shapes, strides, maps): values, NULL-ness of pointers
            out.append([int(bool(v)) if a._type_ is ctypes.c_void_p else int(v) for v in a])
        elif ty is ctypes.c_void_p:
            out.append(int(a is not None and int(a) != 0))
        elif ty is ctypes.c_float:
            out.append(repr(float(a)))
        else:
            out.append(int(a))
    return out, rb


def record(fn):
    """Run fn() with every library launch recorded.  Returns (canonical sequence, [(name, C, rb)] of the lstm_scan3 launches)."""
    seq, rbs = [], []
    orig = _lib.call

    def rec(name, *args):
        entry, rb = canonical(name, args)
        seq.append(entry)
        if rb is not None:
            rbs.append((name, int(_header.LaunchArgs(name, args).C), rb))
        return orig(name, *args)
    _lib.call = rec
    try:
        fn()
    finally:
        _lib.call = orig
    return seq, rbs


def summary(seq):
    hist = {}
    for e in seq:
        hist[e[0]] = hist.get(e[0], 0) + 1
    return dict(count=len(seq), hist=dict(sorted(hist.items())), sha256=hashlib.sha256(json.dumps(seq).encode()).hexdigest())


def run_mode(m, xs, masks, mode):
    T = xs.shape[0]
    if mode == 'train':
        feats, _ = m.forward_sequence(xs, None, masks)
        sum(feats[s].float().sum() for s in (1, 2, 3, 4)).backward()
    elif mode == 'nograd':
        with torch.no_grad():
            m.forward_sequence(xs, None, masks)
    else:
        states = None
        with torch.no_grad():
            for t in range(T):
                _, states = m(xs[t], states, None if masks is None else masks[t])


def trace_emu(name, dt, tun, mode, dev=torch.device('cpu')):
    """Caller has installed the emulator library and TEST_GEOMETRY (tests/conftest.py does; main() below does)."""
    from tests.test_backbone import build_model
    with tuning.override(**HOST_LOOP, **EMU_TUNINGS[tun]):
        m = build_model(name, dev, DTYPES[dt])
        xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
        masks = torch.from_numpy(casegen.make_token_masks(name)).to(dev) if casegen.case_cfg(name)['enable_masking'] else None
        return record(lambda: run_mode(m, xs, masks, mode))


def trace_hip(key, mode, dev=torch.device('cuda', 0)):
    """Caller is on the production route (tuning.production())."""
    size, dataset, dt, T, B, extra = HIP_MODELS[key]
    with tuning.override(**HOST_LOOP, **extra):
        torch.manual_seed(0)
        m = RNNDetector(backbone_config(size, dataset), compute_dtype=DTYPES[dt]).to(dev)
        hw = (360, 640) if dataset == 'gen4' else (240, 304)
        g = torch.Generator(device=dev).manual_seed(3)
        xs = torch.randint(0, 11, (1 if mode == 'stream' else T, B, 20, *hw), generator=g, dtype=torch.uint8, device=dev)
        out = record(lambda: run_mode(m, xs, None, mode))
        torch.cuda.synchronize()
        return out


# ---- detector tail: (fixture, dtype) x mode, the same cases on either backend ----
TAIL_GOLDEN = os.path.join(os.path.dirname(GOLDEN), 'tail_launch_trace.json')
TAIL_FIXTURES = ('fpn_micro', 'head_micro')
TAIL_MODES = ('train2',             # training forward + backward twice in a row: arena zeroing and counters once per forward
              'nograd',             # eval forward under no_grad, twice: build + pack + BatchNorm affines, then plain reuse
              'eval_grad_frozen',   # eval forward, grad mode on, nothing requires grad: still one launch per unit
              'eval_grad',          # eval forward, grad mode on, parameters require grad: the unfused eval route
              'eval_bump')          # eval forward, a conv weight's and a BatchNorm weight's _version bumped, eval forward
TAIL_HEAD_MODES = ('detect',)       # YOLOXHead.detect_padded


def tail_cases():
    return [(f'tail/{n}/{d}/{m}', n, d, m) for n in TAIL_FIXTURES for d in DTYPES
            for m in TAIL_MODES + (TAIL_HEAD_MODES if n == 'head_micro' else ())]


def trace_tail(name, dt, mode, dev=torch.device('cpu')):
    """Caller has installed the library of `dev`'s backend."""
    if name == 'fpn_micro':
        from tests import casegen_fpn as cg
        from tests.test_fpn import _build
        m, _ = _build(name, dev, DTYPES[dt])
        xs = {s: torch.from_numpy(a).to(dev) for s, a in cg.make_inputs(name).items()}
        cots = [torch.from_numpy(a).to(dev) for a in cg.make_cotangents(name)]

        def train_step():
            outs = m({s: x.clone().requires_grad_(True) for s, x in xs.items()})
            sum((o.float() * ct).sum() for o, ct in zip(outs, cots)).backward()
        a_conv = m.bu_conv2
    else:
        from tests import casegen_head as cg
        from tests.test_head import _build
        m, _ = _build(name, dev, DTYPES[dt])
        xs = [torch.from_numpy(a).to(dev) for a in cg.make_inputs(name)]
        labels = torch.from_numpy(cg.make_labels(name, cg.CASES[name])).to(dev)

        def train_step():
            m([x.clone().requires_grad_(True) for x in xs], labels)[1]['loss'].backward()
        a_conv = m.stems[1]

    def run():
        if mode == 'train2':
            m.train()
            train_step()
            train_step()
            return
        m.eval()
        if mode == 'nograd':
            with torch.no_grad():
                m(xs)
                m(xs)
        elif mode == 'eval_grad_frozen':
            m.requires_grad_(False)
            m(xs)
        elif mode == 'eval_grad':
            m(xs)
        elif mode == 'eval_bump':
            with torch.no_grad():
                m(xs)
                a_conv.conv.weight.add_(0.0)
                a_conv.bn.weight.add_(0.0)
                m(xs)
        else:
            m.detect_padded(xs, 0.1, 0.45)
    out = record(run)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--backend', required=True, choices=['emu', 'hip'])
    ap.add_argument('--suite', default='backbone', choices=['backbone', 'tail'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.suite == 'tail':
        return main_tail(a)
    a.out = a.out or GOLDEN
    gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    gold = {k: v for k, v in gold.items() if not k.startswith(a.backend + '/')}
    if a.backend == 'emu':
        from tests.backends import emu_library
        _lib._install_test_library(emu_library())
        tuning.use(**tuning.TEST_GEOMETRY)
        for key, n, d, t, mode in emu_cases():
            gold[key] = summary(trace_emu(n, d, t, mode)[0])
            print(key, gold[key]['count'], gold[key]['sha256'][:12], flush=True)
    else:
        tuning.production()
        for key, k, mode in hip_cases():
            gold[key] = summary(trace_hip(k, mode)[0])
            print(key, gold[key]['count'], gold[key]['sha256'][:12], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(dict(sorted(gold.items())), f, indent=1)
        f.write('\n')


def main_tail(a):
    """One golden for both backends: written from the emulator by default; `--backend hip` is for comparing (--out elsewhere)."""
    if a.backend == 'emu':
        from tests.backends import emu_library
        _lib._install_test_library(emu_library())
    tuning.use(**tuning.TEST_GEOMETRY)
    dev = torch.device('cpu') if a.backend == 'emu' else torch.device('cuda', 0)
    gold = {}
    for key, n, d, mode in tail_cases():
        gold[key] = summary(trace_tail(n, d, mode, dev)[0])
        print(key, gold[key]['count'], gold[key]['sha256'][:12], flush=True)
    with open(a.out or TAIL_GOLDEN, 'w') as f:                       # one case per line
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in sorted(gold.items())) + '\n}\n')


if __name__ == '__main__':
    main()
