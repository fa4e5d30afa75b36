"""Gradient statistics and the non-finite step guard on the device (rvt_amd/optim.py: GradMonitor, AdamW.attach_monitor;
csrc/gradstats.hpp: rvt_grad_stats; csrc/optim.hpp: rvt_optim_step_guarded) against the torch-fp64 restatement of
tests/gradstats_ref.py, whose docstring derives the bound of the sum comparisons.  Counts, maxima and everything the guard touches
are compared exactly."""
import functools
import math

import numpy as np
import pytest
import torch

from rvt_amd import _header, _lib
from rvt_amd.optim import CHUNK, MAX_SCALARS, AdamW, GradMonitor, OneCycle
from tests.backends import backend  # noqa: F401
from tests.gradstats_ref import check_head, check_tensor, tensor_stats

SCHED = dict(total_steps=40, pct_start=0.25, div_factor=25.0, final_div_factor=1e4)
FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-41))
SPECIALS = [float('nan'), float('inf'), -float('inf'), DENORMAL, -0.0, FLT_MAX]

# ---- 1. tail shapes ------------------------------------------------------------------------------------------------------
# the sizes the issue names, a tensor whose 65 chunks wrap the fold's lane stride, and small ones up to 70 tensors with a gradient
# (the fold's 16 waves take tensors round-robin: every wave wraps, and the head's 64-row rounds wrap too)
TAIL_SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, 64 * CHUNK + 1] + [7 + 3 * i for i in range(58)]
UNALIGNED_N = CHUNK + 3          # the view one element into a larger buffer: p and g 4 bytes off a 16-byte boundary, two chunks
I_UNALIGNED, I_ZERO, I_NONE = len(TAIL_SIZES), len(TAIL_SIZES) + 1, len(TAIL_SIZES) + 2


@functools.lru_cache(maxsize=None)
def _tail_values():
    """CPU master copies (parameters, gradients; None = no gradient) and the fp64 reference of each, computed once."""
    gen = torch.Generator().manual_seed(31)
    ps = [torch.randn(n, generator=gen) for n in TAIL_SIZES]
    gs = [torch.randn(n, generator=gen) * 10.0 ** float(i % 7 - 4) for i, n in enumerate(TAIL_SIZES)]
    ps += [torch.randn(UNALIGNED_N, generator=gen), torch.randn(33, generator=gen), torch.randn(9, generator=gen)]
    gs += [torch.randn(UNALIGNED_N, generator=gen), torch.zeros(33), None]
    want = [None if g is None else tensor_stats(g, p) for g, p in zip(gs, ps)]
    return ps, gs, want


def _place(dev, values, unaligned):
    """Tensors on the device with these values; those in `unaligned` are views that start one element into a larger buffer."""
    out = []
    for i, v in enumerate(values):
        if v is None:
            out.append(None)
        elif i in unaligned:
            buf = torch.zeros(v.numel() + 8, device=dev)
            assert buf.data_ptr() % 16 == 0
            view = buf[1:1 + v.numel()]
            view.copy_(v)
            out.append(view)
        else:
            out.append(v.to(dev).clone())
    return out


def _make(dev, ps, gs, unaligned=(), ring=4, skip_nonfinite=True, **kw):
    params = [torch.nn.Parameter(t) for t in _place(dev, ps, unaligned)]
    for p, g in zip(params, _place(dev, gs, unaligned)):
        p.grad = g
    for i in unaligned:
        assert params[i].data_ptr() % 16 == 4 and params[i].grad.data_ptr() % 16 == 4
    names = [f'layer{i}.weight' for i in range(len(params))]
    opt = AdamW(params, lr=1e-3, clip_value=1.0, schedule=OneCycle(**SCHED), **kw)
    mon = opt.attach_monitor(zip(names, params), ring=ring, skip_nonfinite=skip_nonfinite)
    return params, names, opt, mon


def _tail_case(dev):
    ps, gs, want = _tail_values()
    return _make(dev, ps, gs, unaligned=(I_UNALIGNED,)) + (want,)


def test_tail_shapes(backend):
    params, names, opt, mon, want = _tail_case(backend)
    assert sum(g is not None for g in _tail_values()[1]) >= 65
    mon.observe()
    (rec,) = mon.read()
    assert rec['step'] == 0 and rec['scalars'] == [] and rec['nonfinite'] == 0
    assert list(rec['params']) == [n for n, w in zip(names, want) if w is not None]        # .grad None is left out
    for n, w in zip(names, want):
        if w is not None:
            check_tensor(n, rec['params'][n], w)
    z = rec['params'][names[I_ZERO]]
    assert (z['grad_abs_sum'], z['grad_sq_sum'], z['grad_abs_max'], z['nonfinite']) == (0.0, 0.0, 0.0, 0) and z['param_sq_sum'] > 0
    check_head('head', rec, [w for w in want if w is not None])
    # the head's sum is the tensor rows added in index order, exactly
    total = 0.0
    for n in rec['params']:
        total += rec['params'][n]['grad_sq_sum']
    assert rec['grad_sq_sum'] == total
    assert len(opt._chunks) == int(mon._first[-1]) == sum((w['numel'] + CHUNK - 1) // CHUNK for w in want if w is not None)


# ---- 2. special values ---------------------------------------------------------------------------------------------------
SP_SIZES = [2 * CHUNK + 5, UNALIGNED_N, 6]
# (tensor, element): element 0, the last element of a full chunk, the first element of a tail chunk, the last element of the tensor,
# inside the unaligned tensor (element path), and the last element of the unaligned tensor's full chunk
SP_POSITIONS = [(0, 0), (0, CHUNK - 1), (0, 2 * CHUNK), (0, 2 * CHUNK + 4), (1, 1234), (1, CHUNK - 1)]


@pytest.mark.parametrize('rot', range(len(SPECIALS)))
def test_special_values(backend, rot):
    """Position j carries SPECIALS[(j + rot) % 6]: over the six cases every value sits at every position once."""
    gen = torch.Generator().manual_seed(57 + rot)
    ps = [torch.randn(n, generator=gen) for n in SP_SIZES]
    gs = [torch.randn(n, generator=gen) for n in SP_SIZES]
    for j, (t, e) in enumerate(SP_POSITIONS):
        gs[t][e] = SPECIALS[(j + rot) % len(SPECIALS)]
    assert float(gs[0].abs()[torch.isfinite(gs[0])].max()) == FLT_MAX or float(gs[1].abs()[torch.isfinite(gs[1])].max()) == FLT_MAX
    params, names, opt, mon = _make(backend, ps, gs, unaligned=(1,))
    mon.observe()
    (rec,) = mon.read()
    want = [tensor_stats(g, p) for g, p in zip(gs, ps)]
    assert sum(w['nonfinite'] for w in want) == 3 and rec['nonfinite'] == 3                  # NaN, +inf, -inf
    for n, w in zip(names, want):
        check_tensor(n, rec['params'][n], w)
    check_head('head', rec, want)
    assert rec['grad_abs_max'] == FLT_MAX and math.isfinite(rec['grad_sq_sum']) and rec['grad_sq_sum'] >= FLT_MAX ** 2
    # a parameter's norm runs over ITS finite elements, whatever the gradient there holds
    for n, p in zip(names, ps):
        assert abs(rec['params'][n]['param_norm'] - float(p.double().norm())) <= 1e-12 * float(p.double().norm())


def test_denormal_and_negative_zero_alone(backend):
    """A tensor of denormals only, and one of -0.0 only: neither is flushed, counted as non-finite or given a sign."""
    ps = [torch.ones(5), torch.ones(5)]
    gs = [torch.full((5,), -DENORMAL), torch.full((5,), -0.0)]
    params, names, opt, mon = _make(backend, ps, gs)
    mon.observe()
    (rec,) = mon.read()
    d, z = rec['params'][names[0]], rec['params'][names[1]]
    assert d['grad_abs_max'] == DENORMAL and d['grad_abs_sum'] == 5 * DENORMAL and d['nonfinite'] == 0
    assert d['grad_sq_sum'] == 5 * DENORMAL * DENORMAL > 0
    assert z['grad_abs_max'] == 0.0 and math.copysign(1.0, z['grad_abs_max']) == 1.0 and z['grad_abs_sum'] == 0.0 and z['nonfinite'] == 0


# ---- 3. reproducibility --------------------------------------------------------------------------------------------------
def _ring_bytes(mon):
    return mon._buf.detach().cpu().clone()


def test_reproducible_and_grid_independent(backend):
    params, names, opt, mon, want = _tail_case(backend)
    params[3].grad[2] = float('nan')
    mon.observe()
    first = _ring_bytes(mon)
    assert mon.read()[0]['nonfinite'] == 1
    mon.observe()
    assert torch.equal(_ring_bytes(mon), first)
    for mb in (1, 3):
        mon._stats.zero_()
        mon._verdict.zero_()
        mon._empty_ring()                                     # as it was before the first call
        opt.max_blocks = mb
        mon.observe()
        assert torch.equal(_ring_bytes(mon), first), mb


# ---- 4. the guard --------------------------------------------------------------------------------------------------------
G_SIZES = [5, CHUNK + 1, 300, 2 * CHUNK + 5, CHUNK]


def _guard_values(seed, steps):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=gen) for n in G_SIZES]
    grads = [[torch.randn(n, generator=gen) * (3.0 if s % 2 == 0 else 1e-3) for n in G_SIZES] for s in range(steps)]
    return ps, grads


def _state(opt, params):
    return [t.detach().clone() for p in params for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])] if opt.state else \
        [p.detach().clone() for p in params]


def _same(a, b):
    """Bit equality (torch.equal treats NaN as unequal and -0.0 as equal to 0.0: compare the bit patterns)."""
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _set_grads(params, gs):
    for p, g in zip(params, gs):
        p.grad.copy_(g)


def test_guard_clean_gradients_step_like_the_plain_step(backend):
    ps, grads = _guard_values(5, 3)
    pa, _, opt_a, mon = _make(backend, ps, grads[0], unaligned=(2,))
    pb = [torch.nn.Parameter(t) for t in _place(backend, ps, (2,))]
    for p, g in zip(pb, _place(backend, grads[0], (2,))):
        p.grad = g
    opt_b = AdamW(pb, lr=1e-3, clip_value=1.0, schedule=OneCycle(**SCHED))
    calls, orig = [], _lib.call

    def rec(name, *args):
        calls.append(name)
        return orig(name, *args)
    _lib.call = rec
    try:
        for gs in grads:
            _set_grads(pa, gs)
            _set_grads(pb, gs)
            mon.observe()
            opt_a.step()
            opt_b.step()
    finally:
        _lib.call = orig
    assert calls == ['rvt_grad_stats', 'rvt_optim_step_guarded', 'rvt_optim_step'] * 3
    assert _same(_state(opt_a, pa), _state(opt_b, pb))
    assert opt_a.step_count() == opt_b.step_count() == 3 and mon.skipped_steps() == 0
    assert [r['step'] for r in mon.read(last=4)] == [0, 1, 2]


def test_guard_skips_a_nan_step_bit_for_bit(backend):
    ps, grads = _guard_values(6, 3)
    pa, names, opt_a, mon = _make(backend, ps, grads[0], unaligned=(2,))
    pb, _, opt_b, _ = _make(backend, ps, grads[0], unaligned=(2,), skip_nonfinite=False)       # the twin whose HOST skips the step
    mon.observe()
    opt_a.step()
    opt_b.step()
    before = _state(opt_a, pa)
    _set_grads(pa, grads[1])
    pa[3].grad[CHUNK + 7] = float('nan')                     # one NaN in one tensor
    mon.observe()
    opt_a.step()
    assert _same(_state(opt_a, pa), before)                  # every p, m and v of every tensor
    assert opt_a.step_count() == 1 and mon.skipped_steps() == 1
    rec = mon.read()[0]
    assert rec['step'] == 1 and rec['nonfinite'] == 1 and rec['params'][names[3]]['nonfinite'] == 1
    assert sum(r['nonfinite'] for r in rec['params'].values()) == 1
    for opt, params, m in ((opt_a, pa, mon), (opt_b, pb, None)):
        _set_grads(params, grads[2])
        if m is not None:
            m.observe()
        opt.step()
    assert _same(_state(opt_a, pa), _state(opt_b, pb))
    assert opt_a.step_count() == opt_b.step_count() == 2 and mon.skipped_steps() == 1
    assert mon.read()[0]['step'] == 1 and mon.read()[0]['nonfinite'] == 0          # the skipped observation's slot was taken again


def test_unguarded_monitor_records_and_steps(backend):
    ps, grads = _guard_values(7, 1)
    params, names, opt, mon = _make(backend, ps, grads[0], skip_nonfinite=False)
    params[1].grad[0] = float('nan')
    before = _state(opt, params)
    calls, orig = [], _lib.call

    def rec(name, *args):
        calls.append(name)
        return orig(name, *args)
    _lib.call = rec
    try:
        mon.observe()
        opt.step()
    finally:
        _lib.call = orig
    assert calls == ['rvt_grad_stats', 'rvt_optim_step']
    assert mon.read()[0]['nonfinite'] == 1 and opt.step_count() == 1 and mon.skipped_steps() == 0
    assert all(not torch.equal(p, b) for p, b in zip(params, before))


# ---- 5. ring, scalars and graph (GPU only) -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_observe_and_step_fill_the_ring():
    """[observe(scalars=(a, b)); step()] captured once with ring = 2 (after one eager warm-up step, which builds the tables) and
    replayed four times with gradients and scalars rewritten in place; the third replay carries an inf."""
    from rvt_amd.graph import GraphedStep
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    ps, grads = _guard_values(8, 5)
    grads[3][1][CHUNK] = float('inf')                        # warm-up = grads[0]; replays 1..4 = grads[1..4]; the third has the inf
    pa, names, opt_a, mon_a = _make(dev, ps, grads[0], unaligned=(2,), ring=2)
    pb, _, opt_b, mon_b = _make(dev, ps, grads[0], unaligned=(2,), ring=2)
    a, b = torch.zeros((), device=dev), torch.zeros(1, device=dev)

    def fn():
        mon_a.observe(scalars=(a, b))
        opt_a.step()
    gs = GraphedStep(fn, warmup=1)
    mon_b.observe(scalars=(a, b))
    opt_b.step()
    steps_seen, want_step = [], [1, 2, 3, 3]
    for r in range(4):
        _set_grads(pa, grads[r + 1])
        _set_grads(pb, grads[r + 1])
        a.fill_(0.5 + r)
        b.fill_(-2.0 * r)
        gs()
        mon_b.observe(scalars=(a, b))                        # the eager twin: its host reads the verdict and skips the step itself
        (eb,) = mon_b.read()
        if eb['nonfinite'] == 0:
            opt_b.step()
        (ea,) = mon_a.read()
        assert ea['step'] == eb['step'] == want_step[r] and ea['scalars'] == eb['scalars'] == [0.5 + r, -2.0 * r]
        assert ea['nonfinite'] == eb['nonfinite'] == (1 if r == 2 else 0)
        assert ea == eb
        steps_seen.append(sorted(x['step'] for x in mon_a.read(last=2)))
    torch.cuda.synchronize()
    assert steps_seen == [[0, 1], [1, 2], [2, 3], [2, 3]]   # slot = step % 2: device-counter order, wrapping
    heads = mon_a._buf[:2 * 64].cpu().numpy().view(_lib.row_dtype('RvtGradStatHead'))
    assert [int(s) for s in heads['step']] == [2, 3]
    assert mon_a.skipped_steps() == 1 and mon_b.skipped_steps() == 0
    assert opt_a.step_count() == opt_b.step_count() == 4
    assert _same(_state(opt_a, pa), _state(opt_b, pb))


# ---- 6. host contract ----------------------------------------------------------------------------------------------------
def test_grad_flow_is_the_reference_data_dict(backend):
    dev = backend
    gen = torch.Generator().manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)).to(dev)
    net[1].bias.requires_grad_(False)
    for name, p in net.named_parameters():
        if p.requires_grad and name != '2.weight':
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
    # the optimizer's groups order the parameters differently from named_parameters
    opt = AdamW([dict(params=[p for p in net[2].parameters()] + [p for p in net[0].parameters()]), dict(params=list(net[1].parameters()))])
    mon = opt.attach_monitor(net.named_parameters(), ring=1)
    mon.observe()
    got = mon.grad_flow()
    want = {'name': [], 'grad_abs': []}
    for name, p in net.named_parameters():                   # callbacks/utils/visualization.py: get_grad_flow_figure, in fp64
        if p.requires_grad and p.grad is not None:
            want['name'].append(name)
            want['grad_abs'].append(float(p.grad.detach().cpu().double().abs().mean()))
    assert got['name'] == want['name'] == ['0.weight', '0.bias', '1.weight', '2.bias']
    for g, w in zip(got['grad_abs'], want['grad_abs']):
        assert abs(g - w) <= 64 * 2.0 ** -52 * w              # at most 35 terms each


def test_attach_and_observe_reject(backend):
    dev = backend
    params = [torch.randn(6, device=dev).requires_grad_() for _ in range(2)]
    for p in params:
        p.grad = torch.ones_like(p)
    opt = AdamW(params)
    for ring in (0, -1, 1.5):
        with pytest.raises(ValueError, match='ring'):
            opt.attach_monitor([('a', params[0])], ring=ring)
    stranger = torch.randn(6, device=dev).requires_grad_()
    with pytest.raises(ValueError, match="'c' is not one of the optimizer's"):
        opt.attach_monitor([('a', params[0]), ('c', stranger)])
    assert opt._monitor is None
    mon = opt.attach_monitor([('a', params[0]), ('b', params[1])], ring=1)
    assert isinstance(mon, GradMonitor) and MAX_SCALARS == 8
    one = torch.zeros((), device=dev)
    with pytest.raises(ValueError, match='at most 8 scalars'):
        mon.observe(scalars=[one] * 9)
    with pytest.raises(TypeError, match='float32'):
        mon.observe(scalars=[one.double()])
    with pytest.raises(TypeError, match='float32'):
        mon.observe(scalars=[1.0])
    with pytest.raises(ValueError, match='one-element'):
        mon.observe(scalars=[torch.zeros(2, device=dev)])
    mon.observe(scalars=[one + i for i in range(8)])
    assert mon.read()[0]['scalars'] == [float(i) for i in range(8)]


def test_tensor_array_is_rebuilt_with_the_chunk_table(backend):
    dev = backend
    params = [torch.randn(n, device=dev).requires_grad_() for n in (5, CHUNK + 1, 300)]
    for p in params:
        p.grad = torch.randn_like(p)
    opt = AdamW(params, lr=1e-3)
    mon = opt.attach_monitor([(f'p{i}', p) for i, p in enumerate(params)], ring=2)
    assert mon._first is None and opt._chunks is None
    mon.observe()
    table, first = opt._chunks, mon._first
    assert first.tolist() == [0, 1, 3, 4]
    opt.step()
    for p in params:
        p.grad.mul_(0.5)                                      # new contents, same addresses
    mon.observe()
    opt.step()
    assert opt._chunks is table and mon._first is first
    assert [r['step'] for r in mon.read(last=2)] == [0, 1]
    keep = params[0].grad
    params[0].grad = None                                     # one gradient fewer: both rebuilt, by whichever call comes first
    opt.step()
    assert opt._chunks is not table and mon._first is not first and mon._first.tolist() == [0, 2, 3]
    assert mon.read(last=2) == []                             # the ring's rows were indexed by the old table: it starts empty
    table, first = opt._chunks, mon._first
    mon.observe()
    assert opt._chunks is table and mon._first is first
    (rec,) = mon.read()
    assert list(rec['params']) == ['p1', 'p2'] and rec['step'] == 3 and keep is not None


# ---- 7. header, exports, pricing -----------------------------------------------------------------------------------------
def test_records_match_the_c_compiler(tmp_path):
    """The two device-written records against a C compiler, like the table rows (tests/test_host.py)."""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert set(_header.RECORDS) == {'RvtGradStat', 'RvtGradStatHead'} and not set(_header.RECORDS) & set(_header.STRUCTS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rvt_hip.h"', 'int main(void) {']
    for n, st in _header.RECORDS.items():
        lines.append(f'    printf("{n} %zu\\n", sizeof({n}));')
        lines += [f'    printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f in _header.fields(st)]
    lines += ['    printf("MAX %d\\n", (int)RVT_GRADSTAT_MAX_SCALARS);', '    return 0;', '}']
    src, exe = tmp_path / 'records.c', tmp_path / 'records'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    c = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    for n, st in _header.RECORDS.items():
        dt = _lib.row_dtype(n)
        assert c[n] == ctypes.sizeof(st) == dt.itemsize == {'RvtGradStat': 32, 'RvtGradStatHead': 64}[n] and dt.itemsize % 8 == 0
        for f in dt.names:
            assert c[f'{n}.{f}'] == getattr(st, f).offset == dt.fields[f][1], (n, f)
    assert set(_lib.row_dtype('RvtGradStat').names) == {'abs_sum', 'sq_sum', 'param_sq_sum', 'abs_max', 'nonfinite'}
    assert set(_lib.row_dtype('RvtGradStatHead').names) == {'step', 'nonfinite', 'sq_sum', 'abs_max', 'n_scalars', 'scalars'}
    assert c['MAX'] == _header.ENUMS['RVT_GRADSTAT_MAX_SCALARS'] == 8 == _lib.row_dtype('RvtGradStatHead')['scalars'].shape[0]


def test_exports_and_pricing():
    import opmodel
    from tests.backends import emu_library
    lib = emu_library()
    for name in ('rvt_grad_stats', 'rvt_grad_stats_ws_bytes', 'rvt_optim_step_guarded'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.rvt_grad_stats_ws_bytes(10) == 320 and lib.rvt_grad_stats_ws_bytes(0) == 0
    n_chunks, n_tensors = 100, 7
    args = (1, n_chunks, 2, n_tensors, 3, None, 0, 4, n_tensors, 5, 64, 6, 7, 3200, 0, None)
    assert opmodel.model('rvt_grad_stats', args) == (0.0, opmodel.grad_stats_bytes(n_chunks * CHUNK, n_chunks, n_tensors))
    assert opmodel.grad_stats_bytes(1000, 1, 1) == 8.0 * 1000 + 40 + 2 * 32 + 32 + 64 + 8
    assert opmodel.model('rvt_optim_step_guarded', (1, n_chunks, 2, 1, 3, 4, 0, None)) == (0.0, opmodel.optim_step_bytes(n_chunks * CHUNK, n_chunks))
    assert opmodel.optim_step_bytes(1000, 1) == 28.0 * 1000 + 40
