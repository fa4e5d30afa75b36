"""The optimizer step on the device (rvt_amd/optim.py, csrc/optim.hpp: value clip + AdamW + OneCycleLR in one launch) against
torch.optim itself, which is the reference's optimizer (modules/detection.py:360-392): torch.optim.AdamW(foreach=False) +
clip_grad_value_ + OneCycleLR on the CPU.

TOLERANCE of every numeric comparison here (`_check`): the torch pieces run twice on identical inputs, in fp64 (the truth) and
in fp32 (the yardstick).  Over all elements of all tensors of the optimizer, and separately for the parameters, exp_avg and
exp_avg_sq,   max |ours - fp64|  <=  2 * max |torch fp32 - fp64|  +  one fp32 ulp at the largest magnitude of that quantity.
The factor 2: a second fp32 implementation with a different but legal operation order (torch's CPU lerp fuses a multiply-add,
its addcmul multiplies in another order) rounds differently, so bit equality is not demanded; a kernel that drops a term, is one
step off in the bias correction or the schedule, or clips the wrong way is outside the bound by orders of magnitude.
"""
import math

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR

from rvt_amd import _lib
from rvt_amd.optim import CHUNK, AdamW, OneCycle, _check_grad, from_train_config
from tests.backends import backend  # noqa: F401

CLIP, STEPS = 1.0, 12
SCHED = dict(total_steps=40, pct_start=0.25, div_factor=25.0, final_div_factor=1e4)
TAIL_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK + 1, 70001]


# ---- the torch side (CPU) -----------------------------------------------------------------------------------------------
def _torch_opt(params, groups, sched):
    """groups: list of (indices, dict(lr, weight_decay, betas, eps)); sched: OneCycle kwargs in the REFERENCE's meaning or None."""
    opt = torch.optim.AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups], foreach=False)
    sch = None
    if sched is not None:
        oc = OneCycle(**sched)
        sch = OneCycleLR(opt, max_lr=[kw['lr'] for _, kw in groups], total_steps=oc.total_steps, pct_start=oc.pct_start,
                         div_factor=oc.div_factor, final_div_factor=oc.torch_final_div_factor, cycle_momentum=False,
                         anneal_strategy='linear')
    return opt, sch


def _torch_steps(params, opt, sch, grads, clip):
    """grads: per step a list with one tensor or None per parameter."""
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = None if g is None else g.detach().cpu().to(p.dtype).clone()
        if clip is not None:
            torch.nn.utils.clip_grad_value_([p for p in params if p.grad is not None], clip, foreach=False)
        opt.step()
        if sch is not None:
            sch.step()


def _torch_run(dtype, p0, groups, sched, grads, clip):
    params = [p.detach().cpu().to(dtype).clone().requires_grad_() for p in p0]
    opt, sch = _torch_opt(params, groups, sched)
    _torch_steps(params, opt, sch, grads, clip)
    return params, opt


def _torch_state(params, opt, key):
    return [opt.state[p][key] if key in opt.state.get(p, {}) else None for p in params]


def _check(what, ours, truth, yard):
    """The tolerance of the module docstring over lists of tensors (None = no such tensor on either side)."""
    e_ours = e_yard = big = 0.0
    for o, t, y in zip(ours, truth, yard):
        assert (o is None) == (t is None), what
        if o is None:
            continue
        o64 = o.detach().cpu().double().reshape(-1)
        t64 = t.detach().double().reshape(-1)
        assert bool(torch.isfinite(o64).all()), what
        e_ours = max(e_ours, float((o64 - t64).abs().max()))
        e_yard = max(e_yard, float((y.detach().double().reshape(-1) - t64).abs().max()))
        big = max(big, float(t64.abs().max()))
    ulp = float(np.spacing(np.float32(big)))
    print(f'{what}: ours {e_ours:.3e}  torch fp32 {e_yard:.3e}  ulp {ulp:.3e}  bound {2 * e_yard + ulp:.3e}')
    assert e_ours <= 2 * e_yard + ulp, (what, e_ours, e_yard, ulp)


def _check_all(params, opt, t64, t32):
    (p64, o64), (p32, o32) = t64, t32
    _check('p', params, p64, p32)
    for key in ('exp_avg', 'exp_avg_sq'):
        ours = [opt.state[p][key] if key in opt.state.get(p, {}) else None for p in params]
        _check(key, ours, _torch_state(p64, o64, key), _torch_state(p32, o32, key))


def _make_grads(shapes, steps, seed, none_idx=()):
    """Gradient scales alternating between 3.0 (clipped at 1) and 1e-3, with values of exactly +clip, -clip and 0."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        row = []
        for i, shp in enumerate(shapes):
            if i in none_idx:
                row.append(None)
                continue
            t = torch.randn(shp, generator=g) * (3.0 if s % 2 == 0 else 1e-3)
            flat = t.reshape(-1)
            if flat.numel() >= 3:
                flat[0], flat[1], flat[-1] = CLIP, -CLIP, 0.0
            else:
                flat[0] = (CLIP, -CLIP, 0.0)[s % 3]
            row.append(t)
        out.append(row)
    return out


def _ours_steps(opt, params, grads, dev, gbufs=None):
    """Step `opt` with the given gradients (copied into persistent gradient storage, so the addresses stay put)."""
    for gs in grads:
        for i, (p, g) in enumerate(zip(params, gs)):
            if g is None:
                p.grad = None
            elif gbufs is not None and gbufs[i] is not None:
                gbufs[i].copy_(g)
                p.grad = gbufs[i]
            else:
                p.grad = g.to(dev).clone()
        opt.step()


# ---- 1. tail shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_blocks', [0, 3])
def test_matches_torch_at_tail_shapes(backend, max_blocks):
    """Sizes around the float4 width, the workgroup width and the chunk length; one parameter + gradient one element off a
    16-byte boundary (the scalar path); one parameter without a gradient (untouched, no state).  max_blocks = 3: 30 chunks on
    a grid of three workgroups, the grid-stride walk."""
    dev = backend
    g = torch.Generator().manual_seed(0)
    sizes = TAIL_SIZES + [5000, 7]                            # [-2]: the unaligned one, [-1]: grad = None
    una, non = len(sizes) - 2, len(sizes) - 1
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = _make_grads([(n,) for n in sizes], STEPS, 1, none_idx=(non,))
    groups = [(list(range(len(sizes))), dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8))]
    t64 = _torch_run(torch.float64, p0, groups, SCHED, grads, CLIP)
    t32 = _torch_run(torch.float32, p0, groups, SCHED, grads, CLIP)

    pbuf, gbuf = torch.zeros(sizes[una] + 1, device=dev), torch.zeros(sizes[una] + 1, device=dev)
    params, gbufs = [], []
    for i, p in enumerate(p0):
        if i == una:
            pbuf[1:].copy_(p)
            params.append(pbuf[1:].requires_grad_())
            gbufs.append(gbuf[1:])
        else:
            params.append(p.to(dev).clone().requires_grad_())
            gbufs.append(None if i == non else torch.zeros(sizes[i], device=dev))
    assert params[una].data_ptr() % 16 == 4 and gbufs[una].data_ptr() % 16 == 4
    opt = AdamW(params, lr=1e-2, weight_decay=0.01, clip_value=CLIP, schedule=OneCycle(**SCHED))
    opt.max_blocks = max_blocks
    _ours_steps(opt, params, grads, dev, gbufs)
    _check_all(params, opt, t64, t32)
    # the stored gradients are read only (clip_grad_value_ would have rewritten the clipped ones)
    for gb, gl in zip(gbufs, grads[-1]):
        if gb is not None:
            assert torch.equal(gb.cpu(), gl)
    assert float(max(gl.abs().max() for gl in grads[-2] if gl is not None)) > CLIP          # (there was something to clip)
    assert torch.equal(params[non].detach().cpu(), p0[non]) and len(opt.state.get(params[non], {})) == 0
    assert opt.step_count() == STEPS


# ---- 2. options ----------------------------------------------------------------------------------------------------------
def test_no_clip_no_decay_no_schedule(backend):
    dev = backend
    g = torch.Generator().manual_seed(2)
    sizes = [5, 1025, CHUNK + 1]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = _make_grads([(n,) for n in sizes], 6, 3)
    groups = [([0, 1, 2], dict(lr=3e-3, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8))]
    t64 = _torch_run(torch.float64, p0, groups, None, grads, None)
    t32 = _torch_run(torch.float32, p0, groups, None, grads, None)
    params = [p.to(dev).clone().requires_grad_() for p in p0]
    opt = AdamW(params, lr=3e-3, weight_decay=0.0)
    _ours_steps(opt, params, grads, dev)
    _check_all(params, opt, t64, t32)
    assert opt.current_lr() == [3e-3]


def test_two_parameter_groups(backend):
    dev = backend
    g = torch.Generator().manual_seed(4)
    sizes = [1023, 6, CHUNK + 1, 70]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = _make_grads([(n,) for n in sizes], 8, 5)
    groups = [([0, 1], dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)),
              ([2, 3], dict(lr=2e-3, weight_decay=0.2, betas=(0.8, 0.95), eps=1e-6))]
    t64 = _torch_run(torch.float64, p0, groups, SCHED, grads, CLIP)
    t32 = _torch_run(torch.float32, p0, groups, SCHED, grads, CLIP)
    params = [p.to(dev).clone().requires_grad_() for p in p0]
    opt = AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups], clip_value=CLIP, schedule=OneCycle(**SCHED))
    _ours_steps(opt, params, grads, dev)
    _check_all(params, opt, t64, t32)


def test_unsupported_options_raise(backend):
    dev = backend
    p = torch.zeros(8, device=dev, requires_grad=True)
    with pytest.raises(ValueError):
        AdamW([p], amsgrad=True)
    with pytest.raises(ValueError):
        AdamW([p], maximize=True)
    with pytest.raises(TypeError):
        AdamW([torch.zeros(8, device=dev, dtype=torch.bfloat16, requires_grad=True)])
    # (torch itself refuses a bf16 .grad on an fp32 leaf; the check step() runs on every gradient is what can be handed one)
    with pytest.raises(TypeError):
        _check_grad(p, torch.zeros(8, device=dev, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        _check_grad(p, torch.zeros(8, device=dev).to_sparse())
    _check_grad(p, torch.zeros(8, device=dev))


# ---- 3. schedule ---------------------------------------------------------------------------------------------------------
def _torch_lr_at(max_lr, oc, positions):
    """OneCycleLR's closed form at the given positions (its own get_lr at last_epoch = position; no stepping)."""
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=max_lr)
    sch = OneCycleLR(opt, max_lr=max_lr, total_steps=oc.total_steps, pct_start=oc.pct_start, div_factor=oc.div_factor,
                     final_div_factor=oc.torch_final_div_factor, cycle_momentum=False, anneal_strategy='linear')
    out = []
    for pos in positions:
        sch.last_epoch = pos
        sch._get_lr_called_within_step = True
        out.append(sch.get_lr()[0])
    return out


def _set_count(opt, p, k):
    """Put the device counter at k the public way: a torch-format state_dict with step = k."""
    sd = opt.state_dict()
    sd['state'] = {0: dict(step=torch.tensor(float(k)), exp_avg=torch.zeros_like(p).cpu(), exp_avg_sq=torch.zeros_like(p).cpu())}
    opt.load_state_dict(sd)


@pytest.mark.parametrize('total,pct,div,final_div,max_lr,positions', [
    (40, 0.25, 25.0, 1e4, 1e-2, list(range(40))),
    (25, 0.3, 25.0, 1e4, 1e-2, list(range(25))),             # fractional phase boundary at 6.5
    (400000, 0.005, 25.0, 1e4, 2e-4, [0, 1, 1998, 1999, 2000, 2001, 200000, 399998, 399999]),      # the shipped configuration
])
def test_schedule_matches_onecyclelr(backend, total, pct, div, final_div, max_lr, positions):
    dev = backend
    oc = OneCycle(total, pct, div, final_div)
    want = _torch_lr_at(max_lr, oc, positions)
    p = torch.ones(4, device=dev, requires_grad=True)
    opt = AdamW([p], lr=max_lr, weight_decay=1.0, schedule=oc)
    for pos, w in zip(positions, want):
        _set_count(opt, p, pos)
        got = opt.current_lr()[0]
        assert abs(got - w) <= 1e-12 * abs(w), (pos, got, w)
    _set_count(opt, p, total)                                 # one position past the end (torch raises one further on)
    assert opt.current_lr()[0] == oc.constants(max_lr)[2]
    assert abs(opt.current_lr()[0] - max_lr / final_div) <= 1e-12 * max_lr / final_div
    # ... and what the KERNEL used at a position: with a zero gradient and weight_decay = 1 a step leaves p = fl32(1 - lr), one
    # rounding of a value in [0.5, 1], i.e. within 2^-25 of 1 - lr (+ 1e-12 for the double arithmetic on both sides)
    for pos, w in list(zip(positions, want))[::max(1, len(positions) // 9)] + [(total, max_lr / final_div)]:
        _set_count(opt, p, pos)
        with torch.no_grad():
            p.fill_(1.0)
        p.grad = torch.zeros_like(p)
        opt.step()
        assert abs(float(p.detach()[0]) - (1.0 - w)) <= 2.0 ** -25 + 1e-12, (pos, float(p.detach()[0]), w)
        assert opt.step_count() == pos + 1


def test_from_train_config_reads_the_reference_keys(backend):
    dev = backend
    cfg = dict(learning_rate=2e-4, weight_decay=0, gradient_clip_val=1.0,
               lr_scheduler=dict(use=True, total_steps=400000, pct_start=0.005, div_factor=25, final_div_factor=10000))
    p = torch.zeros(4, device=dev, requires_grad=True)
    opt = from_train_config([p], cfg)
    assert opt.clip_value == 1.0 and opt.param_groups[0]['lr'] == 2e-4 and opt.param_groups[0]['weight_decay'] == 0
    init, mx, fin, warm, last = opt.schedule.constants(2e-4)
    assert (mx, warm, last) == (2e-4, 1999.0, 399999.0)
    assert math.isclose(init, 2e-4 / 25, rel_tol=1e-15) and math.isclose(fin, 2e-4 / 10000, rel_tol=1e-15)
    cfg['lr_scheduler']['use'] = False
    cfg['gradient_clip_val'] = None
    opt = from_train_config([p], cfg)
    assert opt.schedule is None and opt.clip_value is None and opt.current_lr() == [2e-4]


# ---- 4. state_dict both ways ---------------------------------------------------------------------------------------------
def test_state_dict_both_ways(backend):
    dev = backend
    g = torch.Generator().manual_seed(6)
    sizes = [5, 1025, CHUNK + 1]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = _make_grads([(n,) for n in sizes], 9, 7)
    kw = dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    groups = [([0, 1, 2], kw)]
    runs = {}
    for dt in (torch.float64, torch.float32):
        ps = [p.to(dt).clone().requires_grad_() for p in p0]
        opt, sch = _torch_opt(ps, groups, SCHED)
        _torch_steps(ps, opt, sch, grads[:3], CLIP)
        runs[dt] = (ps, opt, sch)
    # torch -> ours after three steps (the fp32 run's state), three more in all of them
    ps32, o32, s32 = runs[torch.float32]
    params = [p.detach().to(dev).clone().requires_grad_() for p in ps32]
    opt = AdamW(params, clip_value=CLIP, schedule=OneCycle(**SCHED), **kw)
    opt.load_state_dict(o32.state_dict())
    assert opt.step_count() == 3 and opt.param_groups[0]['lr'] == 1e-2
    assert abs(opt.current_lr()[0] - s32.get_last_lr()[0]) <= 1e-12 * s32.get_last_lr()[0]
    for ps, o, s in runs.values():
        _torch_steps(ps, o, s, grads[3:6], CLIP)
    _ours_steps(opt, params, grads[3:6], dev)
    t64, t32 = runs[torch.float64][:2], runs[torch.float32][:2]
    _check_all(params, opt, t64, t32)
    # ours -> a fresh torch.optim.AdamW (+ a OneCycleLR put at the same position), three more steps
    sd = opt.state_dict()
    assert all(float(st['step']) == 6.0 for st in sd['state'].values()) and len(sd['state']) == 3
    cont = [p.detach().cpu().clone().requires_grad_() for p in params]
    o_new, s_new = _torch_opt(cont, groups, SCHED)
    o_new.load_state_dict(sd)
    assert abs(o_new.param_groups[0]['lr'] - runs[torch.float32][2].get_last_lr()[0]) <= 1e-12
    s_new.last_epoch = 6
    for ps, o, s in runs.values():
        _torch_steps(ps, o, s, grads[6:9], CLIP)
    _torch_steps(cont, o_new, s_new, grads[6:9], CLIP)
    _check('p (ours -> torch)', cont, t64[0], t32[0])
    for key in ('exp_avg', 'exp_avg_sq'):
        _check(key + ' (ours -> torch)', _torch_state(cont, o_new, key), _torch_state(*t64, key), _torch_state(*t32, key))
    # disagreeing step entries
    bad = o32.state_dict()
    bad['state'][1]['step'] = bad['state'][1]['step'] + 1
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)
    assert opt.step_count() == 6


# ---- 5. one launch, stable table -----------------------------------------------------------------------------------------
def test_one_launch_and_stable_table(backend):
    dev = backend
    params = [torch.randn(n, device=dev).requires_grad_() for n in (5, CHUNK + 1, 300)]
    opt = AdamW(params, lr=1e-3, clip_value=CLIP, schedule=OneCycle(**SCHED))
    for p in params:
        p.grad = torch.randn_like(p)
    calls = []
    orig = _lib.call

    def rec(name, *args):
        calls.append(name)
        return orig(name, *args)
    _lib.call = rec
    try:
        opt.step()
        table = opt._chunks
        assert len(table) == 1 + 2 + 1
        for p in params:
            p.grad.mul_(0.5)                                  # new contents, same addresses
        opt.step()
        assert opt._chunks is table
        old = [p.grad for p in params]                        # (kept alive: the new gradients cannot land on their addresses)
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in params) and len(old) == 3
        keep = [torch.randn_like(p) for p in params]
        for p, k in zip(params, keep):
            p.grad = k
        opt.step()
        assert opt._chunks is not table
        params[0].grad = None                                 # one gradient fewer: three chunks
        opt.step()
        assert len(opt._chunks) == 3
    finally:
        _lib.call = orig
    assert calls == ['rvt_optim_step'] * 4 and opt.step_count() == 4


# ---- 6. version bump and the models' weight caches -----------------------------------------------------------------------
def _micro(dev):
    from tests.test_backbone import build_model
    return build_model('micro', dev, torch.float32)


def test_version_bump_repacks_inference_weights(backend):
    from tests import casegen
    dev = backend
    m = _micro(dev).eval()
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    with torch.no_grad():
        f0, _ = m.forward_sequence(xs, None)
        f0 = {k: v.clone() for k, v in f0.items()}
    params = list(m.parameters())
    before = [p._version for p in params]
    opt = AdamW(params, lr=1e-2, clip_value=CLIP)
    g = torch.Generator().manual_seed(8)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()
    assert all(p._version > b for p, b in zip(params, before))
    with torch.no_grad():
        f1, _ = m.forward_sequence(xs, None)
    assert any(not torch.equal(f1[k], f0[k]) for k in f0)
    fresh = _micro(dev).eval()
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        f2, _ = fresh.forward_sequence(xs, None)
    for k in f0:
        assert torch.equal(f1[k], f2[k]), k


# ---- 7. the backbone's own gradient buckets ------------------------------------------------------------------------------
def test_steps_the_backbone_gradient_buckets(backend):
    from tests import casegen
    dev = backend
    m = _micro(dev)
    m.zero_copy_grads = True
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    cots = [torch.from_numpy(a).to(dev) for a in casegen.make_cotangents('micro')]
    feats, _ = m.forward_sequence(xs, None)
    sum((feats[s + 1].float() * cots[s]).sum() for s in range(4)).backward()
    params = list(m.parameters())
    assert all(p.grad is not None for p in params)
    flats = [sg.flat for sg in m._mw_cache.grads]
    in_bucket = sum(any(f.data_ptr() <= p.grad.data_ptr() < f.data_ptr() + 4 * f.numel() for f in flats) for p in params)
    assert in_bucket == len(params)                           # the gradients ARE bucket views
    p0 = [p.detach().cpu().clone() for p in params]
    grads = [[p.grad.detach().cpu().clone() for p in params]] * 2
    kw = dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    groups = [(list(range(len(params))), kw)]
    t64 = _torch_run(torch.float64, p0, groups, SCHED, grads, CLIP)
    t32 = _torch_run(torch.float32, p0, groups, SCHED, grads, CLIP)
    opt = AdamW(params, clip_value=CLIP, schedule=OneCycle(**SCHED), **kw)
    opt.step()
    table = opt._chunks
    opt.step()
    assert opt._chunks is table
    _check_all(params, opt, t64, t32)


# ---- 8. hipGraph (GPU only) ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graphed_step_matches_eager_steps():
    """forward_sequence + BPTT backward + the optimizer step captured by GraphedStep.  The capture itself fails if step()
    synchronises or allocates.  N = 5 replays must leave every parameter, both moments and the device step count bit-identical to
    N eager steps of a second optimizer from the same start on the same inputs.  The backward folds some gradients with fp32
    atomics, whose order is free from run to run, so "the same inputs" of the eager optimizer are the gradients each replay
    produced (the captured step copies them out); everything the optimizer itself does is then deterministic."""
    from tests import casegen
    from rvt_amd.graph import GraphedStep
    _lib._install_test_library(None)
    dev = torch.device('cuda', 0)
    m = _micro(dev)
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    cots = [torch.from_numpy(a).to(dev) for a in casegen.make_cotangents('micro')]
    params = list(m.parameters())
    mk = dict(lr=1e-3, weight_decay=0.01, clip_value=1e-2, schedule=OneCycle(**SCHED))
    opt = AdamW(params, **mk)
    seen = [torch.zeros_like(p) for p in params]

    def step():
        feats, _ = m.forward_sequence(xs, None)
        torch.autograd.backward([feats[s + 1] for s in range(4)], [c.to(feats[s + 1].dtype) for s, c in enumerate(cots)])
        torch._foreach_copy_(seen, [p.grad for p in params])
        opt.step()
        opt.zero_grad(set_to_none=True)
    warm, N = 2, 5
    gs = GraphedStep(step, warmup=warm, models=(m,))          # the warm-up steps are REAL steps; the capture pass only records
    torch.cuda.synchronize()
    assert opt.step_count() == warm
    eager = [p.detach().clone().requires_grad_() for p in params]
    opt_e = AdamW(eager, **mk)
    opt_e.load_state_dict(opt.state_dict())
    for _ in range(N):
        gs()
        torch.cuda.synchronize()
        for p, g in zip(eager, seen):
            p.grad = g.clone()
        opt_e.step()
    torch.cuda.synchronize()
    assert any(float(g.abs().max()) > 1e-2 for g in seen)    # (the clip was active)
    for a, b in zip(params, eager):
        assert torch.equal(a, b)
        for key in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(opt.state[a][key], opt_e.state[b][key])
    assert torch.equal(opt._step, opt_e._step) and opt.step_count() == warm + N
    want = _torch_lr_at(1e-3, OneCycle(**SCHED), [warm + N])[0]
    assert abs(opt.current_lr()[0] - want) <= 1e-12 * want
    gs.close()
