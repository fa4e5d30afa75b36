"""The C-side stage driver (include/rvt_hip.h: rvt_stage_seq_fwd, csrc/capi_stage.hip) against the Python host loop of
rvt_amd/stage.py: the no-grad forward launches the same operators in the same order either way, so features and states must be
BIT-identical; and against the reference golden through the normal parity path (the driver is the default no-grad route)."""
import ctypes
import re

import pytest
import torch

from rvt_amd import _lib, stage_driver, tuning
from tests import casegen
from tests import make_golden_launch_trace as LT
from tests.backends import backend  # noqa: F401
from tests.test_backbone import build_model
from tests.test_route_record import _same

# route_lstm_scan = 0 on `micro` in bf16: stage 4 (C = 128) runs lstm_scan3, stages 1-3 one launch per step - the shared ConvLSTM tail
# of the two drivers in both of its forms
NO_SCAN = dict(route_lstm_scan=0)


def _has_both_tails(seq):
    names = {e[0] for e in seq}
    assert 'rvt_lstm_scan3_fwd' in names and 'rvt_lstm_fwd' in names, sorted(n for n in names if 'lstm' in n)


def _nograd_run(m, xs):
    """(sequence features, sequence states, streaming features per step, streaming states): the whole sequence at once from a zero
    state, then T = 1 calls with carried states."""
    feats_seq, st_seq = m.forward_sequence(xs, None)
    states = None
    per_step = []
    for t in range(xs.shape[0]):
        f, states = m(xs[t], states)
        per_step.append(f)
    return feats_seq, st_seq, per_step, states


@pytest.mark.parametrize('name,dtype,tun', [
    pytest.param('micro', torch.float32, {}, id='micro-dtype0'), pytest.param('micro', torch.bfloat16, {}, id='micro-dtype1'),
    pytest.param('base_qvga', torch.bfloat16, {}, id='base_qvga-dtype2'), pytest.param('micro_dh24', torch.float32, {}, id='micro_dh24-dtype3'),
    pytest.param('micro', torch.bfloat16, NO_SCAN, id='micro-bf16-routes_3_and_0')])
def test_stage_driver_matches_host_loop(backend, name, dtype, tun):
    dev = backend
    m = build_model(name, dev, dtype).eval()
    xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
    T = xs.shape[0]
    outs = {}
    for drv in (0, 1):
        with tuning.override(route_stage_driver=drv, **tun), torch.no_grad():
            if drv == 0 and tun:
                seq, _ = LT.record(lambda: outs.__setitem__(drv, _nograd_run(m, xs)))
                _has_both_tails(seq)
            else:
                outs[drv] = _nograd_run(m, xs)
    a, b = outs[0], outs[1]
    for s in (1, 2, 3, 4):
        assert torch.equal(a[0][s], b[0][s]), f'sequence features of stage {s} differ between driver and host loop'
        for t in range(T):
            assert torch.equal(a[2][t][s], b[2][t][s]), f'streaming features, step {t} stage {s}'
    for s in range(4):
        for x, y in zip(a[1][s] + a[3][s], b[1][s] + b[3][s]):
            assert torch.equal(x, y), f'states of stage {s + 1}'
    # streaming == sequence (same arithmetic; fp32 tight, bf16 the scan / per-step kernels differ in summation order)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for s in (1, 2, 3, 4):
        for t in range(T):
            want = b[0][s][t].float()
            err = (b[2][t][s].float() - want).abs().max().item() / max(want.abs().max().item(), 1e-9)
            assert err <= tol, (s, t, err)


def test_stage_driver_declines_what_it_does_not_cover(backend):
    """Token masks (and the DWS-ConvLSTM) stay on the operator-by-operator host loop: same results as before, no error."""
    dev = backend
    m = build_model('micro_mask', dev, torch.float32).eval()
    xs = torch.from_numpy(casegen.make_inputs('micro_mask')).to(dev)
    masks = torch.from_numpy(casegen.make_token_masks('micro_mask')).to(dev)
    with torch.no_grad():
        f1, _ = m.forward_sequence(xs, None, masks)
        with tuning.override(route_stage_driver=0):
            f0, _ = m.forward_sequence(xs, None, masks)
    for s in (1, 2, 3, 4):
        assert torch.equal(f0[s], f1[s])
    m2 = build_model('micro_dws_hidden', dev, torch.float32).eval()
    x2 = torch.from_numpy(casegen.make_inputs('micro_dws_hidden')).to(dev)
    with torch.no_grad():
        g1, _ = m2.forward_sequence(x2, None)
        with tuning.override(route_stage_driver=0):
            g0, _ = m2.forward_sequence(x2, None)
    for s in (1, 2, 3, 4):
        assert torch.equal(g0[s], g1[s])


# ---- training-side driver (round 6): rvt_stage_seq_train_fwd / rvt_stage_seq_bwd against the Python host loop -----------------------
def _train_run(name, dev, dtype, with_state):
    m = build_model(name, dev, dtype)
    xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
    cots = [torch.from_numpy(a).to(dev) for a in casegen.make_cotangents(name)]
    states = None
    if with_state:                       # incoming states with gradient flow into them (BPTT across calls within a batch)
        with torch.no_grad():
            _, st = m.forward_sequence(xs, None)
        states = [(h.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)) for h, c in st]
    feats, st_out = m.forward_sequence(xs, states)
    loss = sum((feats[s + 1].float() * cots[s]).sum() for s in range(4)) + sum(c.float().sum() * 0.5 for _, c in st_out)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    sgrads = [] if states is None else [t.grad.clone() for hc in states for t in hc]
    return feats, st_out, grads, sgrads


@pytest.mark.parametrize('name,dtype,with_state,tun', [
    pytest.param('micro', torch.float32, False, {}, id='micro-dtype0-False'), pytest.param('micro', torch.bfloat16, True, {}, id='micro-dtype1-True'),
    pytest.param('base_qvga', torch.bfloat16, False, {}, id='base_qvga-dtype2-False'), pytest.param('micro_dh24', torch.float32, True, {}, id='micro_dh24-dtype3-True'),
    pytest.param('tiny_gen1', torch.bfloat16, False, {}, id='tiny_gen1-dtype4-False'),
    pytest.param('micro', torch.bfloat16, True, NO_SCAN, id='micro-bf16-True-routes_3_and_0')])
def test_train_stage_driver_matches_host_loop(backend, name, dtype, with_state, tun):
    """The training forward + BPTT backward through the C-side stage driver (one library call per stage and direction) must be
    BIT-identical to the Python host loop over the same operators: features, final states, every parameter gradient, and the
    gradients of the incoming states."""
    dev = backend
    if dev.type == 'cpu' and name in ('base_qvga', 'tiny_gen1'):
        pytest.skip('minutes on the CPU emulator; runs on the GPU backend')
    outs = {}
    for drv in (0, 1):
        with tuning.override(route_stage_driver_train=drv, **tun):
            if drv == 0 and tun:
                seq, _ = LT.record(lambda: outs.__setitem__(drv, _train_run(name, dev, dtype, with_state)))
                _has_both_tails(seq)
            else:
                outs[drv] = _train_run(name, dev, dtype, with_state)
    a, b = outs[0], outs[1]
    for s in (1, 2, 3, 4):
        assert torch.equal(a[0][s], b[0][s]), f'features of stage {s}'
    for s in range(4):
        for x, y in zip(a[1][s], b[1][s]):
            assert torch.equal(x, y), f'final states of stage {s + 1}'
    for k in a[2]:
        if dev.type == 'cpu':
            assert torch.equal(a[2][k], b[2][k]), f'gradient of {k}: max diff {float((a[2][k] - b[2][k]).abs().max()):.3e}'
        else:       # on the GPU the LayerNorm / bias gradients fold through fp32 atomics: their order differs from run to run
            err = float((a[2][k] - b[2][k]).abs().max()) / max(float(a[2][k].abs().max()), 1e-30)
            assert err <= 2e-5, f'gradient of {k}: rel diff {err:.3e}'
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert torch.equal(x, y), f'gradient of incoming state tensor {i}'


def test_train_stage_driver_is_taken_and_declines(backend):
    """The driver is the default training route where covered (StageSaved.train is set), and hands token masks / the DWS-ConvLSTM back
    to the host loop without an error."""
    from rvt_amd import stage as stage_mod
    dev = backend
    seen = []
    orig = stage_mod.stage_seq_forward

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out[2] is not None and out[2].train is not None)
        return out
    stage_mod.stage_seq_forward = spy
    import rvt_amd.backbone as bb
    old = bb.stage_seq_forward
    bb.stage_seq_forward = spy
    try:
        for name, want in (('micro', True), ('micro_mask', None), ('micro_dws_hidden', False)):
            seen.clear()
            m = build_model(name, dev, torch.float32)
            xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
            masks = torch.from_numpy(casegen.make_token_masks(name)).to(dev) if name == 'micro_mask' else None
            feats, _ = m.forward_sequence(xs, None, masks)
            sum(feats[s].float().sum() for s in (1, 2, 3, 4)).backward()
            assert all(p.grad is not None for p in m.parameters())
            if want is True:
                assert all(seen) and len(seen) == 4, seen
            elif want is False:
                assert not any(seen), seen
            else:
                assert seen[0] is False and all(seen[1:]), seen       # the mask only touches stage 1
    finally:
        stage_mod.stage_seq_forward = orig
        bb.stage_seq_forward = old


# ---- the drivers' workspaces: sized by the carve itself, the size cached by what it depends on ----------------------------------------
def _flat(feats, states, grads=(), sgrads=()):
    out = {f'feat{s}': feats[s].detach() for s in (1, 2, 3, 4)}
    out.update({f'state{i}.{j}': t.detach() for i, hc in enumerate(states) for j, t in enumerate(hc)})
    out.update(grads)
    out.update({f'state_grad{i}': t for i, t in enumerate(sgrads)})
    return out


@pytest.mark.parametrize('first', ['defaults', 'override'])
def test_fwd_workspace_size_follows_the_tuning_record(backend, first, monkeypatch):
    """StageCall lives on the cached ModelWeights and outlives a tuning change; the size it caches depends on the routes, and the routes
    on the tuning record.  One model object, no-grad, T = B = 1, under two records in either order: the driver must run under both
    (a stale size made the library refuse: 'workspace of 5245696 bytes < rvt_stage_seq_fwd_ws_bytes = 8428288') and equal the host loop."""
    dev = backend
    monkeypatch.setattr(_lib, '_WS', {})              # (a workspace grown by an earlier test would hide a size that is too small)
    m = build_model('base_qvga', dev, torch.bfloat16).eval()
    xs = torch.from_numpy(casegen.make_inputs('base_qvga')).to(dev)[:1, :1]
    op_by_op = dict(route_attn_block=0, route_fused_mlp=0)
    with torch.no_grad():
        for tun in ([{}, op_by_op] if first == 'defaults' else [op_by_op, {}]):
            with tuning.override(**tun):
                got = _flat(*m.forward_sequence(xs, None))
                with tuning.override(route_stage_driver=0):
                    want = _flat(*m.forward_sequence(xs, None))
            for k in want:
                assert torch.equal(got[k], want[k]), f'{k} differs between driver and host loop under {tun}'


_PATTERN, _FRONT, _BEHIND = 0xA5, 64, 1 << 20


class _GuardedWorkspaces:
    """rvt_amd._lib.workspace for the kinds 'fwd' and 'train': exactly the n elements asked for, starting 64 bytes into a larger
    allocation whose 64 bytes in front and 1 MiB behind hold a byte pattern.  Other kinds pass through."""

    def __init__(self, monkeypatch):
        self.kinds, self.bufs = set(), []
        orig = _lib.workspace

        def workspace(kind, like, n, dtype, floor=0):
            if kind not in ('fwd', 'train'):
                return orig(kind, like, n, dtype, floor)
            assert dtype == torch.uint8
            self.kinds.add(kind)
            raw = torch.full((_FRONT + n + _BEHIND,), _PATTERN, dtype=torch.uint8, device=like.device)
            self.bufs.append((kind, n, raw))
            return _lib.stream_of(like), raw[_FRONT:_FRONT + n]
        monkeypatch.setattr(_lib, 'workspace', workspace)

    def check(self):
        for kind, n, raw in self.bufs:
            assert bool((raw[:_FRONT] == _PATTERN).all()), f'{kind} workspace of {n} bytes: written in front of it'
            assert bool((raw[_FRONT + n:] == _PATTERN).all()), f'{kind} workspace of {n} bytes: written behind it'
        self.bufs.clear()


def _every_driver_run(dev, dtype):
    """No-grad sequence + streaming pass with carried states, and a training step with incoming states, on `micro`."""
    m = build_model('micro', dev, dtype).eval()
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    with torch.no_grad():
        feats_seq, st_seq, per_step, st_stream = _nograd_run(m, xs)
    out = {f'seq.{k}': v for k, v in _flat(feats_seq, st_seq).items()}
    for t, f in enumerate(per_step):
        out.update({f'step{t}.feat{s}': f[s] for s in (1, 2, 3, 4)})
    out.update({f'stream.state{i}.{j}': x for i, hc in enumerate(st_stream) for j, x in enumerate(hc)})
    out.update({f'train.{k}': v for k, v in _flat(*_train_run('micro', dev, dtype, with_state=True)).items()})
    return out


@pytest.mark.parametrize('tun', [{}, dict(route_lstm_scan=0), dict(route_fused_mlp=0)], ids=['test_geometry', 'lstm_scan0', 'fused_mlp0'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_drivers_stay_inside_the_workspace_they_ask_for(backend, dtype, tun, monkeypatch):
    """The size functions are the carve on a counting Carver: a workspace of exactly that many bytes, at an address that is aligned to
    nothing beyond 64 bytes, must hold every piece.  Between them the three records visit every carve branch `micro` reaches
    (lstm_route 0 - 3, mlp_route 0 / 1, op-by-op attention, the prepack buffer)."""
    dev = backend
    with tuning.override(**tun):
        want = _every_driver_run(dev, dtype)
        guard = _GuardedWorkspaces(monkeypatch)
        got = _every_driver_run(dev, dtype)
        guard.check()
    assert guard.kinds == {'fwd', 'train'}, guard.kinds
    assert got.keys() == want.keys()
    _same(want, got, dev, f'guarded workspaces {tun}')


def test_fwd_driver_refuses_a_short_workspace(backend, monkeypatch):
    """One byte less than rvt_stage_seq_fwd_ws_bytes: refused with both numbers in the message, before any launch."""
    dev = backend
    seen = []
    orig = stage_driver.stage_seq_fwd
    monkeypatch.setattr(stage_driver, 'stage_seq_fwd', lambda *a: (seen.append(a), orig(*a))[1])
    m = build_model('micro', dev, torch.float32).eval()
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    with torch.no_grad():
        m.forward_sequence(xs, None)
    call, inp, _, _, T, B = seen[0]                   # stage 1
    lib, g = _lib.get_lib(), call.g
    n = int(lib.rvt_stage_seq_fwd_ws_bytes(ctypes.byref(call.desc), T, B))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    Hall = torch.full((T + 1, B, g.H, g.W, g.C), 7.0, dtype=call.dtype, device=dev)
    c_last = torch.full((B, g.H, g.W, g.C), 7.0, dtype=torch.float32, device=dev)

    def run(ws_bytes):
        return lib.rvt_stage_seq_fwd(ctypes.byref(call.desc), _lib.ptr(inp), None, None, _lib.ptr(Hall), _lib.ptr(c_last), _lib.ptr(ws), ws_bytes,
                                     T, B, _lib.stream_of(inp))
    assert run(n - 1) != 0
    msg = lib.rvt_last_error().decode()
    assert re.search(rf'\b{n - 1}\b.*\b{n}\b', msg), msg
    assert bool((Hall == 7).all()) and bool((c_last == 7).all()), 'a refused call launched something'
    assert run(n) == 0, lib.rvt_last_error().decode()
    assert not bool((Hall[1:] == 7).all())


def test_bwd_driver_refuses_a_short_workspace(backend, monkeypatch):
    """The same for rvt_stage_seq_bwd, through the binding: the host hands it one byte less than rvt_stage_seq_bwd_ws_bytes."""
    dev = backend
    orig, asked = _lib.workspace, []

    def short(kind, like, n, dtype, floor=0):
        if kind != 'train':
            return orig(kind, like, n, dtype, floor)
        asked.append(n)
        return _lib.stream_of(like), torch.empty(n - 1, dtype=dtype, device=like.device)
    monkeypatch.setattr(_lib, 'workspace', short)
    m = build_model('micro', dev, torch.float32)
    xs = torch.from_numpy(casegen.make_inputs('micro')).to(dev)
    feats, _ = m.forward_sequence(xs, None)
    with pytest.raises(RuntimeError, match='rvt_stage_seq_bwd failed') as e:
        sum(feats[s].float().sum() for s in (1, 2, 3, 4)).backward()
    assert len(asked) == 1 and re.search(rf'\b{asked[0] - 1}\b.*\b{asked[0]}\b', str(e.value)), (asked, str(e.value))
    # stage 4 is the first to run backward: its gradient bucket, zeroed before the call, has received nothing
    assert not bool(m._mw_cache.grads[3].flat.any()), 'a refused call launched something'
