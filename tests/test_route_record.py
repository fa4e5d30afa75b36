"""The routes of a stage are decided once per forward (include/rvt_hip.h: rvt_stage_routes) and travel with the saved activations
(StageSaved.routes): a backward that runs under ANOTHER tuning record than its forward must still run what the forward prepared
for.  Checked by scoping `tuning.override(X)` around the forward only and comparing with the run that has X around both passes."""
import ctypes
import inspect

import pytest
import torch

from rvt_amd import _lib, backbone, stage, stage_driver, tuning
from tests import casegen
from tests import make_golden_launch_trace as LT
from tests.backends import backend, emu_library  # noqa: F401
from tests.test_backbone import build_model

OVERRIDES = {'attn_preln': dict(route_attn_preln=0), 'lstm_scan_wgrad': dict(route_lstm_scan_wgrad=0),
             'conv_dgrad4': dict(route_conv_dgrad4=0), 'fused_mlp': dict(route_fused_mlp=0), 'lstm_scan': dict(route_lstm_scan=0)}
# parameter gradients that fold through fp32 atomics on the GPU (LayerNorm weights / biases, every bias): their summation order differs
# from run to run, so two runs of the SAME launches agree to 2e-5 there (the rule of tests/test_stage_driver.py), bit for bit elsewhere
_ATOMIC = ('bias', 'norm.weight', 'norm1.weight', 'norm2.weight', 'mask_token')


def _step(name, dev, dtype, fwd_override, split):
    """One training step; `fwd_override` is in force during the forward, and during the backward too unless `split`."""
    m = build_model(name, dev, dtype)
    xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
    cots = [torch.from_numpy(a).to(dev) for a in casegen.make_cotangents(name)]
    with tuning.override(**fwd_override):
        feats, st_out = m.forward_sequence(xs, None)
        loss = sum((feats[s + 1].float() * cots[s]).sum() for s in range(4)) + sum(c.float().sum() * 0.5 for _, c in st_out)
        if not split:
            loss.backward()
    if split:
        loss.backward()
    out = {'feat%d' % s: feats[s].detach() for s in (1, 2, 3, 4)}
    out.update({k: p.grad for k, p in m.named_parameters()})
    return out


def _same(a, b, dev, what):
    worst = 0.0
    for k in a:
        if dev.type == 'cpu' or not k.endswith(_ATOMIC):
            assert torch.equal(a[k], b[k]), f'{what}: {k} differs, max {float((a[k].float() - b[k].float()).abs().max()):.3e}'
        else:
            err = float((a[k] - b[k]).abs().max()) / max(float(a[k].abs().max()), 1e-30)
            worst = max(worst, err)
            assert err <= 2e-5, f'{what}: {k} rel diff {err:.3e}'
    print(f'{what}: worst atomically folded gradient {worst:.3e}')


CASES = [pytest.param('micro', torch.bfloat16, id='micro-bf16'), pytest.param('micro', torch.float32, id='micro-f32'),
         pytest.param('base_qvga', torch.bfloat16, id='base_qvga-bf16')]


@pytest.mark.parametrize('drv', [0, 1], ids=['host_loop', 'c_driver'])
@pytest.mark.parametrize('x', list(OVERRIDES))
@pytest.mark.parametrize('name,dtype', CASES)
def test_backward_runs_the_forwards_routes(backend, name, dtype, x, drv):
    dev = backend
    if dev.type == 'cpu' and name == 'base_qvga':
        pytest.skip('minutes on the CPU emulator; runs on the GPU backend')
    with tuning.override(route_stage_driver_train=drv):
        inside = _step(name, dev, dtype, OVERRIDES[x], split=False)
        split = _step(name, dev, dtype, OVERRIDES[x], split=True)
    _same(inside, split, dev, f'{name} {x} drv={drv}')


def _train_trace(name, dev, dtype, **tun):
    with tuning.override(**LT.HOST_LOOP, **tun):
        m = build_model(name, dev, dtype)
        xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
        return LT.record(lambda: LT.run_mode(m, xs, None, 'train'))[0]


@pytest.mark.parametrize('x', list(OVERRIDES))
def test_every_override_moves_a_launch(backend, x):
    """A row of the test above proves something only if X changes the step's launches in one of its cases.  `micro` shows four of the
    five; route_conv_dgrad4 needs the widths of `base_qvga` (bf16, C = 64 -> 128 down-sampling), which only the GPU backend runs."""
    dev = backend
    name, dtype = ('base_qvga', torch.bfloat16) if x == 'conv_dgrad4' else ('micro', torch.bfloat16)
    if dev.type == 'cpu' and name == 'base_qvga':
        pytest.skip('minutes on the CPU emulator; runs on the GPU backend')
    assert _train_trace(name, dev, dtype) != _train_trace(name, dev, dtype, **OVERRIDES[x])


@pytest.mark.parametrize('drv', [0, 1], ids=['host_loop', 'c_driver'])
@pytest.mark.parametrize('name', ['micro', 'base_qvga'])
def test_lstm_scan3_backward_uses_the_forwards_tile_factor(backend, name, drv):
    """The dump layout of rvt_lstm_scan3_fwd (gsave / Csave) depends on the tile factor rb.  Forward under rb = 2, backward under the
    default 1 (this direction only: the dumps are then sized for the larger tile, so no code can read past them): the reverse scan
    must address the dumps with the forward's rb.  Before the route record the worst parameter gradient of this case was off by 56 %."""
    dev, dtype = backend, torch.bfloat16
    if dev.type == 'cpu' and name == 'base_qvga':
        pytest.skip('minutes on the CPU emulator; runs on the GPU backend')
    rb2 = dict(lstm_scan3_rb128=2, lstm_scan3_rb256=2)
    with tuning.override(route_lstm_scan=0, route_stage_driver_train=drv):
        assert tuning.get('lstm_scan3_rb128') == 1 and tuning.get('lstm_scan3_rb256') == 1
        if drv == 0:                     # the stage path really is on lstm_scan3, with the forward's rb in both directions
            with tuning.override(**rb2):
                m = build_model(name, dev, dtype)
                xs = torch.from_numpy(casegen.make_inputs(name)).to(dev)
                feats, _ = m.forward_sequence(xs, None)
            _, rbs = LT.record(lambda: sum(f.float().sum() for f in feats.values()).backward())
            assert rbs and all(n == 'rvt_lstm_scan3_bwd' and rb == 2 for n, _, rb in rbs), rbs
        inside = _step(name, dev, dtype, rb2, split=False)
        split = _step(name, dev, dtype, rb2, split=True)
    _same(inside, split, dev, f'{name} lstm_scan3 rb drv={drv}')


# ---- the planner alone (no kernel runs) ----
def _desc(dtype, C, T, tokens):
    B = tokens // 2560
    blocks = (stage_driver.RvtBlockWeights * 2)()             # n1_w NULL: the first block of a stage has no norm1
    d = stage_driver.RvtStageDesc()
    d.struct_bytes, d.dtype, d.C, d.Cin, d.cin_pad = ctypes.sizeof(d), _lib.dtype_code(dtype), C, max(C // 2, 8), max(C // 2, 8)
    d.H_in, d.W_in, d.k, d.stride, d.pad = 64, 160, 3, 2, 1     # -> 32 x 80 = 2560 tokens per frame
    d.ph, d.pw, d.dim_head, d.num_blocks, d.eps = 8, 10, 32, 1, 1e-5
    d.blocks = ctypes.cast(blocks, ctypes.POINTER(stage_driver.RvtBlockWeights))
    return d, blocks, B


@pytest.mark.parametrize('tun', ['test_geometry', 'production'])
def test_planner_invariants(tun):
    lib = emu_library()
    _lib._install_test_library(lib)
    saved = tuning.overrides()
    try:
        if tun == 'production':
            tuning.production()
        seen = set()
        for dtype in (torch.bfloat16, torch.float32):
            for C in (32, 64, 128, 256, 512):
                for T, tokens in ((1, 2560), (21, 2560), (21, 92160)):
                    for save in (0, 1):
                        for dws, mask in ((0, 0), (1, 0), (0, 1)):
                            d, keep, B = _desc(dtype, C, T, tokens)
                            r = stage_driver.RvtStageRoutes()
                            assert lib.rvt_stage_routes(ctypes.byref(d), T, B, save, dws, mask, ctypes.byref(r)) == 0
                            what = (dtype, C, T, tokens, save, dws, mask)
                            assert all(getattr(r, f) in (0, 1) for f, _ in r._fields_ if f not in ('mlp_route', 'lstm_route', 'lstm_scan3_rb')), what
                            assert r.mlp_route in (0, 1, 2) and r.lstm_route in (0, 1, 2, 3), what
                            assert not (r.ln_linear and r.attn_block), what
                            assert not r.mlp_bwd_both or r.mlp_route == 1, what
                            assert not r.lstm_scan_wgrad or r.lstm_route == 1, what
                            assert (r.lstm_scan3_rb in (1, 2)) == (r.lstm_route == 3) and (r.lstm_route == 3 or r.lstm_scan3_rb == 0), what
                            assert r.mlp_route != 2 or save, what
                            assert not (r.mlp_store_pre or r.mlp_bwd_dgrad) or r.mlp_route == 2, what
                            assert not (r.mlp_store_pre and r.mlp_bwd_dgrad), what
                            assert not r.attn_preln or ((r.attn_block or r.dgrad_ln_qkv) and not mask), what
                            if dws or mask:
                                assert r.driver_covers == 0, what
                            if dws:
                                assert r.lstm_route == 0, what
                            if save and not dws and not mask:   # the training driver leaves only the saving fused-MLP flavour to the host loop
                                assert r.driver_covers == (r.mlp_route != 2), what
                            seen.add((r.lstm_route, r.mlp_route, r.attn_block))
        assert len(seen) > 4, seen          # (the grid reaches several routes: the invariants are not checked on one record 180 times)
    finally:
        tuning.use(**saved)
        _lib._install_test_library(None)


def test_backward_reads_nothing_but_the_record():
    """Crude, but it is the property: the host-loop backward chooses its kernels by sv.routes alone."""
    src = inspect.getsource(stage.stage_seq_backward)
    assert 'tuning.get(' not in src and '_supported(' not in src and 'sv.routes' in src
    assert not any(hasattr(stage, n) for n in ('use_fused_mlp', 'use_attn_block', 'use_lstm_scan', 'use_lstm_scan3'))
    assert not hasattr(stage_driver, 'train_routes')
    bsrc = inspect.getsource(backbone._BackboneSeqFn.backward)
    assert 'tuning' not in bsrc and 'SideStream' not in bsrc and not hasattr(stage, 'SideStream')
