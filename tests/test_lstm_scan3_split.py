"""lstm_scan3 after the re-split to one 32-channel block per wave (rvt_amd/csrc/lstm_scan3.hpp): tails of both tile heights, the
forward's tile factor against the reverse scan's own tile, the weight ring across tile boundaries, and the two packed weight orders.
References and bounds are the ones of tests/test_lstm_scan.py: the fp64 cell, the rounding model of tests/bf16_model.py, tests/bounds.py."""
import pytest
import torch

from rvt_amd import ops, tuning, weights
from tests import bounds
from tests.backends import backend  # noqa: F401
from tests.test_lstm_scan import _scan3_run, modelled, near, ref_lstm, rnd

OUTS = ('Hall', 'c_last', 'dx', 'dz', 'dh0', 'dc0')
TAILS = [31, 33, 63, 65, 97, 129]     # 63 / 65 / 129: partial second row block of a 64-token tile; 31 / 33: partial first
_runs = {}


def run(dev, C, M, T, zero_state, rb):
    """One forward + reverse scan per (backend, shape, rb), shared by the tests below and never modified."""
    key = (dev.type, C, M, T, zero_state, rb)
    if key not in _runs:
        _runs[key] = _scan3_run(dev, C, M, T, zero_state, rb)
    return _runs[key]


@pytest.mark.parametrize('C', [128, 256])
@pytest.mark.parametrize('M', TAILS)
@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('rb', [1, 2])
@pytest.mark.parametrize('zero_state', [False, True])
def test_tails_against_fp64(backend, C, M, T, rb, zero_state):
    against_fp64(run(backend, C, M, T, zero_state, rb), C, M, zero_state)


def against_fp64(r, C, M, zero_state, grads=('dx', 'dz', 'dh0', 'dc0')):
    """All six outputs against the fp64 cell and its autograd, each under the ceiling of the rounding model (tests/bounds.py).
    Returns the fp64 h and c_last and the model's outputs."""
    dt = torch.bfloat16
    f64 = lambda t: t.double().cpu()
    xr, wr, br, h0r = (f64(r[k]).requires_grad_(True) for k in ('x', 'w', 'b', 'h0'))
    c0r = (torch.zeros(M, C, dtype=torch.float64) if r['c0'] is None else f64(r['c0'])).requires_grad_(True)
    hs, cs, zs = ref_lstm(xr, h0r, c0r, wr, br)
    truth = dict(h=hs, c_last=cs[-1])
    if not zero_state:
        (hs * f64(r['dH'])).sum().backward(retain_graph=True)
        torch.autograd.backward([cs[-1]], [f64(r['dc_last'])])
        truth.update(dz=torch.stack([z.grad for z in zs]), dx=xr.grad, dh0=h0r.grad, dc0=c0r.grad)
    m = modelled(dt, truth, r['x'], r['h0'], r['c0'], r['w'], r['b'], r['dH'], r['dc_last'], saved_gates=True)
    near(r['Hall'][1:], hs, dt, 'h', model=m['h'])
    near(r['c_last'], cs[-1], dt, 'c_last', model=m['c_last'])
    if zero_state:         # no upstream cotangents at all -> every gradient is exactly zero
        for k in ('dx', 'dz', 'dh0', 'dc0'):
            assert float(r[k].float().abs().max()) == 0.0, k
        return hs.detach(), cs[-1].detach(), m
    for k in grads:
        near(r[k], truth[k], dt, k, model=m[k])
    return hs.detach(), cs[-1].detach(), m


@pytest.mark.parametrize('C', [128, 256])
@pytest.mark.parametrize('M', TAILS)
def test_rb1_and_rb2_give_the_same_bits(backend, C, M):
    """The accumulation order per element does not depend on the tile height: a difference is a bug in the dump addressing or the row
    masks, not rounding.  Each reverse scan reads its own forward's dumps."""
    a, b = run(backend, C, M, 2, False, 1), run(backend, C, M, 2, False, 2)
    for k in OUTS:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


@pytest.mark.parametrize('C', [128, 256])
def test_forward_rb_is_independent_of_the_backward_tile(backend, C):
    """Several tiles of both heights, ragged end: the reverse scan walks its own tiles over dumps written by 32- and by 64-token
    forward tiles and must produce the same dx / dz bits."""
    a, b = run(backend, C, 200, 3, False, 1), run(backend, C, 200, 3, False, 2)
    for k in ('dx', 'dz'):
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


@pytest.mark.parametrize('C', [128, 256])
def test_more_tiles_than_workgroups_ragged_last_tile(backend, C):
    """M = (workgroups the launcher starts) x 64 + 33: every workgroup keeps its weight ring running into a second tile, the last one
    ragged.  On the GPU that is the production grid - the 64-token forward is bound by LDS to 2 (C = 128) / 1 (C = 256) workgroups per
    CU; the emulator has no occupancy to ask for, there the grid is set to 2.  Against the per-step kernels, as
    test_lstm_scan3_matches_per_step_kernels does."""
    dev, dt, T = backend, torch.bfloat16, 2
    if dev.type == 'cuda':
        wgs = torch.cuda.get_device_properties(dev).multi_processor_count * (2 if C == 128 else 1)
        grid = dict(gemm_resident=0)
    else:
        wgs = 2
        grid = dict(gemm_resident=wgs)
    M = wgs * 64 + 33
    with tuning.override(**grid):
        r = _scan3_run(dev, C, M, T, False, 2)
    perm = weights.lstm_gate_perm(C, dev)
    Hs = torch.empty_like(r['Hall'])
    Hs[0].copy_(r['h0'])
    Cs = torch.zeros(T + 1, M, C, dtype=torch.float32, device=dev)
    Cs[0].copy_(r['c0'])
    for t in range(T):
        ops.lstm_fwd(r['x'][t], Hs[t], Cs[t], r['w'][perm].contiguous(), r['b'][perm].contiguous(), Hs[t + 1], Cs[t + 1], None)
    # the reverse scan crossed tile boundaries too (dz, four times the size, is what dx and dh0 are products of: checked through them)
    hs, c_last, m = against_fp64(r, C, M, False, grads=('dx', 'dh0', 'dc0'))
    c_h, c_c = bounds.ceiling(hs, m['h'], True, 4), bounds.ceiling(c_last, m['c_last'], False, 4)
    near(r['Hall'][1:], Hs[1:], dt, 'h vs per-step kernels', ceiling=c_h + c_h)
    near(r['c_last'], Cs[T], dt, 'c_last vs per-step kernels', ceiling=c_c + c_c)


@pytest.mark.parametrize('C', [128, 256])
def test_pack_orders(backend, C):
    """Unpacking the two packed buffers on the host gives back W and W^T exactly.  Forward: [wave][k-step][gate][lane][8] =
    W[gate C + 32 wave + (lane & 31)][16 ks + 8 (lane >> 5) ..]; backward: [wave][k-step][x | h part][lane][8] = eight ROWS
    16 ks + 8 (lane >> 5) .. of column part C + 32 wave + (lane & 31)."""
    w = rnd((4 * C, 2 * C), backend, torch.bfloat16, 11)
    wp, wtp = ops.lstm_scan3_pack(w)
    w = w.cpu()
    fwd = wp.cpu().view(C // 32, 2 * C // 16, 4, 2, 32, 8)          # wave, ks, gate, half, li, e
    assert torch.equal(fwd.permute(2, 0, 4, 1, 3, 5).reshape(4 * C, 2 * C), w)
    bwd = wtp.cpu().view(C // 32, 4 * C // 16, 2, 2, 32, 8)         # wave, ks, part, half, li, e
    wt = bwd.permute(2, 0, 4, 1, 3, 5).reshape(2 * C, 4 * C)        # (part, wave, li) = column of W, (ks, half, e) = row of W
    assert torch.equal(wt, w.t())
    assert torch.equal(wt.t().contiguous(), w)
