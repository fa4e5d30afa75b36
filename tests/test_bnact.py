"""The BatchNorm2d + SiLU row kernels of the PAFPN / head BaseConv units (csrc/bnact.hpp: rvt_bn_stats, rvt_bn_finalize,
rvt_bn_act_fwd, rvt_bn_train_act_fwd, rvt_bn_act_bwd_stats, rvt_bn_act_bwd_apply), each called directly through rvt_amd._lib the
way rvt_amd/fpn.py calls it, against the same operation in fp64 torch.

REFERENCE.  F.batch_norm(training=True, momentum=0.1, eps=1e-5) followed by F.silu (or nothing, act = 0) and its autograd, in
fp64, on the inputs as the kernel sees them (bf16 inputs are rounded first, then widened).  ISOLATION: a kernel that takes
statistics gets them from the fp64 truth, rounded to fp32, and is compared with the fp64 restatement of ITS operation on exactly
those inputs (`_Case.finalize_from / y_from / dz_sums_from / dx_from`; the restatements are themselves pinned to F.batch_norm's autograd in
`_Case.__init__`), so an error of one kernel neither blurs nor excuses the next.  `_run_chain` runs stats -> train_act_fwd ->
bwd_stats -> bwd_apply on each other's outputs, as _BaseConvFn does, against F.batch_norm itself.

TOLERANCE (the idiom of tests/test_optim.py: fp64 truth, fp32 yardstick; nothing is measured against the code under test).  torch's
own fp32 batch_norm + silu + autograd runs on the same device on the same inputs.  For every fp32 output, including every fp32
statistic of the bf16 runs,
        max |ours - fp64|  <=  4 * max |torch fp32 - fp64|  +  4 ulp(fp32) at the largest magnitude of that tensor.
The factor is 4 where the optimizer test has 2 because these kernels legally differ from torch in more than operation order: a
hardware exp2 and a hardware reciprocal of about one ulp each, a fused multiply-add in z = x * scale + shift, a column reduction
over atomics.  The ulp term: at 2 or 3 rows the yardstick is a maximum over a few dozen numbers and can happen to be nearly exact.
bf16 tensors (y, dx), element-wise:  |ours - fp64| <= 2^-8 |fp64| (one bf16 ulp: the right value or its neighbour) + the fp32 bound.
Every output must be finite.  Each check prints ours / yardstick / bound (`pytest -s`); NOTES.md holds the worst ratios seen.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rvt_amd import _lib as L
from tests.backends import backend  # noqa: F401

EPS, MOM = 1e-5, 0.1
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]

# (rows, C): the smallest shapes that reach each path of the thread layout Gp = pow2 >= C / 8 column groups x 256 / Gp row lanes
SHAPES = [
    (2, 8),          # Gp = 1, 254 of 256 row lanes idle; the fp64 problem itself is ill-conditioned at two rows
    (3, 24),         # Gp = 4 with one dead column group
    (31, 96),        # Gp = 16, 12 live groups, rows not a multiple of the 16 row lanes
    (257, 40),       # Gp = 8, 5 live groups, two workgroups with a tail
    (2049, 384),     # Gp = 64, 48 live groups, many workgroups, the last one nearly empty
    (1000, 1024),    # the widest the two reductions accept, two row lanes
]
WIDE = (19, 2040)    # Gp = 256, one row lane, not a power of two: the three row kernels only (their sums come from the host)
ACT0_SHAPES = [(3, 24), (257, 40), WIDE]                     # act = 0 (affine only); act = 1 runs at every shape
SHIFTED = [(2049, 384), (2000, 24)]
LARGE = (65553, 1024)                                        # past the grid caps: 16 384 rows (reductions), 65 536 (row kernels)


def _shape_act(shapes):
    return [pytest.param(s, a, id=f'{s[0]}x{s[1]}-act{a}') for s in shapes for a in (1, 0) if a == 1 or s in ACT0_SHAPES]


def _act(z, act):
    return F.silu(z) if act else z


def _dact(z, act):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s)) if act else torch.ones_like(z)


class _Case:
    """Inputs, the fp64 truth and the errors of torch's fp32 run (the yardstick), computed once per (device, shape, dtype, act,
    offset) and shared, unchanged, by every test that needs them."""

    def __init__(self, dev, rows, C, dt, act, offset=0.0):
        self.dev, self.rows, self.C, self.dt, self.act = dev, rows, C, dt, act
        g = torch.Generator().manual_seed(7919 * rows + C)
        gamma = 0.5 + torch.rand(C, generator=g)                                  # [0.5, 1.5], beta about 0.1 (tests/casegen_fpn.py)
        beta = 0.1 * torch.randn(C, generator=g)
        if rows * C <= 1 << 22:
            x, dy = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
        else:                                                                     # (the one large case: drawn on the device)
            gd = torch.Generator(device=dev).manual_seed(rows)
            x, dy = (torch.randn(rows, C, generator=gd, device=dev) for _ in range(2))
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        off = offset * sign                                                       # channel mean of +-offset standard deviations
        x += off.to(x.device)
        if rows >= 257:
            # one row (never the first) whose z lands near +30 / -30, alternating by channel: the saturated ends of silu / silu' on
            # the hardware exp2.  xhat of a lone value v among n unit-variance rows is v / sqrt(1 + v^2 / n) < sqrt(n): aim at
            # 30 / gamma where the row count allows it
            t = torch.minimum(30.0 / gamma, torch.tensor(0.7 * rows ** 0.5))
            v = t / torch.sqrt(1 - t * t / rows)
            alt = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
            x[rows // 2] = (off + alt * v).to(x.device)
        self.x, self.dy = x.to(dt).to(dev), dy.to(dt).to(dev)
        self.gamma, self.beta = gamma.to(dev), beta.to(dev)
        self.rm0 = (0.3 * torch.randn(C, generator=g)).to(dev)                    # non-trivial running statistics to start from
        self.rv0 = (0.5 + 1.5 * torch.rand(C, generator=g)).to(dev)
        self.x64, self.dy64 = self.x.double(), self.dy.double()
        self.truth, self.yard, self.big = {}, {}, {}

        def run(ft):
            xr = self.x.to(ft).requires_grad_(True)
            gm, bt = self.gamma.to(ft).requires_grad_(True), self.beta.to(ft).requires_grad_(True)
            rm, rv = self.rm0.to(ft).clone(), self.rv0.to(ft).clone()
            y = _act(F.batch_norm(xr, rm, rv, gm, bt, True, MOM, EPS), act)
            y.backward(self.dy.to(ft))
            out = dict(y=y.detach(), dx=xr.grad, dsum=bt.grad, dxsum=gm.grad, running_mean=rm, running_var=rv,
                       sum=xr.detach().sum(0), sumsq=(xr.detach() ** 2).sum(0))
            if ft == torch.float64:
                mean, var = xr.detach().mean(0), xr.detach().var(0, unbiased=False)
                rstd = 1.0 / torch.sqrt(var + EPS)
            else:                                       # torch's own fp32 statistics: the mean and invstd its kernel saves
                _, mean, rstd = torch.native_batch_norm(xr.detach(), gm.detach(), bt.detach(), rm.clone(), rv.clone(), True, MOM, EPS)
            sc = gm.detach() * rstd
            out.update(mean=mean, rstd=rstd, scale=sc, shift=bt.detach() - mean * sc)
            return out
        self.truth = run(torch.float64)
        y32 = run(torch.float32)
        for k, t in self.truth.items():
            self.yard[k] = float((y32[k].double() - t).abs().max())
            self.big[k] = float(t.abs().max())
        del y32
        # the fp64 restatements below ARE batch_norm + act and its backward: pin them to torch's autograd once
        tr = self.truth
        st = {k: tr[k] for k in ('mean', 'rstd', 'scale', 'shift')}
        for got, want in ((self.y_from(st), tr['y']), (self.dz_sums_from(st)[0], tr['dsum']), (self.dz_sums_from(st)[1], tr['dxsum']),
                          (self.dx_from(st, tr['dsum'], tr['dxsum']), tr['dx'])):
            assert float((got - want).abs().max()) <= 1e-9 * max(float(want.abs().max()), 1.0)

    # ---- fp64 restatements of what each kernel computes FROM ITS INPUTS (st: mean / rstd / scale / shift as the kernel gets them)
    def finalize_from(self, stats):
        n = float(self.rows)
        mean = stats[0] / n
        var = stats[1] / n - mean * mean
        rstd = 1.0 / torch.sqrt(var + EPS)
        sc = self.gamma.double() * rstd
        return dict(mean=mean, rstd=rstd, scale=sc, shift=self.beta.double() - mean * sc,
                    running_mean=(1 - MOM) * self.rm0.double() + MOM * mean,
                    running_var=(1 - MOM) * self.rv0.double() + MOM * var * (n / (n - 1.0)))

    def y_from(self, st):
        return _act(self.x64 * st['scale'].double() + st['shift'].double(), self.act)

    def _dz(self, st):
        return self.dy64 * _dact(self.x64 * st['scale'].double() + st['shift'].double(), self.act)

    def dz_sums_from(self, st):
        dz = self._dz(st)
        return dz.sum(0), (dz * (self.x64 - st['mean'].double()) * st['rstd'].double()).sum(0)

    def dx_from(self, st, dsum, dxsum):
        xh = (self.x64 - st['mean'].double()) * st['rstd'].double()
        return st['scale'].double() * (self._dz(st) - dsum.double() / self.rows - xh * dxsum.double() / self.rows)

    def f32(self, *names):
        """fp64 truth rounded to fp32: what an isolated kernel is fed."""
        return {k: self.truth[k].float().contiguous() for k in names}


@functools.lru_cache(maxsize=None)
def _cached_case(dev_type, rows, C, dt, act, offset):
    return _Case(torch.device('cuda', 0) if dev_type == 'cuda' else torch.device('cpu'), rows, C, dt, act, offset)


def _case(dev, shape, dt, act, offset=0.0):
    return _cached_case(dev.type, shape[0], shape[1], dt, act, offset)


def _check(c, kernel, name, ours, truth=None):
    """The module docstring's bound for output `name` of `kernel`; truth defaults to F.batch_norm's own."""
    truth = (c.truth[name] if truth is None else truth).detach()
    o64 = ours.detach().double()
    assert bool(torch.isfinite(o64).all()), (kernel, name)
    assert o64.shape == truth.shape
    bound = 4 * c.yard[name] + 4 * float(np.spacing(np.float32(max(c.big[name], float(truth.detach().abs().max())))))
    err = (o64 - truth).abs()
    e_ours = float(err.max())
    tag = f'bnact|{kernel}|{str(c.dt)[6:]}|{name}|{c.rows}x{c.C}|act{c.act}'
    if ours.dtype == BF16:
        excess = float((err - 2.0 ** -8 * truth.abs()).max())                     # what the bf16 rounding of the output does not explain
        print(f'{tag}: ours {e_ours:.3e} (beyond one bf16 ulp {max(excess, 0.0):.3e})  torch fp32 {c.yard[name]:.3e}  bound {bound:.3e}')
        assert excess <= bound, (kernel, name, e_ours, excess, c.yard[name], bound)
    else:
        ratio = e_ours / c.yard[name] if c.yard[name] > 0 else float('inf') if e_ours > 0 else 0.0
        print(f'{tag}: ours {e_ours:.3e}  torch fp32 {c.yard[name]:.3e}  bound {bound:.3e}  ours/torch {ratio:.2f}')
        assert e_ours <= bound, (kernel, name, e_ours, c.yard[name], bound)


CANARY = 256


def _guarded(c, shape, dt, fill=0.0):
    """An output tensor with 256 canary elements behind it (an idle column group or a row past the end that writes shows there)."""
    n = int(np.prod(shape))
    buf = torch.full((n + CANARY,), 12345.0, dtype=dt, device=c.dev)
    buf[:n] = fill
    return buf[:n].view(*shape), buf


def _intact(buf):
    assert bool((buf[-CANARY:] == 12345.0).all()), 'write past the end of an output'


def _code(c):
    return L.dtype_code(c.dt)


# ---- one runner per entry point ------------------------------------------------------------------------------------------
def _run_stats(c):
    st, buf = _guarded(c, (2, c.C), torch.float64)
    L.call('rvt_bn_stats', L.ptr(c.x), L.ptr(st), _code(c), c.rows, c.C, L.stream_of(c.x))
    _intact(buf)
    _check(c, 'bn_stats', 'sum', st[0])
    _check(c, 'bn_stats', 'sumsq', st[1])
    return st


def _sums_in(c):
    """rvt_bn_stats' two fp64 vectors from the truth."""
    return torch.stack([c.truth['sum'], c.truth['sumsq']]).contiguous()


def _run_finalize_training(c):
    s = _sums_in(c)
    want = c.finalize_from(s)
    fin, buf = _guarded(c, (4, c.C), F32)
    rm, rv = c.rm0.clone(), c.rv0.clone()
    L.call('rvt_bn_finalize', L.ptr(s), c.rows, L.ptr(c.gamma), L.ptr(c.beta), EPS, MOM, L.ptr(rm), L.ptr(rv),
           L.ptr(fin[0]), L.ptr(fin[1]), L.ptr(fin[2]), L.ptr(fin[3]), c.C, 1, L.stream_of(fin))
    _intact(buf)
    for i, k in enumerate(('mean', 'rstd', 'scale', 'shift')):
        _check(c, 'bn_finalize', k, fin[i], want[k])
    _check(c, 'bn_finalize', 'running_mean', rm, want['running_mean'])
    _check(c, 'bn_finalize', 'running_var', rv, want['running_var'])


def _run_act_fwd(c):
    st = c.f32('scale', 'shift')
    y, buf = _guarded(c, (c.rows, c.C), c.dt)
    L.call('rvt_bn_act_fwd', L.ptr(c.x), L.ptr(st['scale']), L.ptr(st['shift']), L.ptr(y), _code(c), c.rows, c.C, c.act, L.stream_of(y))
    _intact(buf)
    _check(c, 'bn_act_fwd', 'y', y, c.y_from(st))


def _train_act_fwd(c, s, kernel, want=None):
    fin, fbuf = _guarded(c, (4, c.C), F32)
    y, ybuf = _guarded(c, (c.rows, c.C), c.dt)
    rm, rv = c.rm0.clone(), c.rv0.clone()
    L.call('rvt_bn_train_act_fwd', L.ptr(c.x), L.ptr(s), c.rows, L.ptr(c.gamma), L.ptr(c.beta), EPS, MOM,
           L.ptr(rm), L.ptr(rv), L.ptr(fin[0]), L.ptr(fin[1]), L.ptr(fin[2]), L.ptr(fin[3]), L.ptr(y), _code(c), c.rows, c.C, c.act,
           L.stream_of(y))
    _intact(fbuf)
    _intact(ybuf)
    want = want or {}
    for i, k in enumerate(('mean', 'rstd', 'scale', 'shift')):
        _check(c, kernel, k, fin[i], want.get(k))
    _check(c, kernel, 'running_mean', rm, want.get('running_mean'))
    _check(c, kernel, 'running_var', rv, want.get('running_var'))
    _check(c, kernel, 'y', y, want.get('y'))
    return fin, y


def _run_train_act_fwd(c):
    s = _sums_in(c)
    want = c.finalize_from(s)
    want['y'] = c.y_from(want)
    _train_act_fwd(c, s, 'bn_train_act_fwd', want)


def _bwd_stats(c, st, kernel, want=None):
    ds, buf = _guarded(c, (2, c.C), torch.float64)
    L.call('rvt_bn_act_bwd_stats', L.ptr(c.dy), L.ptr(c.x), L.ptr(st['scale']), L.ptr(st['shift']), L.ptr(st['mean']), L.ptr(st['rstd']),
           L.ptr(ds[0]), L.ptr(ds[1]), _code(c), c.rows, c.C, c.act, L.stream_of(ds))
    _intact(buf)
    _check(c, kernel, 'dsum', ds[0], None if want is None else want[0])
    _check(c, kernel, 'dxsum', ds[1], None if want is None else want[1])
    return ds


def _run_bwd_stats(c):
    st = c.f32('mean', 'rstd', 'scale', 'shift')
    _bwd_stats(c, st, 'bn_act_bwd_stats', c.dz_sums_from(st))


def _bwd_apply(c, st, dsum, dxsum, kernel, want=None):
    dx, buf = _guarded(c, (c.rows, c.C), c.dt)
    L.call('rvt_bn_act_bwd_apply', L.ptr(c.dy), L.ptr(c.x), L.ptr(st['scale']), L.ptr(st['shift']), L.ptr(st['mean']), L.ptr(st['rstd']),
           L.ptr(dsum), L.ptr(dxsum), L.ptr(dx), _code(c), c.rows, c.C, c.act, L.stream_of(dx))
    _intact(buf)
    _check(c, kernel, 'dx', dx, want)


def _run_bwd_apply(c):
    st = c.f32('mean', 'rstd', 'scale', 'shift')
    dsum, dxsum = c.truth['dsum'].contiguous(), c.truth['dxsum'].contiguous()    # the fp64 sums, not bn_act_bwd_stats' own
    _bwd_apply(c, st, dsum, dxsum, 'bn_act_bwd_apply', c.dx_from(st, dsum, dxsum))


def _run_chain(c):
    """stats -> train_act_fwd -> bwd_stats -> bwd_apply on each other's outputs (what _BaseConvFn runs), against F.batch_norm."""
    s = _run_stats(c).contiguous()
    fin, _ = _train_act_fwd(c, s, 'chain')
    st = dict(mean=fin[0].contiguous(), rstd=fin[1].contiguous(), scale=fin[2].contiguous(), shift=fin[3].contiguous())
    ds = _bwd_stats(c, st, 'chain')
    _bwd_apply(c, st, ds[0].contiguous(), ds[1].contiguous(), 'chain')


ISOLATED = [_run_stats, _run_finalize_training, _run_act_fwd, _run_train_act_fwd, _run_bwd_stats, _run_bwd_apply]


# ---- the tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_bn_stats(backend, shape, dt):
    _run_stats(_case(backend, shape, dt, 1))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', SHAPES)
def test_bn_finalize_training(backend, shape, dt):
    """training = 1, the two-launch route: mean / rstd / scale / shift and the running-statistics update (unbiased variance)."""
    _run_finalize_training(_case(backend, shape, dt, 1))


@pytest.mark.parametrize('null_outs', [False, True])
@pytest.mark.parametrize('C', [8, 300, 2040])
def test_bn_finalize_eval(backend, C, null_outs):
    """training = 0: scale / shift from the running statistics, which stay untouched; mean_out / rstd_out may be null.  The
    yardstick is the same three lines in torch fp32."""
    dev = backend
    g = torch.Generator().manual_seed(C)
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    rm, rv = (3.0 * torch.randn(C, generator=g)).to(dev), (0.01 + 4.0 * torch.rand(C, generator=g)).to(dev)
    rm0, rv0 = rm.clone(), rv.clone()
    fin = torch.full((4, C), float('nan'), device=dev)
    outs = (None, None) if null_outs else (L.ptr(fin[0]), L.ptr(fin[1]))
    L.call('rvt_bn_finalize', None, 1, L.ptr(gamma), L.ptr(beta), EPS, MOM, L.ptr(rm), L.ptr(rv), *outs, L.ptr(fin[2]),
           L.ptr(fin[3]), C, 0, L.stream_of(fin))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    rstd64 = 1.0 / torch.sqrt(rv.double() + EPS)
    sc64 = gamma.double() * rstd64
    rstd32 = 1.0 / torch.sqrt(rv + EPS)
    sc32 = gamma * rstd32
    rows = [(2, 'scale', sc64, sc32), (3, 'shift', beta.double() - rm.double() * sc64, beta - rm * sc32)]
    if null_outs:
        assert bool(torch.isnan(fin[:2]).all())
    else:
        assert torch.equal(fin[0], rm)
        rows.append((1, 'rstd', rstd64, rstd32))
    for i, name, t64, t32 in rows:
        e_ours, e_yard = float((fin[i].double() - t64).abs().max()), float((t32.double() - t64).abs().max())
        bound = 4 * e_yard + 4 * float(np.spacing(np.float32(t64.abs().max().item())))
        print(f'bnact|bn_finalize_eval|float32|{name}|C{C}: ours {e_ours:.3e}  torch fp32 {e_yard:.3e}  bound {bound:.3e}')
        assert bool(torch.isfinite(fin[i]).all()) and e_ours <= bound, (name, e_ours, e_yard, bound)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape,act', _shape_act(SHAPES + [WIDE]))
def test_bn_act_fwd(backend, shape, act, dt):
    _run_act_fwd(_case(backend, shape, dt, act))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape,act', _shape_act(SHAPES + [WIDE]))
def test_bn_train_act_fwd(backend, shape, act, dt):
    _run_train_act_fwd(_case(backend, shape, dt, act))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape,act', _shape_act(SHAPES))
def test_bn_act_bwd_stats(backend, shape, act, dt):
    _run_bwd_stats(_case(backend, shape, dt, act))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape,act', _shape_act(SHAPES + [WIDE]))
def test_bn_act_bwd_apply(backend, shape, act, dt):
    _run_bwd_apply(_case(backend, shape, dt, act))


@pytest.mark.parametrize('dt', DTYPES)
def test_bn_chain(backend, dt):
    _run_chain(_case(backend, (2049, 384), dt, 1))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('offset', [4.0, 16.0])
@pytest.mark.parametrize('shape', SHIFTED)
def test_bn_shifted_means(backend, shape, offset, dt):
    """Channel means of +-4 and +-16 standard deviations (sign drawn per channel), at the bound of every other case.  Sums of x and
    x^2 around zero lose the variance to cancellation there (relative error ~ (mean / std)^2 * 2^-24: 30 to 100 times torch's at
    +-16, measured; NOTES.md); rvt_bn_stats sums in fp64 instead.  Every kernel alone, then the chain."""
    c = _case(backend, shape, dt, 1, offset)
    for run in ISOLATED:
        run(c)
    _run_chain(c)


@pytest.mark.gpu
def test_bn_all_kernels_past_the_grid_caps():
    """65 553 x 1024 in bf16 (134 MB a tensor): the two reductions cap their grid at 1024 workgroups (16 384 rows a pass at this
    width), the row kernels at 4096 (65 536 rows), so every kernel makes further grid-stride passes and the last one is partial.  The
    fp64 reference stays on the device."""
    L._install_test_library(None)
    c = _Case(torch.device('cuda', 0), *LARGE, BF16, 1)
    for run in ISOLATED:
        run(c)
    _run_chain(c)


def test_bn_argument_checks(backend):
    """Refused before any launch: a non-zero return and rvt_last_error naming the entry point."""
    dev = backend
    lib = L.get_lib()
    z = torch.zeros(4 * 2056, device=dev)
    p, st = L.ptr(z), L.stream_of(z)

    def calls(C, act):
        return {
            'bn_stats': ('rvt_bn_stats', p, p, 0, 1, C, st),
            'bn_act_bwd_stats': ('rvt_bn_act_bwd_stats', p, p, p, p, p, p, p, p, 0, 1, C, act, st),
            'bn_act_fwd': ('rvt_bn_act_fwd', p, p, p, p, 0, 1, C, act, st),
            'bn_train_act_fwd': ('rvt_bn_train_act_fwd', p, p, 1, p, p, EPS, MOM, p, p, p, p, p, p, p, 0, 1, C, act, st),
            'bn_act_bwd_apply': ('rvt_bn_act_bwd_apply', p, p, p, p, p, p, p, p, p, 0, 1, C, act, st),
        }

    def refused(who, args):
        rc = getattr(lib, args[0])(*args[1:])
        assert rc != 0, (who, args[-3:])
        assert who + ':' in lib.rvt_last_error().decode(), (who, lib.rvt_last_error())
    reductions, rowk = ('bn_stats', 'bn_act_bwd_stats'), ('bn_act_fwd', 'bn_train_act_fwd', 'bn_act_bwd_apply')
    for who, args in calls(20, 1).items():                                       # not a multiple of 8
        refused(who, args)
    for who in reductions:                                                       # wider than the reductions' shared-memory layout
        refused(who, calls(1032, 1)[who])
    for who in rowk:                                                             # wider than 256 column groups
        refused(who, calls(2056, 1)[who])
    for who in ('bn_act_fwd', 'bn_train_act_fwd', 'bn_act_bwd_stats', 'bn_act_bwd_apply'):
        refused(who, calls(16, 2)[who])
    assert bool((z == 0).all())
