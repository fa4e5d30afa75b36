"""The host tables of a stage are built once per weight set (rvt_amd/weights.py: ModelWeights.stage_call, StageGrads.blocks / .stage /
.train): descriptors, the backward's block table and RvtStageTrain template, and the gradient records named by the header.  They must
be built once, follow the weight set when it is rebuilt, keep the input flavours apart, and leave two live forwards their own records.
"Equal" is the rule of tests/test_route_record._same: bit for bit, except the atomically folded gradients on the GPU."""
import collections
import ctypes

import pytest
import torch

from rvt_amd import RNNDetector, stage_driver, tuning, weights
from rvt_amd._header import STRUCTS, fields
from tests import casegen
from tests.backends import backend  # noqa: F401
from tests.test_backbone import build_model, make_cfg
from tests.test_route_record import _same
from tests.test_stage_driver import _flat


def _data(name, dev, seed=1):
    xs = torch.from_numpy(casegen.make_inputs(name, seed=seed)).to(dev)
    return xs, [torch.from_numpy(a).to(dev) for a in casegen.make_cotangents(name)]


def _train_step(m, xs, cots, states=None):
    m.zero_grad(set_to_none=True)
    feats, st = m.forward_sequence(xs, states)
    (sum((feats[s + 1].float() * cots[s]).sum() for s in range(4)) + sum(c.float().sum() * 0.5 for _, c in st)).backward()
    return _flat(feats, st, {k: p.grad.clone() for k, p in m.named_parameters()})


def _nograd(m, xs):
    with torch.no_grad():
        return _flat(*m.forward_sequence(xs, None))


def _twin(m, name, dev, dtype):
    """A freshly built model holding m's current parameter values."""
    f = build_model(name, dev, dtype)
    f.load_state_dict(m.state_dict())
    return f


def _tables(mw):
    return list(mw._calls.values()) + [sg.train for sg in mw.grads]


# ---- 1. built once ------------------------------------------------------------------------------------------------------------------
def test_tables_are_built_once_and_see_repacked_weights(backend, monkeypatch):
    dev, dtype = backend, torch.bfloat16
    built = collections.Counter()
    for cls in (stage_driver.StageCall, stage_driver.TrainTables):
        def counted(self, *a, _init=cls.__init__, _name=cls.__name__, **k):
            built[_name] += 1
            _init(self, *a, **k)
        monkeypatch.setattr(cls, '__init__', counted)
    m = build_model('micro', dev, dtype)
    xs, cots = _data('micro', dev)
    for step in range(3):
        if step == 2:
            twin = _twin(m, 'micro', dev, dtype)
        got = _train_step(m, xs, cots)
        if step == 0:
            mw, first, n_built = m._mw_cache, _tables(m._mw_cache), dict(built)
            assert n_built == dict(StageCall=4, TrainTables=4), n_built
        if step < 2:
            with torch.no_grad():
                for p in m.parameters():                   # the way an optimizer writes: no version bump, no new storage
                    p.data.add_(p.grad, alpha=-1e-3)
    assert dict(built) == n_built, f'tables were built again after step 1: {dict(built)}'
    now = _tables(m._mw_cache)
    assert m._mw_cache is mw and len(now) == len(first) and all(a is b for a, b in zip(now, first))
    built.clear()
    _same(_train_step(twin, xs, cots), got, dev, 'step 3 on cached tables against a fresh model')


# ---- 2. the tables follow the weight set ----------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def _check_pointers(m, dropped):
    """Every pointer of every table of the current weight set, walked by header field name, is the data_ptr() of the current view of
    that name, and lies in none of the `dropped` (base, bytes) regions."""
    mw = m._mw_cache
    seen = []

    def expect(struct, rec, field, want):
        got = getattr(rec, field)
        assert got == want, f'{struct}.{field}: {got} is not the current view ({want})'
        if got is not None:
            seen.append((f'{struct}.{field}', got))
    assert mw._calls and mw.grads
    for call in mw._calls.values():
        sw = call.sw
        assert any(sw is s for s in mw.stages)
        for f in ('conv_w', 'ln_w', 'ln_b', 'lstm_w', 'lstm_b', 'lstm_wn', 'lstm_bn'):
            expect('RvtStageDesc', call.desc, f, _p(getattr(sw, f)))
        assert ctypes.cast(call.desc.blocks, ctypes.c_void_p).value == ctypes.addressof(call.blocks)
        for i, bw in enumerate(b for pair in sw.blocks for b in pair):
            for f in fields(STRUCTS['RvtBlockWeights']):
                expect('RvtBlockWeights', call.blocks[i], f, _p(bw[f]))
    for si, (sw, sg) in enumerate(zip(mw.stages, mw.grads)):
        pre, tt = f'stages.{si}.', sg.train
        names = [f'{pre}att_blocks.{bi}.{blk}.' for bi in range(len(sw.blocks)) for blk in ('att_window', 'att_grid')]
        for i, (bp, bw) in enumerate(zip(names, (b for pair in sw.blocks for b in pair))):
            for f in fields(STRUCTS['RvtBlockTrain']):
                want = _p(sg.view.get(bp + weights.BLOCK_GRADS[f])) if f.startswith('d_') else _p(bw[f])
                expect('RvtBlockTrain', tt.tb[i], f, want)
        t = tt.template
        assert t.struct_bytes == ctypes.sizeof(t) and ctypes.cast(t.tb, ctypes.c_void_p).value == ctypes.addressof(tt.tb)
        for f in ('lstm_wt', 'conv_wd4', 'conv_wd'):
            expect('RvtStageTrain', t, f, _p(getattr(sw, f)))
        for f in fields(STRUCTS['RvtStageTrain']):
            if f.startswith('d_'):
                expect('RvtStageTrain', t, f, _p(sg.view[pre + weights.STAGE_GRADS[f]]))
        assert all(c.train is mw.grads[k[0]].train for k, c in mw._calls.items())
    for what, ptr in seen:
        for base, n in dropped:
            assert not base <= ptr < base + n, f'{what} still points into a dropped buffer'
    return len(seen)


def _regions(mw):
    return [(t.data_ptr(), t.numel() * t.element_size()) for t in [mw.bufT, mw.buf32] + [sg.flat for sg in mw.grads]]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_tables_follow_the_weight_set(backend, dtype):
    dev = backend
    m = build_model('micro', dev, dtype)
    xs, cots = _data('micro', dev)
    twin = _twin(m, 'micro', dev, dtype)
    want_nograd, want_train = _nograd(twin, xs), _train_step(twin, xs, cots)
    held, dropped = [], []                         # the dropped weight sets stay alive here: their addresses cannot be recycled

    def drop():
        held.append(m._mw_cache)
        dropped.extend(_regions(m._mw_cache))
    _same(want_nograd, _nograd(m, xs), dev, 'no-grad forward')
    assert not m._mw_cache.need_grad and len(m._mw_cache._calls) == 4
    drop()
    _same(want_train, _train_step(m, xs, cots), dev, 'training step on the rebuilt (gradient) weight set')
    assert m._mw_cache is not held[-1] and m._mw_cache.need_grad
    assert _check_pointers(m, dropped) > 100
    drop()
    m.invalidate_weight_cache()
    _same(want_train, _train_step(m, xs, cots), dev, 'training step after invalidate_weight_cache()')
    assert m._mw_cache is not held[-1]
    _check_pointers(m, dropped)
    drop()
    name = 'stages.1.att_blocks.0.att_grid.norm1.weight'        # read by the kernels where it is: RvtBlockWeights.n1_w of stage 2, block 1
    p = m.get_parameter(name)
    held.append(p.data)
    dropped.append((p.data_ptr(), p.numel() * p.element_size()))
    p.data = p.data.clone()
    _same(want_train, _train_step(m, xs, cots), dev, 'training step after one parameter moved to a new storage')
    assert m._mw_cache is not held[-2]
    _check_pointers(m, dropped)
    assert [c.blocks[1].n1_w for k, c in m._mw_cache._calls.items() if k[0] == 1] == [p.data_ptr()]


# ---- 3. input flavours ------------------------------------------------------------------------------------------------------------------
def test_input_flavours_keep_their_descriptors(backend):
    dev, dtype = backend, torch.bfloat16
    m = build_model('micro', dev, dtype)
    xs, cots = _data('micro', dev)
    xf = xs.float()
    twin = _twin(m, 'micro', dev, dtype)
    t1, tf, t3 = _train_step(m, xs, cots), _train_step(m, xf, cots), _train_step(m, xs, cots)
    mw = m._mw_cache
    n1, nf, n3 = _nograd(m, xs), _nograd(m, xf), _nograd(m, xs)
    assert m._mw_cache is mw
    _same(t1, t3, dev, 'training step on uint8 planes, before and after a float32 run')
    _same(n1, n3, dev, 'no-grad forward on uint8 planes, before and after a float32 run')
    _same(_train_step(twin, xf, cots), tf, dev, 'float32 training step against a fresh model')
    _same(_nograd(twin, xf), nf, dev, 'float32 no-grad forward against a fresh model')
    per_stage = collections.Counter(k[0] for k in mw._calls)
    assert per_stage == {0: 2, 1: 1, 2: 1, 3: 1}, sorted(mw._calls)
    flavours = sorted(k[3:] for k in mw._calls if k[0] == 0)
    assert flavours == [(False, 0, 0), (True, *xs.shape[-2:])], flavours


# ---- 4. two forwards alive ------------------------------------------------------------------------------------------------------------
def _two_forwards(dev, dtype, drv):
    with tuning.override(route_stage_driver_train=drv):
        m = build_model('micro', dev, dtype)
        (xa, cots), (xb, _) = _data('micro', dev, seed=1), _data('micro', dev, seed=2)
        assert not torch.equal(xa, xb)
        with torch.no_grad():
            _, st = m.forward_sequence(xb, None)
        states = [(h.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)) for h, c in st]
        fa, sa = m.forward_sequence(xa, states)
        fb, sb = m.forward_sequence(xb, sa)                # both forwards are alive; the second continues the first's states
        if drv:
            mw = m._mw_cache
            assert len(mw._calls) == 4 and all(sg.train is not None for sg in mw.grads)
        loss = sum((f[s + 1].float() * cots[s]).sum() for f in (fa, fb) for s in range(4)) + sum(c.float().sum() * 0.5 for _, c in sa + sb)
        loss.backward()
        out = {f'a.{k}': v for k, v in _flat(fa, sa).items()}
        out.update({f'b.{k}': v for k, v in _flat(fb, sb).items()})
        out.update({k: p.grad for k, p in m.named_parameters()})
        out.update({f'state_grad{i}': t.grad for i, hc in enumerate(states) for t in hc})
        return out


def test_two_live_forwards_keep_their_own_records(backend):
    dev, dtype = backend, torch.bfloat16
    want, got = _two_forwards(dev, dtype, 0), _two_forwards(dev, dtype, 1)
    assert got.keys() == want.keys() and all(v is not None for v in got.values())
    _same(want, got, dev, 'two forwards, one backward: C-side driver against the host loop')


# ---- 5. the name table covers the header (no library call) ------------------------------------------------------------------------------
def _name_table_problems(block, stage, host, folds, unpack):
    """What is wrong with a set of name tables: against the d_* fields of the header's two records, and against the parameter names of
    three models (plain, token mask, DWS-ConvLSTM on x and h), each of which must be reached exactly once."""
    out = []
    for struct, table in (('RvtBlockTrain', block), ('RvtStageTrain', stage)):
        slots = [f for f in fields(STRUCTS[struct]) if f.startswith('d_')]
        if sorted(slots) != sorted(table):
            out.append(f'{struct}: header slots {sorted(set(slots) ^ set(table))} without exactly one entry')
    if set(host) & (set(fields(STRUCTS['RvtStageTrain'])) | set(stage)):
        out.append('a host-loop-only slot carries a header name')
    for case in ('micro', 'micro_mask', 'micro_dws_xh'):
        m = RNNDetector(make_cfg(case))
        for si in range(m.num_stages):
            pre = f'stages.{si}.'
            params = {n for n in m._param_names if n.startswith(pre)}
            reached = collections.Counter()
            for bi in range(m.num_blocks[si]):
                for blk in ('att_window', 'att_grid'):
                    bp = f'{pre}att_blocks.{bi}.{blk}.'
                    reached.update(bp + n for n in block.values())
                    for S, cs, W, b, gamma, _ in folds:
                        reached.update(bp + n for n in (W, b, gamma))
                        reached.subtract(bp + block[s] for s in (S, cs) if s in block)       # a raw product is consumed by its fold
            reached.update(pre + n for n in list(stage.values()) + list(host.values()))
            if unpack is not None:
                reached[pre + unpack[1]] += 1
                reached[pre + stage.get(unpack[0], '?')] -= 1
            out += [f'{case}: {n} is reached {reached[n]} times' for n in sorted(params) if reached[n] != 1]
            out += [f'{case}: {n} is no parameter and nothing consumes it' for n, c in sorted(reached.items())
                    if c > 0 and n not in params and not n.endswith(('norm1.weight', 'norm1.bias', 'mask_token')) and 'conv3x3_dws' not in n]
    return out


def test_gradient_name_table_covers_the_header_and_the_parameters():
    W = weights
    tables = dict(block=W.BLOCK_GRADS, stage=W.STAGE_GRADS, host=W.HOST_LOOP_GRADS, folds=W.LAYERSCALE_FOLDS, unpack=W.CONV_UNPACK)
    assert _name_table_problems(**tables) == []
    # the check bites: any one entry taken out of a copy of the tables
    for which in ('block', 'stage', 'host'):
        for slot in tables[which]:
            cut = dict(tables, **{which: {k: v for k, v in tables[which].items() if k != slot}})
            assert _name_table_problems(**cut), f'removing {slot} from the {which} table went unnoticed'
    for i in range(len(W.LAYERSCALE_FOLDS)):
        assert _name_table_problems(**dict(tables, folds=W.LAYERSCALE_FOLDS[:i] + W.LAYERSCALE_FOLDS[i + 1:]))
    assert _name_table_problems(**dict(tables, unpack=None))
