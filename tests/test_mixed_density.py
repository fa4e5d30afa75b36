"""The mixed-density event stack on the device: rvt_amd.representations.MixedDensityEventStack (one window) and
EventSequenceBuilder(representation='mixed_density') (whole (T, B, bins, H', W') int8 sequences; csrc/evseq.hpp), against fixtures
recorded from the unmodified reference (tests/make_golden_mixed_density.py).  Integer output: every comparison is bit-exact.

The device takes the bin from the binary exponent of the fp32 normalised time instead of the reference's fp32 log quotient.  The two
agree for every window spanning at most 2^20 us, which every fixture window does (the recorder asserts it); beyond 2^22 us the
reference itself is off by one bin a few ulps below a power of two and the device returns the exact bin, so the large-span test
compares with a numpy restatement of the exponent rule, deliberately not with the reference."""
import os

import numpy as np
import pytest
import torch

from rvt_amd import RNNDetector, _lib
from rvt_amd._header import LaunchArgs
from rvt_amd.representations import EventSequenceBuilder, MixedDensityEventStack
from tests import casegen
from tests.backends import backend  # noqa: F401
from tests.casegen_mixed_density import SEQUENCE, SINGLE, sequence_kwargs, stack_kwargs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_COORD = (torch.int16, torch.int32, torch.int64)


def load_sequence(name, dev, coord=torch.int16):
    """Streams of the stacked-histogram fixture of the same case, expected planes / bounds of the mixed representation."""
    s = np.load(os.path.join(GOLD, f'evseq_{name}.npz'))
    g = np.load(os.path.join(GOLD, f'evseq_md_{name}.npz'))
    B = g['bounds'].shape[0]
    # clone: torch's own allocation, 64-byte aligned on either backend (the 16-byte load path)
    streams = [tuple(torch.from_numpy(s[f'{k}{b}']).to(coord).clone().to(dev) for k in 'xyp') + (torch.from_numpy(s[f't{b}']).clone().to(dev),)
               for b in range(B)]
    assert all(a.data_ptr() % 16 == 0 for st in streams for a in st)
    assert np.array_equal(s['ts_end'], g['ts_end'])
    return streams, torch.from_numpy(g['ts_end']).to(dev), g['bounds'], g['planes']


# ---- 1. one window ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SINGLE))
def test_construct_matches_reference_fixture(backend, name):
    dev = backend
    g = np.load(os.path.join(GOLD, f'mdstack_{name}.npz'))
    c = SINGLE[name]
    rep = MixedDensityEventStack(**stack_kwargs(c))
    assert rep.get_shape() == (c['bins'], c['H'], c['W']) == g['out'].shape
    assert rep.get_numpy_dtype() == np.dtype('int8') and rep.get_torch_dtype() == torch.int8 and rep.dtype == torch.int8
    ev = [torch.from_numpy(g[k].astype(np.int64)).to(dev) for k in 'xypt']
    out = rep.construct(*ev)
    assert out.dtype == torch.int8 and tuple(out.shape) == g['out'].shape
    assert np.array_equal(out.cpu().numpy(), g['out'])
    # the second call runs on the scratch image the first one left behind: it must have been left clean
    assert np.array_equal(rep.construct(*ev).cpu().numpy(), g['out'])
    # narrower integer inputs are widened by construct
    assert np.array_equal(rep.construct(*(a.to(torch.int32) for a in ev[:3]), ev[3]).cpu().numpy(), g['out'])
    want = {'hot_pos': (3, 44), 'hot_neg': (3, 56), 'cutoff0': None}.get(name, ())
    if want is None:
        assert not g['out'].any()
    elif want:
        assert int(out[want[0], 5, 3]) == want[1]                       # the wrapped hot cell in the last bin
    if name == 'prefix_wrap':
        assert [int(v) for v in out[7:, 5, 3]] == [0, 100, -56]
    if name == 'one_timestamp':
        assert not g['out'][:5].any() and g['out'][5].any() and np.array_equal(g['out'][5], g['out'][24])


# ---- 2. whole sequences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SEQUENCE))
def test_sequence_matches_reference_fixture(backend, name):
    dev = backend
    kw = sequence_kwargs(name)
    streams, ts_end, bounds, planes = load_sequence(name, dev)
    T, B = planes.shape[:2]
    eb = EventSequenceBuilder(**kw)
    assert eb.get_shape() == planes.shape[2:] and eb.get_shape()[0] == kw['bins']
    out, bnd = eb.build(streams, ts_end)
    assert out.dtype == torch.int8 and tuple(out.shape) == planes.shape
    assert bnd.dtype == torch.int64 and np.array_equal(bnd.cpu().numpy(), bounds)
    assert np.array_equal(out.cpu().numpy(), planes)
    # a second build reuses the workspace, which the first must have left clean
    out2, bnd2 = eb.build(streams, ts_end)
    assert np.array_equal(out2.cpu().numpy(), planes) and np.array_equal(bnd2.cpu().numpy(), bounds)
    # the three coordinate widths agree
    for coord in _COORD[1:]:
        s2, _, _, _ = load_sequence(name, dev, coord)
        o, b2 = eb.build(s2, ts_end)
        assert np.array_equal(o.cpu().numpy(), planes) and np.array_equal(b2.cpu().numpy(), bounds), coord
    # out= pointing into a larger buffer: nothing outside the addressed windows is written
    cells = int(np.prod(planes.shape))
    pad = 37                                                   # an odd byte offset: the 16-byte stores have to peel
    buf = torch.full((pad + cells + pad,), 0xAB, dtype=torch.uint8, device=dev)
    view = buf[pad:pad + cells].view(torch.int8).view(planes.shape)
    o, _ = eb.build(streams, ts_end, out=view)
    assert o.data_ptr() == view.data_ptr() == buf.data_ptr() + pad
    host = buf.cpu().numpy()
    assert np.array_equal(host[pad:pad + cells].view(np.int8).reshape(planes.shape), planes)
    assert (host[:pad] == 0xAB).all() and (host[pad + cells:] == 0xAB).all()
    # one window in flight equals the default chunking
    one = EventSequenceBuilder(**kw, max_windows_in_flight=1)
    o1, b1 = one.build(streams, ts_end)
    assert np.array_equal(o1.cpu().numpy(), planes) and np.array_equal(b1.cpu().numpy(), bounds)


# ---- 3. element-load path -------------------------------------------------------------------------------------------------------
def test_unaligned_stream_views(backend):
    """Streams that are views at odd element offsets (bases off the 16-byte grid) take the element-load path: same result."""
    dev = backend
    name = 'ds2_small'
    streams, ts_end, bounds, planes = load_sequence(name, dev)
    shifted = []
    for s in streams:
        shifted.append(tuple(torch.cat([a.new_zeros(1), a])[1:] for a in s))
        assert shifted[-1][0].data_ptr() % 16 != 0
    out, bnd = EventSequenceBuilder(**sequence_kwargs(name)).build(shifted, ts_end)
    assert np.array_equal(out.cpu().numpy(), planes) and np.array_equal(bnd.cpu().numpy(), bounds)


# ---- 4. the sequence against the one-window entry at shapes the fixtures lack -----------------------------------------------------
def _host_stream(n, H, W, span, seed, neg_pol=False):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, W, n).astype(np.int16)
    y = rng.integers(0, H, n).astype(np.int16)
    p = rng.integers(-1 if neg_pol else 0, 2, n).astype(np.int16)
    t = np.sort(rng.integers(0, span, n)).astype(np.int64) + 1_000_000
    return tuple(torch.from_numpy(a) for a in (x, y, p, t))


@pytest.mark.parametrize('H,W,ds,cutoff', [(36, 64, True, None), (36, 64, False, 4), (15, 21, True, 3), (15, 21, False, None)])
def test_sequence_equals_construct_per_window(backend, H, W, ds, cutoff):
    """36 x 64 -> 18 x 32 = 576 pixels per plane (16-byte store path, also at full size); 15 x 21 -> 7 x 10 and 315 pixels (the
    pixel-per-lane path).  Each window of the sequence equals construct on the window's slice, then [:, 1::2, 1::2]."""
    dev = backend
    bins, B, T, step = 6, 2, 3, 50_000
    streams = [tuple(a.to(dev) for a in _host_stream(6000, H, W, step * T + 9_000, 50 + b)) for b in range(B)]
    ts_end = (1_000_000 + step * torch.arange(1, T + 1)).to(dev)
    eb = EventSequenceBuilder(bins, H, W, count_cutoff=cutoff, downsample_by_2=ds, window_us=step, representation='mixed_density')
    out, bnd = eb.build(streams, ts_end)
    rep = MixedDensityEventStack(bins, H, W, cutoff)
    assert tuple(out.shape) == (T, B) + ((bins, H // 2, W // 2) if ds else (bins, H, W))
    for b, (x, y, p, t) in enumerate(streams):
        tc = t.cpu().numpy()
        end = np.searchsorted(tc, ts_end.cpu().numpy(), side='right')
        start = np.searchsorted(tc, ts_end.cpu().numpy() - step, side='left')
        assert np.array_equal(bnd[b].cpu().numpy(), np.stack([start, end], -1))
        for w in range(T):
            i0, i1 = int(start[w]), int(end[w])
            assert i1 - i0 > 1000
            full = rep.construct(x[i0:i1], y[i0:i1], p[i0:i1], t[i0:i1])
            want = full[:, 1::2, 1::2] if ds else full
            assert torch.equal(out[w, b], want), (b, w)
    assert int(out.abs().max()) >= (cutoff if cutoff is not None else 3)


# ---- 5. a window far beyond the span contract ---------------------------------------------------------------------------------------
def _exponent_rule(x, y, p, t, bins, H, W, cutoff):
    """The device's rule restated with numpy: fp32 normalised time, clamp, bin = max(bins + floor(log2(tn)), 0) read off frexp
    (exact: no logarithm), +-1 scatter, running sum over the bins, int8 wrap, clamp."""
    den = np.float32(max(int(t[-1] - t[0]), 1))
    tn = (t - t[0]).astype(np.float32) / den
    tn = np.clip(tn, np.float32(1e-6), np.float32(1 - 1e-6))
    assert tn.dtype == np.float32
    e = np.frexp(tn)[1].astype(np.int64) - 1                  # tn = m * 2^exp with 0.5 <= m < 1: floor(log2(tn)) = exp - 1
    b = np.maximum(bins + e, 0)
    img = np.zeros((bins, H, W), dtype=np.int64)
    np.add.at(img, (b, y, x), 2 * np.clip(p, 0, 1) - 1)
    out = np.cumsum(img, 0).astype(np.int8)                   # int64 -> int8 keeps the low 8 bits
    if cutoff is not None:
        out = np.clip(out, -cutoff, cutoff)
    return out, b


def test_large_span_window_takes_the_exact_bin(backend):
    """Span 2^24 us.  Offsets 8 388 605 .. 8 388 607 lie 3, 2, 1 fp32 steps of tn below 1/2: bin bins - 2, where the reference's
    fp32 log quotient rounds to an integer and answers bins - 1 (8 388 606: reference bin 9 of 10, exact bin 8).  The device must
    give the exact bin, so the expectation is the numpy restatement of the exponent rule and NOT the reference."""
    dev = backend
    bins, H, W = 10, 8, 16
    offs = np.array([0, 4_194_303, 8_388_605, 8_388_606, 8_388_607, 8_388_608, 8_388_609, 1 << 24], dtype=np.int64)
    n = offs.size
    x, y, p = np.arange(n, dtype=np.int64), np.full(n, 3, dtype=np.int64), np.ones(n, dtype=np.int64)
    t = 1_000_000 + offs
    want, b = _exponent_rule(x, y, p, t, bins, H, W, None)
    assert b.tolist() == [0, 7, 8, 8, 8, 9, 9, 9]
    ev = [torch.from_numpy(a).to(dev) for a in (x, y, p, t)]
    got = MixedDensityEventStack(bins, H, W).construct(*ev)
    assert np.array_equal(got.cpu().numpy(), want)
    eb = EventSequenceBuilder(bins, H, W, window_us=1 << 25, representation='mixed_density')
    seq, bnd = eb.build([tuple(a.to(torch.int32) for a in ev[:3]) + (ev[3],)], torch.tensor([int(t[-1])], device=dev))
    assert bnd.cpu().tolist() == [[[0, n]]] and np.array_equal(seq[0, 0].cpu().numpy(), want)


# ---- 6. graph capture (GPU only) ---------------------------------------------------------------------------------------------------
def _device_stream(n, H, W, span, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(0, W, (n,), generator=g, device=dev).to(torch.int16)
    y = torch.randint(0, H, (n,), generator=g, device=dev).to(torch.int16)
    p = torch.randint(0, 2, (n,), generator=g, device=dev).to(torch.int16)
    t = torch.sort(torch.randint(0, span, (n,), generator=g, device=dev)).values + 1_000_000
    return x, y, p, t


@pytest.mark.gpu
def test_graph_capture_and_replay():
    """build_from_table captured in a graph; events, counts and window ends rewritten in place; the replay equals an eager build
    of the new data."""
    dev = torch.device('cuda', 0)
    _lib._install_test_library(None)
    H, W, bins, B, T, step, cap = 240, 304, 10, 2, 3, 50_000, 60_000
    kw = dict(count_cutoff=32, downsample_by_2=True, window_us=step, representation='mixed_density')
    eb = EventSequenceBuilder(bins, H, W, **kw)
    bufs = [tuple(a.clone() for a in _device_stream(cap, H, W, step * T, 20 + b, dev)) for b in range(B)]
    ts_end = 1_000_000 + step * torch.arange(1, T + 1, device=dev)
    table = eb.make_table(bufs, ts_end)
    out = torch.empty((T, B) + eb.get_shape(), dtype=torch.int8, device=dev)
    bnd = torch.empty(B, T, 2, dtype=torch.int64, device=dev)
    eb.build_from_table(table, out, bnd)                            # allocates the workspace ahead of the capture
    first = out.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eb.build_from_table(table, out, bnd)
    for k, counts in enumerate(([40_000, 25_001], [cap, 7])):
        fresh = [_device_stream(n, H, W, step * T, 30 + 2 * k + b, dev) for b, n in enumerate(counts)]
        for buf, new, n in zip(bufs, fresh, counts):
            for a, v in zip(buf, new):
                a[:n].copy_(v)
        ts_end.add_(3_000)
        eb.write_table(table, counts=counts)
        out.fill_(7)
        bnd.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want, want_b = EventSequenceBuilder(bins, H, W, **kw).build(fresh, ts_end)
        assert torch.equal(bnd, want_b) and torch.equal(out, want)
        assert not torch.equal(out, first)


# ---- 7. argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    dev = backend
    name = 'ds2_small'
    streams, ts_end, _, planes = load_sequence(name, dev)
    kw = sequence_kwargs(name)
    for bad in (128, -1):
        with pytest.raises(ValueError, match='count_cutoff'):
            EventSequenceBuilder(**dict(kw, count_cutoff=bad))
    with pytest.raises(ValueError, match='representation'):
        EventSequenceBuilder(**dict(kw, representation='voxel_grid'))
    with pytest.raises(ValueError, match='fastmode'):
        EventSequenceBuilder(**kw, fastmode=False)
    eb = EventSequenceBuilder(**kw)
    with pytest.raises(ValueError, match='out must be'):
        eb.build(streams, ts_end, out=torch.empty(planes.shape, dtype=torch.uint8, device=dev))
    # the histogram builder keeps its own rules: cutoff 0 is still refused there, int8 out too
    with pytest.raises(ValueError, match='count_cutoff'):
        EventSequenceBuilder(10, 24, 32, count_cutoff=0, window_us=1000)
    hist = EventSequenceBuilder(10, 24, 32, downsample_by_2=True, window_us=50_000)
    assert hist.representation == 'stacked_histogram' and hist.get_shape() == (20, 12, 16)
    with pytest.raises(ValueError, match='out must be'):
        hist.build(streams, ts_end, out=torch.empty((6, 2, 20, 12, 16), dtype=torch.int8, device=dev))


# ---- 8. int8 planes into the backbone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_backbone_takes_int8_planes(backend, dtype):
    """forward_sequence(int8 planes) equals forward_sequence(planes.float()) bit for bit, on the no-grad route and on the autograd
    route, and reaches the compute dtype through rvt_prepack_input with source kind 2 (no float32 copy of the planes)."""
    from tests.test_backbone import make_cfg
    dev = backend
    bins, T, B = 10, 2, 2
    cfg = make_cfg('micro')
    cfg['input_channels'] = bins
    torch.manual_seed(0)
    m = RNNDetector(cfg, compute_dtype=dtype).to(dev)
    assert m.in_channels == bins
    h, w = casegen.CASES['micro']['hw']
    planes = torch.from_numpy(np.random.default_rng(3).integers(-128, 128, (T, B, bins, h, w)).astype(np.int8)).to(dev)
    calls = []
    orig = _lib.call

    def rec(name, *args):
        calls.append((name, args))
        return orig(name, *args)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            want_f, want_s = m.forward_sequence(planes.float())
            del calls[:]
            _lib.call = rec
            try:
                got_f, got_s = m.forward_sequence(planes)
            finally:
                _lib.call = orig
        kinds = [LaunchArgs(n, a).src_kind for n, a in calls if n == 'rvt_prepack_input']
        assert kinds == [2], (grad, kinds)
        assert sorted(got_f) == sorted(want_f) == [1, 2, 3, 4]
        for k in want_f:
            assert got_f[k].dtype == want_f[k].dtype and torch.equal(got_f[k], want_f[k]), (grad, k)
        for (gh, gc), (wh, wc) in zip(got_s, want_s):
            assert torch.equal(gh, wh) and torch.equal(gc, wc), grad
        assert float(got_f[4].detach().float().abs().max()) > 0
