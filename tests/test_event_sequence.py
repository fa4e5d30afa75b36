"""Raw event streams -> (T, B, 2*bins, H', W') window sequences on the device (rvt_amd.representations.EventSequenceBuilder,
csrc/evseq.hpp) against fixtures recorded from the reference's own composition (tests/make_golden_evseq.py: numpy searchsorted,
one StackedHistogram.construct per window, interpolate(scale_factor=0.5, mode='nearest-exact')).  Integer work: bit-exact."""
import os

import numpy as np
import pytest
import torch

from rvt_amd.representations import EventSequenceBuilder, StackedHistogram
from tests.backends import backend  # noqa: F401
from tests.casegen_evseq import CASES, builder_kwargs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_COORD = (torch.int16, torch.int32, torch.int64)


def load_case(name, dev, coord=torch.int16):
    g = np.load(os.path.join(GOLD, f'evseq_{name}.npz'))
    B = g['bounds'].shape[0]
    # clone: torch's own allocation, 64-byte aligned on either backend (the 16-byte load path)
    streams = [tuple(torch.from_numpy(g[f'{k}{b}']).to(coord).clone().to(dev) for k in 'xyp') + (torch.from_numpy(g[f't{b}']).clone().to(dev),)
               for b in range(B)]
    assert all(a.data_ptr() % 16 == 0 for s in streams for a in s)
    return streams, torch.from_numpy(g['ts_end']).to(dev), g['bounds'], g['planes']


@pytest.mark.parametrize('name', list(CASES))
def test_matches_reference_fixture(backend, name):
    dev = backend
    kw = builder_kwargs(CASES[name])
    streams, ts_end, bounds, planes = load_case(name, dev)
    T, B = planes.shape[:2]
    eb = EventSequenceBuilder(**kw)
    assert eb.get_shape() == planes.shape[2:]
    out, bnd = eb.build(streams, ts_end)
    assert out.dtype == torch.uint8 and tuple(out.shape) == planes.shape
    assert bnd.dtype == torch.int64 and np.array_equal(bnd.cpu().numpy(), bounds)
    assert np.array_equal(out.cpu().numpy(), planes)
    # a second build reuses the workspace, which the first must have left clean
    out2, bnd2 = eb.build(streams, ts_end)
    assert np.array_equal(out2.cpu().numpy(), planes) and np.array_equal(bnd2.cpu().numpy(), bounds)
    # the three coordinate widths agree
    for coord in _COORD[1:]:
        s2, _, _, _ = load_case(name, dev, coord)
        o, b2 = eb.build(s2, ts_end)
        assert np.array_equal(o.cpu().numpy(), planes) and np.array_equal(b2.cpu().numpy(), bounds), coord
    # out= pointing into a larger buffer: nothing outside the addressed windows is written
    cells = int(np.prod(planes.shape))
    pad = 37                                                   # an odd byte offset: the 16-byte stores have to peel
    buf = torch.full((pad + cells + pad,), 0xAB, dtype=torch.uint8, device=dev)
    view = buf[pad:pad + cells].view(planes.shape)
    o, _ = eb.build(streams, ts_end, out=view)
    assert o.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(host[pad:pad + cells].reshape(planes.shape), planes)
    assert (host[:pad] == 0xAB).all() and (host[pad + cells:] == 0xAB).all()
    # one window in flight equals the default chunking
    one = EventSequenceBuilder(**kw, max_windows_in_flight=1)
    o1, b1 = one.build(streams, ts_end)
    assert np.array_equal(o1.cpu().numpy(), planes) and np.array_equal(b1.cpu().numpy(), bounds)


def test_unaligned_stream_views(backend):
    """Streams that are views at odd element offsets (bases off the 16-byte grid) take the element-load path: same result."""
    dev = backend
    name = 'ds2_small'
    streams, ts_end, bounds, planes = load_case(name, dev)
    shifted = []
    for s in streams:
        shifted.append(tuple(torch.cat([a.new_zeros(1), a])[1:] for a in s))
        assert shifted[-1][0].data_ptr() % 16 != 0
    out, bnd = EventSequenceBuilder(**builder_kwargs(CASES[name])).build(shifted, ts_end)
    assert np.array_equal(out.cpu().numpy(), planes) and np.array_equal(bnd.cpu().numpy(), bounds)


def test_table_counts_and_rewrite(backend):
    """The event count is read from the table: a stream buffer used up to n < capacity gives the result of the shorter stream,
    and write_table switches an existing table to new counts / window ends in place."""
    dev = backend
    name = 'ds2_small'
    kw = builder_kwargs(CASES[name])
    streams, ts_end, bounds, planes = load_case(name, dev)
    eb = EventSequenceBuilder(**kw)
    counts = [int(s[3].numel()) // 2 for s in streams]
    want, want_b = eb.build([tuple(a[:n].clone() for a in s) for s, n in zip(streams, counts)], ts_end)
    table = eb.make_table(streams, ts_end, counts)
    got, got_b = eb.build_from_table(table)
    assert torch.equal(got, want) and torch.equal(got_b, want_b)
    assert not np.array_equal(got.cpu().numpy(), planes)
    eb.write_table(table, counts=[int(s[3].numel()) for s in streams])
    got, got_b = eb.build_from_table(table)
    assert np.array_equal(got.cpu().numpy(), planes) and np.array_equal(got_b.cpu().numpy(), bounds)


def test_argument_checks(backend):
    dev = backend
    streams, ts_end, _, planes = load_case('ds2_small', dev)
    kw = builder_kwargs(CASES['ds2_small'])
    with pytest.raises(ValueError, match='exactly one'):
        EventSequenceBuilder(10, 24, 32)
    with pytest.raises(ValueError, match='exactly one'):
        EventSequenceBuilder(10, 24, 32, window_us=1000, window_events=10)
    eb = EventSequenceBuilder(**kw)
    with pytest.raises(TypeError, match='int64'):
        eb.build(streams, ts_end.to(torch.int32))
    with pytest.raises(ValueError, match=r'\(3, 2\)'):
        eb.build(streams, ts_end.new_zeros(3, 2))
    x, y, p, t = streams[0]
    with pytest.raises(TypeError, match='torch.int32'):
        eb.build([(x, y.to(torch.int32), p, t)], ts_end)
    with pytest.raises(TypeError, match='torch.float32'):
        eb.build([(x.float(), y.float(), p.float(), t)], ts_end)
    with pytest.raises(TypeError, match='t must be int64'):
        eb.build([(x, y, p, t.to(torch.int32))], ts_end)
    with pytest.raises(ValueError, match='one length'):
        eb.build([(x[:-1], y, p, t)], ts_end)
    with pytest.raises(ValueError, match='out must be'):
        eb.build(streams, ts_end, out=torch.empty(planes.shape[1:], dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='bounds_out must be'):
        eb.build(streams, ts_end, bounds_out=torch.empty(2, 6, 2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='capacity'):
        eb.make_table(streams, ts_end, counts=[t.numel() + 1, 0])


# ------------------------------------------------------------------------------------------------------------ GPU only
def _device_stream(n, H, W, span, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(0, W, (n,), generator=g, device=dev).to(torch.int16)
    y = torch.randint(0, H, (n,), generator=g, device=dev).to(torch.int16)
    p = torch.randint(0, 2, (n,), generator=g, device=dev).to(torch.int16)
    t = torch.sort(torch.randint(0, span, (n,), generator=g, device=dev)).values + 1_000_000
    return x, y, p, t


def _per_window_route(streams, ts_end, delta, bins, H, W, cutoff, fastmode, ds):
    """What the parent offers: torch.searchsorted + one StackedHistogram.construct per window (+ the odd-pixel selection)."""
    rep = StackedHistogram(bins, H, W, cutoff, fastmode)
    T = ts_end.numel()
    frames, bounds = [], []
    for x, y, p, t in streams:
        end = torch.searchsorted(t, ts_end, right=True)
        start = torch.searchsorted(t, ts_end - delta, right=False)
        bounds.append(torch.stack([start, end], -1))
        row = []
        for w in range(T):
            i0, i1 = int(start[w]), int(end[w])
            full = rep.construct(x[i0:i1], y[i0:i1], p[i0:i1], t[i0:i1])
            row.append(full[..., 1::2, 1::2] if ds else full)
        frames.append(torch.stack(row, 0))
    return torch.stack(frames, 1).contiguous(), torch.stack(bounds, 0)


@pytest.mark.gpu
def test_full_size_1mpx_against_per_window_kernel():
    """720 x 1280 -> 360 x 640, B 2, T 3, 2 M events: bit-equal to the existing per-window kernel on each window's slice followed
    by [..., 1::2, 1::2], bounds equal to torch.searchsorted."""
    dev = torch.device('cuda', 0)
    H, W, bins, B, T, step = 720, 1280, 10, 2, 3, 50_000
    streams = [_device_stream(1_000_000, H, W, step * T + 10_000, 10 + b, dev) for b in range(B)]
    ts_end = 1_000_000 + step * torch.arange(1, T + 1, device=dev)
    eb = EventSequenceBuilder(bins, H, W, count_cutoff=10, fastmode=True, downsample_by_2=True, window_us=step)
    out, bnd = eb.build(streams, ts_end)
    want, want_b = _per_window_route(streams, ts_end, step, bins, H, W, 10, True, True)
    assert tuple(out.shape) == (T, B, 2 * bins, H // 2, W // 2)
    assert torch.equal(bnd, want_b)
    assert int((bnd[..., 1] - bnd[..., 0]).min()) > 250_000
    assert torch.equal(out, want)
    assert int(out.sum(dtype=torch.int64)) > 300_000                # about a quarter of the events land on odd pixels


@pytest.mark.gpu
def test_graph_capture_and_replay():
    """build_from_table captured in a graph; events, counts and window ends rewritten in place; the replay equals an eager build
    of the new data."""
    dev = torch.device('cuda', 0)
    H, W, bins, B, T, step, cap = 240, 304, 10, 2, 3, 50_000, 60_000
    eb = EventSequenceBuilder(bins, H, W, count_cutoff=10, downsample_by_2=True, window_us=step)
    bufs = [tuple(a.clone() for a in _device_stream(cap, H, W, step * T, 20 + b, dev)) for b in range(B)]
    ts_end = 1_000_000 + step * torch.arange(1, T + 1, device=dev)
    table = eb.make_table(bufs, ts_end)
    out = torch.empty((T, B) + eb.get_shape(), dtype=torch.uint8, device=dev)
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
        want, want_b = EventSequenceBuilder(bins, H, W, count_cutoff=10, downsample_by_2=True, window_us=step).build(fresh, ts_end)
        assert torch.equal(bnd, want_b) and torch.equal(out, want)
        assert not torch.equal(out, first)


@pytest.mark.gpu
def test_builder_feeds_the_backbone():
    """The builder's output goes straight into RNNDetector.forward_sequence and gives the features of the per-window route."""
    from tests import casegen
    from tests.test_backbone import build_model
    dev = torch.device('cuda', 0)
    m = build_model('micro', dev, torch.float32)
    h, w = casegen.CASES['micro']['hw']
    H, W, bins, B, T, step = 2 * h, 2 * w, 10, 2, 2, 50_000
    streams = [_device_stream(40_000, H, W, step * T, 40 + b, dev) for b in range(B)]
    ts_end = 1_000_000 + step * torch.arange(1, T + 1, device=dev)
    planes, _ = EventSequenceBuilder(bins, H, W, count_cutoff=10, downsample_by_2=True, window_us=step).build(streams, ts_end)
    want, _ = _per_window_route(streams, ts_end, step, bins, H, W, 10, True, True)
    assert torch.equal(planes, want) and int(planes.max()) > 0
    with torch.no_grad():
        got_f, _ = m.forward_sequence(planes)
        want_f, _ = m.forward_sequence(want)
    assert all(torch.equal(got_f[k], want_f[k]) for k in want_f)
