"""What comes before the event stream, on the device (rvt_amd/csrc/evprep.hpp): the timestamp repair against numpy's running maximum
and the decode of packed Prophesee records against fixtures recorded from the reference's reader (tests/make_golden_recordings.py:
load_td_data and H5Reader._correct_time).  Integer work: everything is bit-exact."""
import os

import numpy as np
import pytest
import torch

from rvt_amd.recordings import DatDecoder
from rvt_amd.representations import EventSequenceBuilder, prep_blocks, repair_time
from tests.backends import backend  # noqa: F401
from tests.casegen_evseq import CASES, builder_kwargs
from tests.casegen_recordings import DAT_CASES

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIZES = (0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 129, 511, 513, 2047, 2049, 4095, 4097, 6149, 20001)
BLOCKS = (0, 1, 2, 3, 7, 64)
PATTERNS = ('sorted', 'spike_first', 'spike_span_end', 'random_steps', 'all_equal', 'negatives', 'high_word', 'low_word_misleads')
SENTINEL = -0x5151515151515151


def span_of(n, K):
    """Events per workgroup, as the kernels cut a stream (rvt_amd/csrc/evprep.hpp: evprep_span)."""
    return (-(-n // K) + 7) & ~7


def make_t(pattern, n, K, seed):
    rng = np.random.default_rng(seed)
    t = 1_000 + np.cumsum(rng.integers(0, 50, n)).astype(np.int64)
    if pattern == 'sorted' or n == 0:
        return t
    if pattern == 'spike_first':                         # the prefix has to cross every span
        t[0] = t[-1] + 1_000
    elif pattern == 'spike_span_end':                    # the last element of the first span (of the stream, when one span holds it)
        t[min(span_of(n, K), n) - 1] = t[-1] + 7
    elif pattern == 'random_steps':
        idx = rng.choice(n, size=max(1, n // 10), replace=False)
        t[idx] -= rng.integers(1, 5_000, idx.size)
    elif pattern == 'all_equal':
        t[:] = 123_456
    elif pattern == 'negatives':                         # the repair starts at 0: negative timestamps become 0
        t = rng.integers(-1_000, 50, n).astype(np.int64)
    elif pattern == 'high_word':                         # order decided by bits 32 and up alone
        t = (rng.integers(0, 6, n).astype(np.int64) << 32) | 0x1234
    elif pattern == 'low_word_misleads':                 # 2^32 + 1 before 2^33, 2^33 + 5 before 2^32 + 9: the low words order them the other way
        base = np.array([2 ** 32 + 1, 2 ** 33, 2 ** 33 + 5, 2 ** 32 + 9], dtype=np.int64)
        t = base[np.arange(n) % 4] + (np.arange(n, dtype=np.int64) // 4) * 2
    return t


def want_repair(t, c=0):
    return np.maximum.accumulate(np.maximum(t, c)) if t.size else t.copy()


def streams_of(ts, dev):
    """Streams around the given timestamp arrays; torch's own allocations are 64-byte aligned (the 16-byte access path)."""
    out = []
    for t in ts:
        z = torch.zeros(t.size, dtype=torch.int16, device=dev)
        out.append((z, z, z, torch.from_numpy(t.copy()).to(dev)))
    return out


def check_repair_call(ns, pats, K, seed, dev):
    B = len(ns)
    kk = K or prep_blocks(B)
    ts = [make_t(pats[b], n, kk, seed + b) for b, n in enumerate(ns)]
    streams = streams_of(ts, dev)
    rep = repair_time(streams, out_repaired=True, blocks_per_stream=K)
    assert tuple(rep.shape) == (B, kk)
    for b, t in enumerate(ts):
        want = want_repair(t)
        got = streams[b][3].cpu().numpy()
        assert np.array_equal(got, want), (pats[b], ns, b)
        assert int(rep[b].sum()) == int((want != t).sum()), (pats[b], ns, b)
        if pats[b] in ('sorted', 'all_equal'):
            assert int(rep[b].sum()) == 0


@pytest.mark.parametrize('K', BLOCKS)
def test_scan_matches_numpy(backend, K):
    """Every size x every pattern for every grid.  Three streams of different length (one of them empty) per call: ten calls
    cover the nineteen sizes.  The library's own grid (K = 0) is some 2048 workgroups per call whatever B is, which costs the
    emulator a third of a second per call; there the product runs as one call per pattern with all nineteen sizes as its
    streams (K = 107), and the B = 3 grid (K = 682) sees two calls.  The GPU runs the B = 3 product for K = 0 too."""
    dev = backend
    if K == 0 and dev.type != 'cuda':
        for pi, pattern in enumerate(PATTERNS):
            check_repair_call(SIZES, (pattern,) * len(SIZES), 0, 1000 * pi, dev)
        check_repair_call((20001, 6149, 0), ('random_steps', 'spike_first', 'sorted'), 0, 7, dev)
        check_repair_call((4097, 0, 513), ('low_word_misleads', 'sorted', 'negatives'), 0, 8, dev)
        return
    for pi, pattern in enumerate(PATTERNS):
        for si in range(10):
            ns = (SIZES[si], SIZES[(si + 10) % len(SIZES)], 0)
            check_repair_call(ns, (pattern,) * 3, K, 100 * pi + 3 * si, dev)


def test_patterns_do_what_they_say():
    """The inputs themselves: the spike patterns need the prefix of another span, the 64-bit patterns fool a 32-bit comparison."""
    n, K = 6149, 7
    t = make_t('spike_first', n, K, 0)
    assert (want_repair(t) == t[0]).all()
    t = make_t('spike_span_end', n, K, 0)
    s = span_of(n, K)
    assert (want_repair(t)[s - 1:] == t[s - 1]).all() and (want_repair(t)[:s - 1] == t[:s - 1]).all()
    t = make_t('low_word_misleads', 8, 1, 0)
    assert t[0] < t[1] and (t[0] & 0xffffffff) > (t[1] & 0xffffffff) and t[2] > t[3] and (t[2] & 0xffffffff) < (t[3] & 0xffffffff)
    t = make_t('high_word', 513, 1, 0)
    assert np.unique(t & 0xffffffff).size == 1 and int((want_repair(t) != t).sum()) > 100
    assert int((want_repair(make_t('negatives', 513, 1, 0)) == 0).sum()) > 0


@pytest.mark.parametrize('K', (0, 3))
def test_carry_chunks_equal_one_shot(backend, K):
    dev = backend
    n = 6149
    t = make_t('random_steps', n, 3, 5)
    t[100] = t[3000]                                     # a spike whose reach crosses the chunk borders below
    want = want_repair(t)
    for cut in (1, 64, 65, 2048, n - 1):
        carry = torch.zeros(1, dtype=torch.int64, device=dev)
        a, b = streams_of([t[:cut], t[cut:]], dev)
        repair_time([a], carry=carry, blocks_per_stream=K)
        assert int(carry[0]) == int(want[cut - 1])
        repair_time([b], carry=carry, blocks_per_stream=K)
        got = np.concatenate([a[3].cpu().numpy(), b[3].cpu().numpy()])
        assert np.array_equal(got, want), cut
        assert int(carry[0]) == int(want[-1])
    # a carry-in above every timestamp flattens the chunk, and stays
    top = int(t.max()) + 5
    carry = torch.tensor([top, 0], dtype=torch.int64, device=dev)
    s = streams_of([t, t], dev)
    rep = repair_time(s, carry=carry, out_repaired=True, blocks_per_stream=K)
    assert (s[0][3].cpu().numpy() == top).all() and int(rep[0].sum()) == n
    assert np.array_equal(s[1][3].cpu().numpy(), want)
    assert carry.cpu().tolist() == [top, int(want[-1])]
    # an empty chunk hands the carry on
    carry = torch.tensor([77], dtype=torch.int64, device=dev)
    repair_time(streams_of([t[:0]], dev), carry=carry, blocks_per_stream=K)
    assert int(carry[0]) == 77


@pytest.mark.parametrize('K', (0, 2))
def test_in_place_and_contained(backend, K):
    """A stream that is a view at an odd element offset of a larger buffer (base off the 16-byte grid), used up to n < capacity:
    the same result, and nothing in front of it or behind n is touched."""
    dev = backend
    n, cap, front = 4097, 4200, 3
    t = make_t('random_steps', n, 2, 9)
    buf = torch.full((front + cap + 5,), SENTINEL, dtype=torch.int64, device=dev)
    view = buf[front:front + cap]
    assert view.data_ptr() % 16 == 8
    view[:n].copy_(torch.from_numpy(t))
    z = torch.zeros(cap, dtype=torch.int16, device=dev)
    table = EventSequenceBuilder(1, 1, 1, window_us=1).make_table([(z, z, z, view)], torch.zeros(1, dtype=torch.int64, device=dev), counts=[n])
    rep = repair_time(table, out_repaired=True, blocks_per_stream=K)
    host = buf.cpu().numpy()
    want = want_repair(t)
    assert np.array_equal(host[front:front + n], want) and int(rep.sum()) == int((want != t).sum())
    assert (host[:front] == SENTINEL).all() and (host[front + n:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ decode
def load_dat_case(name):
    g = np.load(os.path.join(GOLD, f'rec_dat_{name}.npz'))
    off = int(g['header'][0])
    return g, g['raw'][off:]


def records_tensor(body, dev, misalign=False):
    """The record bytes as a device tensor in a fresh allocation; misalign: at an 8-byte but not 16-byte aligned address."""
    if not misalign:
        r = torch.from_numpy(body.copy()).to(dev).clone()
        assert r.data_ptr() % 16 == 0
        return r
    buf = torch.zeros(body.size + 8, dtype=torch.uint8, device=dev)
    r = buf[8:]
    r.copy_(torch.from_numpy(body.copy()))
    assert r.data_ptr() % 16 == 8
    return r


def check_stream(dec, b, g, n, t_key):
    x, y, p, t = (a.cpu().numpy() for a in dec.streams[b])
    assert np.array_equal(x[:n], g['x'][:n]) and np.array_equal(y[:n], g['y'][:n]) and np.array_equal(p[:n], g['p'][:n])
    assert np.array_equal(t[:n], g[t_key][:n])
    return x, y, p, t


@pytest.mark.parametrize('name', list(DAT_CASES))
def test_decode_matches_reference_reader(backend, name):
    dev = backend
    g, body = load_dat_case(name)
    n = g['t'].size
    assert body.size == 8 * n
    for coord in (torch.int16, torch.int32, torch.int64):
        for repair, t_key in ((False, 't'), (True, 't_repaired')):
            dec = DatDecoder(1, n, dev, coord=coord, repair=repair)
            table = dec.decode([records_tensor(body, dev)])
            assert dec.counts() == [n] and table is dec.table
            x, _, _, t = check_stream(dec, 0, g, n, t_key)
            assert x.dtype == {torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}[coord] and t.dtype == np.int64
            if repair:
                assert int(dec.repaired.sum()) == int((g['t_repaired'] != g['t']).sum())
                assert int(dec.carry[0]) == int(g['t_repaired'][-1])
    # int64 words instead of bytes, at an address off the 16-byte grid, through a small explicit grid
    dec = DatDecoder(1, n, dev, blocks_per_stream=3)
    dec.decode([records_tensor(body, dev, misalign=True).view(torch.int64)])
    check_stream(dec, 0, g, n, 't_repaired')


def test_decode_counts_and_capacity(backend):
    """n_records below the capacity and above it (clamped); nothing behind n is written; two streams per call; the carry joins
    consecutive decodes of one stream until reset()."""
    dev = backend
    g, body = load_dat_case('v2_header')
    g2, body2 = load_dat_case('legacy')
    n, n2 = g['t'].size, g2['t'].size
    cap, room = 2500, 300                                # the capacity lies below both recordings, the arrays go on behind it
    dec = DatDecoder(2, cap + room, dev, coord=torch.int16, blocks_per_stream=3)
    dec.capacity = cap                                   # what the entry is told: the last `room` elements are not its to write
    for s in dec.streams:
        for a in s:
            a.fill_(-21555)
    dec.decode([records_tensor(body, dev), records_tensor(body2, dev)], counts=[777, n2])
    assert n2 > cap + room and dec.counts() == [777, cap]            # clamped to the capacity, not to the arrays
    for b, (gg, nn) in enumerate(((g, 777), (g2, cap))):         # (the repair of a prefix is the prefix of the repair)
        x, y, p, t = check_stream(dec, b, gg, nn, 't_repaired')
        assert all(a.size == cap + room and a[nn:].size >= room and (a[nn:] == -21555).all() for a in (x, y, p, t))
    assert dec.carry.cpu().tolist() == [int(g['t_repaired'][776]), int(g2['t_repaired'][cap - 1])]
    # the second half of stream 0 continues the first: together the repair of the whole file
    first = dec.streams[0][3][:777].cpu().numpy().copy()
    dec.decode([records_tensor(body[8 * 777:], dev), records_tensor(body2[:0], dev)])
    assert dec.counts() == [n - 777, 0]
    got = np.concatenate([first, dec.streams[0][3][:n - 777].cpu().numpy()])
    assert np.array_equal(got, g['t_repaired'])
    dec.reset()
    assert dec.carry.cpu().tolist() == [0, 0]
    with pytest.raises(ValueError, match='8-byte aligned'):
        dec.decode([records_tensor(body, dev)[4:-4], records_tensor(body2, dev)])
    with pytest.raises(ValueError, match='whole number'):
        dec.decode([records_tensor(body, dev)[:-3], records_tensor(body2, dev)])


# ----------------------------------------------------------------------------------------------------------------- builder
def _fixture_with_steps(dev):
    """Stream fixture 'ds2_small' with backward steps injected into its timestamps, and the numpy-repaired version."""
    name = 'ds2_small'
    g = np.load(os.path.join(GOLD, f'evseq_{name}.npz'))
    B = g['bounds'].shape[0]
    raw, fixed = [], []
    for b in range(B):
        t = g[f't{b}'].copy()
        rng = np.random.default_rng(40 + b)
        idx = rng.choice(t.size - 1, size=max(4, t.size // 6), replace=False) + 1
        t[idx] -= rng.integers(1, max(2, int(t[-1] - t[0]) // 3), idx.size)
        raw.append(t)
        fixed.append(want_repair(t))
        assert (fixed[-1] != t).any()
    def to_streams(ts):
        return [tuple(torch.from_numpy(g[f'{k}{b}']).clone().to(dev) for k in 'xyp') + (torch.from_numpy(ts[b].copy()).to(dev),) for b in range(B)]
    return name, g, raw, fixed, to_streams


def test_builder_repairs_ahead_of_the_bounds(backend):
    dev = backend
    name, g, raw, fixed, to_streams = _fixture_with_steps(dev)
    kw = builder_kwargs(CASES[name])
    ts_end = torch.from_numpy(g['ts_end']).to(dev)
    want, want_b = EventSequenceBuilder(**kw).build(to_streams(fixed), ts_end)
    broken, broken_b = EventSequenceBuilder(**kw).build(to_streams(raw), ts_end)
    assert not torch.equal(broken, want)                 # without the repair the planes differ: the check below is not trivial
    streams = to_streams(raw)
    eb = EventSequenceBuilder(**kw, repair_time=True)
    got, got_b = eb.build(streams, ts_end)
    assert torch.equal(got, want) and torch.equal(got_b, want_b)
    for b in range(len(streams)):
        assert np.array_equal(streams[b][3].cpu().numpy(), fixed[b])         # and t is left repaired
    got2, got2_b = eb.build(streams, ts_end)             # again on the repaired streams: the same
    assert torch.equal(got2, want) and torch.equal(got2_b, want_b)
    # off by default: the untouched fixture gives what it gave before
    clean = to_streams([g[f't{b}'] for b in range(len(streams))])
    out, bnd = EventSequenceBuilder(**kw).build(clean, ts_end)
    assert np.array_equal(out.cpu().numpy(), g['planes']) and np.array_equal(bnd.cpu().numpy(), g['bounds'])
    out, bnd = EventSequenceBuilder(**kw, repair_time=True).build(clean, ts_end)
    assert np.array_equal(out.cpu().numpy(), g['planes']) and np.array_equal(bnd.cpu().numpy(), g['bounds'])


def test_argument_checks(backend):
    dev = backend
    s = streams_of([np.arange(10, dtype=np.int64)], dev)
    with pytest.raises(ValueError, match='carry'):
        repair_time(s, carry=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match='carry'):
        repair_time(s, carry=torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='out of range'):
        repair_time(s, blocks_per_stream=5000)
    with pytest.raises(ValueError, match='ws must be'):
        repair_time(s, ws=torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError, match='uint8 or int64'):
        DatDecoder(1, 8, dev).decode([torch.zeros(8, dtype=torch.int32, device=dev)])


# ---------------------------------------------------------------------------------------------------------------- GPU only
def _packed(n, H, W, span, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, span, n)) + 1_000_000
    idx = rng.choice(n - 1, size=n // 40, replace=False) + 1
    t[idx] -= rng.integers(1, 2_000, idx.size)           # the clock steps back
    w = rng.integers(0, W, n) | (rng.integers(0, H, n) << 14) | (rng.integers(0, 2, n) << 28) | (rng.integers(0, 8, n) << 29)
    rec = np.zeros(n, dtype=[('t', '<u4'), ('w', '<u4')])
    rec['t'], rec['w'] = t.astype(np.uint32), (w & 0xffffffff).astype(np.uint32)
    return torch.from_numpy(rec.view(np.int64).copy())


@pytest.mark.gpu
def test_graph_capture_and_replay():
    """decode + build_from_table captured in one graph; records and counts rewritten in place; the replay equals the eager result."""
    dev = torch.device('cuda', 0)
    H, W, bins, B, T, step, cap = 240, 304, 10, 2, 3, 50_000, 30_000
    eb = EventSequenceBuilder(bins, H, W, count_cutoff=10, downsample_by_2=True, window_us=step)
    dec = DatDecoder(B, cap, dev)
    ts_end = 1_000_000 + step * torch.arange(1, T + 1, device=dev)
    table = dec.set_window_ends(ts_end)
    recs = [torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(B)]

    def load(seed, counts):
        for b, n in enumerate(counts):
            recs[b][:n].copy_(_packed(n, H, W, step * T, seed + b))
        dec.n_records.copy_(torch.tensor(counts))
        dec.reset()

    out = torch.empty((T, B) + eb.get_shape(), dtype=torch.uint8, device=dev)
    bnd = torch.empty(B, T, 2, dtype=torch.int64, device=dev)
    load(50, [cap, cap // 2])
    dec.decode(recs, counts=[cap, cap // 2])             # uploads the record addresses; allocates nothing afterwards
    eb.build_from_table(table, out, bnd)                 # allocates the builder's workspace ahead of the capture
    first = out.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.decode_in_place()
        eb.build_from_table(table, out, bnd)
    for k, counts in enumerate(([20_000, 12_345], [cap, 9])):
        load(60 + 2 * k, counts)
        out.fill_(7)
        bnd.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert dec.counts() == counts
        got_t = [dec.streams[b][3][:n].clone() for b, n in enumerate(counts)]
        eager = DatDecoder(B, cap, dev)
        etab = eager.set_window_ends(ts_end)
        eager.decode([r.clone() for r in recs], counts=counts)
        want, want_b = EventSequenceBuilder(bins, H, W, count_cutoff=10, downsample_by_2=True, window_us=step).build_from_table(etab)
        assert torch.equal(bnd, want_b) and torch.equal(out, want)
        assert all(torch.equal(got_t[b], eager.streams[b][3][:n]) for b, n in enumerate(counts))
        assert all(bool((got_t[b][1:] >= got_t[b][:-1]).all()) for b in range(B))
        assert not torch.equal(out, first) and int(out.sum(dtype=torch.int64)) > 0
