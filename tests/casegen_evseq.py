"""Seeded event streams and window lists for the event-sequence builder tests (shared by the golden recorder and the tests).

make_case(name) -> (params, streams, ts_end): params = the builder's constructor arguments, streams = B tuples (x, y, p, t) of
int64 numpy arrays (t non-decreasing, p may be -1 where the case says so), ts_end int64 [T] or [B][T]."""
import numpy as np

T_BASE = 1_000_000

CASES = {
    # the basic path: two streams into one (T, B, ...) tensor, contiguous 50 ms windows
    'ds2_small': dict(H=24, W=32, bins=10, ds=True, cutoff=10, fastmode=True, window_us=50_000, B=2, T=6, n=3000),
    # 15 x 21 -> 7 x 10: 1400 cells per window (not a multiple of 16; every other window starts 8 bytes off a 16-byte boundary)
    'odd_hw': dict(H=15, W=21, bins=10, ds=True, cutoff=10, fastmode=True, window_us=50_000, B=2, T=3, n=2500),
    'no_ds': dict(H=24, W=32, bins=10, ds=False, cutoff=10, fastmode=True, window_us=50_000, B=1, T=4, n=4000),
    # delta = 2 x step: every event is counted in two windows
    'overlap': dict(H=24, W=32, bins=10, ds=True, cutoff=10, fastmode=True, window_us=100_000, B=1, T=5, n=4000),
    # N = 500 events per window; the first windows hold fewer (start clamps at 0)
    'count_mode': dict(H=24, W=32, bins=10, ds=True, cutoff=10, fastmode=True, window_events=500, B=2, T=4, n=1500),
    'gaps': dict(H=24, W=32, bins=10, ds=True, cutoff=10, fastmode=True, window_us=50_000, B=1, T=4, n=0),
    'edge_ties': dict(H=24, W=32, bins=10, ds=True, cutoff=None, fastmode=True, window_us=50_000, B=1, T=3, n=3000),
    'hot_wrap': dict(H=16, W=16, bins=2, ds=True, cutoff=None, fastmode=True, window_us=50_000, B=1, T=2, n=2000),
    'hot_wrap_int16': dict(H=16, W=16, bins=2, ds=True, cutoff=None, fastmode=False, window_us=50_000, B=1, T=2, n=2000),
    'neg_pol': dict(H=24, W=32, bins=10, ds=True, cutoff=10, fastmode=True, window_us=50_000, B=1, T=3, n=3000),
    'gen1_like': dict(H=240, W=304, bins=10, ds=False, cutoff=10, fastmode=True, window_us=50_000, B=1, T=3, n=100_000),
}


def _uniform(rng, c, n, span):
    x = rng.integers(0, c['W'], n, dtype=np.int64)
    y = rng.integers(0, c['H'], n, dtype=np.int64)
    p = rng.integers(0, 2, n, dtype=np.int64)
    t = np.sort(rng.integers(0, span, n, dtype=np.int64)) + T_BASE
    return x, y, p, t


def make_case(name):
    c = dict(CASES[name])
    rng = np.random.default_rng(sum(map(ord, name.replace('_int16', ''))))      # the two hot_wrap cases share their streams
    B, T, n = c.pop('B'), c.pop('T'), c.pop('n')
    step = 50_000
    ts_end = T_BASE + step * np.arange(1, T + 1, dtype=np.int64)
    streams = []
    for b in range(B):
        if name == 'gaps':
            # window 0: ordinary; window 1: no event; window 2: one event; window 3: 40 events sharing one timestamp (den = 1)
            x, y, p, t = _uniform(rng, c, 800, step)
            xs, ys, ps, _ = _uniform(rng, c, 41, 1)
            x, y, p = np.concatenate([x, xs]), np.concatenate([y, ys]), np.concatenate([p, ps])
            t = np.concatenate([t, [T_BASE + 2 * step + 777], np.full(40, T_BASE + 3 * step + 5, dtype=np.int64)])
            x[800], y[800] = 5, 7                                         # the single event sits on an odd pixel
        else:
            x, y, p, t = _uniform(rng, c, n, step * T + (step if name != 'count_mode' else 0))   # some events behind the last window
        if name == 'count_mode':
            t = t + b * 20_000                                            # the two samples fill their first windows differently
        if name == 'edge_ties':
            # many events exactly at a window's end (side='right': inside) and exactly at end - delta (side='left': inside)
            for k, e in enumerate(ts_end):
                t[200 * k:200 * k + 60] = e
                t[200 * k + 60:200 * k + 120] = e - c['window_us']
            t = np.sort(t)
        if name.startswith('hot_wrap'):
            # window 0: 300 events on the odd pixel (5, 3) (uint8: 300 - 256 = 44; int16: cut at 255) and 400 on the even pixel
            # (4, 2), which must vanish; window 1: 33000 events on the odd pixel (9, 7) (uint8: 33000 % 256; int16: negative -> 0)
            hx = np.concatenate([np.full(300, 3), np.full(400, 2), np.full(33_000, 7)]).astype(np.int64)
            hy = np.concatenate([np.full(300, 5), np.full(400, 4), np.full(33_000, 9)]).astype(np.int64)
            hp = np.ones(hx.size, dtype=np.int64)
            ht = np.concatenate([np.full(700, T_BASE + 10), np.full(33_000, T_BASE + step + 10)]).astype(np.int64)
            order = np.argsort(np.concatenate([t, ht]), kind='stable')
            x, y, p, t = (np.concatenate([a, h])[order] for a, h in ((x, hx), (y, hy), (p, hp), (t, ht)))
        if name == 'neg_pol':
            p = rng.integers(-1, 2, t.size, dtype=np.int64)
        streams.append((x, y, p, t))
    if name == 'count_mode':
        ts_end = np.stack([ts_end, ts_end + 10_000])                      # a [B][T] window list
    return c, streams, ts_end


def builder_kwargs(c):
    return dict(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=c['cutoff'], fastmode=c['fastmode'], downsample_by_2=c['ds'],
                window_us=c.get('window_us'), window_events=c.get('window_events'))
