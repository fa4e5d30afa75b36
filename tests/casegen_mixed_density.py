"""Cases of the mixed-density event stack tests (shared by the golden recorder tests/make_golden_mixed_density.py and
tests/test_mixed_density.py).

SINGLE: one window each for ``MixedDensityEventStack.construct``; make_single(name) -> (params, x, y, p, t), int64 numpy arrays,
t non-decreasing.  SEQUENCE: the streams and window lists of the eleven tests/casegen_evseq.py cases run through the mixed
representation; only the cutoff is this file's (``fastmode`` does not exist there).  Every window of every case spans at most
MAX_SPAN_US, the range over which the reference's fp32 logarithm and the exact exponent rule agree (the recorder asserts it)."""
import numpy as np

from tests import casegen_evseq as cg

MAX_SPAN_US = 1 << 20
T_BASE = cg.T_BASE

SINGLE = {
    'plain': dict(H=24, W=32, bins=10, cutoff=None),
    # four positives in five: the running sums pass +5 on most pixels and stay above -5
    'cutoff5': dict(H=24, W=32, bins=10, cutoff=5),
    'cutoff0': dict(H=24, W=32, bins=10, cutoff=0),                       # everything clamps to zero
    'bins1': dict(H=24, W=32, bins=1, cutoff=None),
    # all events on one timestamp: den = 1, tn = 0 clamps to 1e-6, exponent -20 -> bin 5 of 25
    'one_timestamp': dict(H=24, W=32, bins=25, cutoff=None),
    'empty': dict(H=24, W=32, bins=10, cutoff=None),
    # span exactly 65536 us, one event at every 65536 >> k and 1 us either side of it, each on a pixel of its own
    'pow2_ties': dict(H=24, W=32, bins=20, cutoff=None),
    'hot_pos': dict(H=16, W=16, bins=4, cutoff=None),                     # 300 x p=1 in one cell: 300 - 256 = 44
    'hot_neg': dict(H=16, W=16, bins=4, cutoff=None),                     # 200 x p=0 in one cell: -200 + 256 = 56
    'prefix_wrap': dict(H=16, W=16, bins=10, cutoff=None),                # 100 positives in each of two bins of one pixel: 100, then -56
    # a plane of 15 x 21 = 315 pixels, off the 16-byte grid: the pixel-per-lane narrowing path at full size
    'odd_plane': dict(H=15, W=21, bins=3, cutoff=7),
}

# cutoff of the mixed representation per casegen_evseq case (32 is what the reference's mixeddensity_stack.yaml ships)
SEQUENCE = {
    'ds2_small': 32, 'odd_hw': 2, 'no_ds': None, 'overlap': 3, 'count_mode': 2, 'gaps': None, 'edge_ties': None, 'hot_wrap': None,
    'hot_wrap_int16': 20, 'neg_pol': 1, 'gen1_like': 3,             # hot_wrap_int16 shares hot_wrap's streams: here it adds the clamp
}


def _uniform(rng, c, n, span, p_one=0.5):
    x = rng.integers(0, c['W'], n, dtype=np.int64)
    y = rng.integers(0, c['H'], n, dtype=np.int64)
    p = (rng.random(n) < p_one).astype(np.int64)
    t = np.sort(rng.integers(0, span, n, dtype=np.int64)) + T_BASE
    return x, y, p, t


def _merge(a, b):
    """Two (x, y, p, t) tuples as one stream ordered by time (stable)."""
    order = np.argsort(np.concatenate([a[3], b[3]]), kind='stable')
    return tuple(np.concatenate([u, v])[order] for u, v in zip(a, b))


def make_single(name):
    c = dict(SINGLE[name])
    rng = np.random.default_rng(sum(map(ord, 'mdstack_' + name)))
    span = 50_000
    if name == 'empty':
        ev = tuple(np.zeros(0, dtype=np.int64) for _ in range(4))
    elif name == 'cutoff5':
        ev = _uniform(rng, c, 6000, span, p_one=0.8)
    elif name == 'one_timestamp':
        x, y, p, _ = _uniform(rng, c, 400, span)
        ev = (x, y, p, np.full(400, T_BASE + 123, dtype=np.int64))
    elif name == 'pow2_ties':
        offs = sorted({o for k in range(17) for o in ((65536 >> k) - 1, 65536 >> k, (65536 >> k) + 1) if 0 <= o <= 65536} | {0, 65536})
        n = len(offs)
        assert n <= c['H'] * c['W']
        i = np.arange(n, dtype=np.int64)
        ev = (i % c['W'], i // c['W'], np.ones(n, dtype=np.int64), T_BASE + np.asarray(offs, dtype=np.int64))
    elif name in ('hot_pos', 'hot_neg'):
        k, pol = (300, 1) if name == 'hot_pos' else (200, 0)
        bg = _uniform(rng, c, 500, span)
        bg[0][bg[0] == 3] = 4                                     # the hot pixel (5, 3) is the hot events' alone
        hot = (np.full(k, 3, dtype=np.int64), np.full(k, 5, dtype=np.int64), np.full(k, pol, dtype=np.int64),
               np.full(k, T_BASE + span, dtype=np.int64))         # the last timestamp: tn clamps to 1 - 1e-6, the last bin
        ev = _merge(bg, hot)
    elif name == 'prefix_wrap':
        bg = _uniform(rng, c, 500, span)
        bg[0][bg[0] == 3] = 4
        bg[3][0], bg[3][-1] = T_BASE, T_BASE + span               # t0 and t1 of the window
        tt = np.concatenate([np.full(100, T_BASE + int(0.3 * span)), np.full(100, T_BASE + int(0.75 * span))]).astype(np.int64)
        hot = (np.full(200, 3, dtype=np.int64), np.full(200, 5, dtype=np.int64), np.ones(200, dtype=np.int64), tt)
        ev = _merge(bg, hot)
    else:
        ev = _uniform(rng, c, 3000, span)
    return (c,) + tuple(ev)


def stack_kwargs(c):
    return dict(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=c['cutoff'])


def make_sequence(name):
    """(params, streams, ts_end) of casegen_evseq's case with the mixed representation's cutoff."""
    c, streams, ts_end = cg.make_case(name)
    c = dict(c, cutoff=SEQUENCE[name])
    c.pop('fastmode')
    return c, streams, ts_end


def sequence_kwargs(name):
    c = dict(cg.CASES[name])
    return dict(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=SEQUENCE[name], downsample_by_2=c['ds'],
                window_us=c.get('window_us'), window_events=c.get('window_events'), representation='mixed_density')
