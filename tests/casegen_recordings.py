"""Seeded inputs of the raw-recording fixtures (tests/golden/rec_*.npz): Prophesee DAT files as bytes and box-label arrays.

TEST INFRASTRUCTURE.  tests/make_golden_recordings.py runs the unmodified reference on exactly these inputs and stores inputs
and results; the tests read the stored files only.  The label inputs keep to what the reference itself asserts: accepted frames
more than 98 ms apart, 1 Mpx labels at 30 or 60 Hz."""
import numpy as np

# the reference's box record (utils/evaluation/prophesee/io/box_loading.py), as rvt_amd.evaluation.BBOX_DTYPE spells it
BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})

# ------------------------------------------------------------------------------------------------------------- DAT files
HEADER_V2 = (b'% Data file containing Event2D events.\n% Version 2\n% Date 2020-03-04 10:11:12\n% Height 240\n% Width 304\n')
HEADER_NO_SIZE = b'% Data file containing Event2D events.\n% Version 2\n'

DAT_CASES = {
    # name: header bytes (None = legacy file without any header), events, sensor (W, H), seed, what is special
    'v2_header': dict(header=HEADER_V2, n=3001, wh=(304, 240), seed=11, steps=True, high_bits=False, extremes=False),
    'no_size': dict(header=HEADER_NO_SIZE, n=2048, wh=(304, 240), seed=12, steps=False, high_bits=True, extremes=False),
    'legacy': dict(header=None, n=4099, wh=(1280, 720), seed=13, steps=True, high_bits=True, extremes=False),
    'extremes': dict(header=HEADER_V2, n=2500, wh=(16384, 16384), seed=14, steps=True, high_bits=True, extremes=True),
    # a clock that runs over some 300 ms: several 50 ms windows of a Gen1 recording hold events
    'windows': dict(header=HEADER_V2, n=3000, wh=(304, 240), seed=15, steps=True, high_bits=False, extremes=False, dt=200),
}


def make_dat(name):
    """-> (case, file bytes uint8).  Records are {uint32 t; int32 w}: x = bits 0-13, y = bits 14-27, p = bit 28, 29-31 unused."""
    c = DAT_CASES[name]
    rng = np.random.default_rng(c['seed'])
    n, (W, H) = c['n'], c['wh']
    x = rng.integers(0, W, n, dtype=np.int64)
    y = rng.integers(0, H, n, dtype=np.int64)
    p = rng.integers(0, 2, n, dtype=np.int64)
    t = 5000 + np.cumsum(rng.integers(0, c.get('dt', 40), n, dtype=np.int64))
    if c['steps']:                                       # the sensor's clock steps back: single events and whole stretches
        back = rng.choice(n - 1, size=n // 50, replace=False) + 1
        t[back] -= rng.integers(1, 3000, back.size)
        a = n // 3
        t[a:a + 300] -= 20000
        t = np.maximum(t, 0)
    if c['extremes']:
        x[:4], y[:4] = (0, 16383, 0, 16383), (0, 0, 16383, 16383)
        x[n // 2], y[n // 2] = 16383, 16383
        t[n - 700] = 2 ** 32 - 1                         # everything behind it is below it
        t[n - 1] = 2 ** 32 - 1
    w = x | (y << 14) | (p << 28)
    if c['high_bits']:                                   # bits 29-31 carry nothing and must not leak into p
        w |= rng.integers(0, 8, n, dtype=np.int64) << 29
    rec = np.zeros(n, dtype=[('t', '<u4'), ('w', '<u4')])
    rec['t'], rec['w'] = t.astype(np.uint32), (w & 0xffffffff).astype(np.uint32)
    body = rec.tobytes()
    if c['header'] is None:
        assert body[:2] != b'% '                         # a legacy file must not look like it opens with a comment line
        raw = body
    else:
        raw = c['header'] + bytes([0, 8]) + body
    return c, np.frombuffer(raw, dtype=np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------- labels
LABEL_CASES = {
    'gen1_train': dict(dataset='gen1', split='train', psee=False, faulty=True, align_t_ms=100, step_ms=50, seed=21),
    'gen1_val_jitter': dict(dataset='gen1', split='val', psee=True, faulty=True, align_t_ms=100, step_ms=100, seed=22),
    'gen4_60hz': dict(dataset='gen4', split='train', psee=False, faulty=True, align_t_ms=100, step_ms=50, seed=23),
    'gen4_30hz': dict(dataset='gen4', split='val', psee=True, faulty=False, align_t_ms=100, step_ms=25, seed=24),
    'single_frame': dict(dataset='gen1', split='train', psee=True, faulty=True, align_t_ms=100, step_ms=50, seed=25),
    'align_late': dict(dataset='gen1', split='test', psee=False, faulty=True, align_t_ms=600, step_ms=50, seed=26),
    'all_filtered': dict(dataset='gen4', split='train', psee=False, faulty=True, align_t_ms=100, step_ms=50, seed=27),
}
HW = {'gen1': (240, 304), 'gen4': (720, 1280)}


def _boxes(rng, ts, dataset, per_ts, classes):
    """Boxes at the given label times: fractional coordinates, some hanging out of the frame on every side, some too small for
    the filters, some as wide as the frame."""
    H, W = HW[dataset]
    rows = []
    for t in ts:
        k = int(rng.integers(per_ts[0], per_ts[1] + 1))
        lab = np.zeros(k, dtype=BBOX_DTYPE)
        lab['t'] = t
        lab['x'] = rng.uniform(-0.15 * W, 1.05 * W, k).astype(np.float32)
        lab['y'] = rng.uniform(-0.15 * H, 1.05 * H, k).astype(np.float32)
        lab['w'] = rng.uniform(2, 0.45 * W, k).astype(np.float32)
        lab['h'] = rng.uniform(2, 0.45 * H, k).astype(np.float32)
        small = rng.random(k) < 0.15
        lab['w'][small] = rng.uniform(1, 12, int(small.sum())).astype(np.float32)
        wide = rng.random(k) < 0.1
        lab['x'][wide] = rng.uniform(-5, 10, int(wide.sum())).astype(np.float32)
        lab['w'][wide] = rng.uniform(0.91 * W, 1.1 * W, int(wide.sum())).astype(np.float32)
        lab['class_id'] = rng.choice(classes, k)
        lab['track_id'] = rng.integers(0, 500, k)
        lab['class_confidence'] = rng.uniform(0.3, 1.0, k).astype(np.float32)
        rows.append(lab)
    # one box that is good under every filter at every label time: no frame loses all its labels
    for lab in rows:
        lab['x'][0], lab['y'][0], lab['w'][0], lab['h'][0] = 0.25 * W + 0.5, 0.25 * H + 0.25, 0.2 * W, 0.3 * H
        lab['class_id'][0] = classes[0]
    return np.concatenate(rows)


def make_labels(name):
    """-> (case, box records sorted by time)."""
    c = LABEL_CASES[name]
    rng = np.random.default_rng(c['seed'])
    ds = c['dataset']
    if name == 'gen1_train':                             # 4 Hz with up to 0.9 ms of jitter (1.8 ms between two frames), first label at 412 ms
        ts = 412_000 + 250_000 * np.arange(9) + rng.integers(-900, 901, 9)
        ts[5] = ts[4] + 500_000                          # one label period without a label: two base periods to the next frame
        ts[6:] = ts[5] + 250_000 * np.arange(1, 4)
        lab = _boxes(rng, ts, ds, (2, 5), [0, 1])
    elif name == 'gen1_val_jitter':                      # label times 5 ms and 120 ms off the grid are no frames
        grid = 300_000 + 250_000 * np.arange(7)
        ts = np.sort(np.concatenate([grid, [grid[2] + 120_000, grid[4] + 5_000]]))
        lab = _boxes(rng, ts, ds, (2, 4), [0, 1])
    elif name == 'gen4_60hz':                            # every sixth label time is a frame
        ts = 150_000 + np.rint(np.arange(40) * 1e6 / 60).astype(np.int64)
        lab = _boxes(rng, ts, ds, (2, 4), [0, 1, 2, 3, 4, 5, 6])
    elif name == 'gen4_30hz':                            # every third
        ts = 233_000 + np.rint(np.arange(22) * 1e6 / 30).astype(np.int64)
        lab = _boxes(rng, ts, ds, (2, 4), [0, 1, 2, 3, 4, 5, 6])
    elif name == 'single_frame':                         # the second label time is off the grid: one frame survives
        ts = np.array([523_456, 523_456 + 130_000])
        lab = _boxes(rng, ts, ds, (3, 3), [0, 1])
    elif name == 'align_late':                           # the labels at 100 ms and 350 ms lie in front of align_t_ms
        ts = 100_000 + 250_000 * np.arange(8)
        lab = _boxes(rng, ts, ds, (1, 3), [0, 1])
    elif name == 'all_filtered':                         # only classes the 1 Mpx filter removes
        ts = 150_000 + np.rint(np.arange(12) * 1e6 / 60).astype(np.int64)
        lab = _boxes(rng, ts, ds, (1, 2), [3, 4, 5, 6])
    else:
        raise KeyError(name)
    assert np.all(lab['t'][:-1] <= lab['t'][1:])
    return c, lab


def make_edge_labels():
    """-> (dataset, box records of two frames, first record of each frame) for the label factory alone: boxes 0.8 px wide at the
    right and bottom edge, which no filter would let through (they ask for 5 px and more), keep an area at full size and go flat at
    half scale: (x + w) / 2 is cut to W / 2 - 1, which lies left of x / 2.  Frame 1 holds nothing else, so it is empty at half scale."""
    H, W = HW['gen4']
    lab = np.zeros(4, dtype=BBOX_DTYPE)
    lab['t'] = (100_000, 100_000, 100_000, 200_000)
    lab['x'] = (100.5, W - 1.9, 640.25, W - 1.9)
    lab['y'] = (50.25, 300.0, H - 1.9, 10.5)
    lab['w'] = (200.0, 0.8, 30.0, 0.8)
    lab['h'] = (100.0, 40.0, 0.8, 33.0)
    lab['class_id'] = (0, 1, 2, 1)
    lab['track_id'] = (1, 2, 3, 2)
    lab['class_confidence'] = 1.0
    return 'gen4', lab, np.array([0, 3], dtype=np.int64)
