"""Deterministic spatial-augmentation test cases from numpy seeds, so that the golden fixtures (recorded from the reference's
RandomSpatialAugmentorGenX by tests/make_golden_augment.py) store drawn states and outputs only.

Per case: B samples, each a sequence of T label frames generated inside the frame (some frames without labels) and a torch
seed for the reference's draw.  Planes come in two kinds:
  * coded planes (coded_planes): five uint8 planes holding x & 255, x >> 8, y & 255, y >> 8 and the constant 255.  The reference's
    output on them IS its source map (and the fifth plane its zero fill), and it compresses to almost nothing, so the fixtures
    cover full 1-Mpx frames;
  * event-like planes (event_planes): values 0..10, checked against a gather through the recorded maps.
The shipped probabilities (config/dataset/base.yaml) are used: prob_hflip 0.5, zoom.prob 0.8, zoom-in weight 8 factor 1..1.5,
zoom-out weight 2 factor 1..1.2.  The torch seeds were chosen so that all six combinations of flip and {none, zoom-in, zoom-out}
occur at every size; check_states / check_results assert that and the other conditions the fixtures rely on (a zoom-in that
drops a label, a frame that loses every label, a window clamped at the frame edge).  They are conditions on the inputs."""
import zlib

import numpy as np

AUGM_CONFIG = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)),
                             zoom_out=dict(weight=2, factor=dict(min=1, max=1.2))))

T_LABELS = 4
CASES = {
    'augment_gen1': dict(hw=(240, 304), seeds=(108, 103, 110, 112, 101, 100, 104, 102, 105, 107)),
    'augment_1mpx': dict(hw=(360, 640), seeds=(200, 205, 207, 208, 201, 220, 209, 202, 203, 212)),
    'augment_odd': dict(hw=(37, 53), seeds=(316, 302, 309, 301, 300, 331, 304, 306, 307, 305, 311, 308)),          # W % 16 != 0: the byte path
}


def _rng(name: str, what: str):
    return np.random.default_rng(zlib.crc32(f'{name}/{what}'.encode()))


def coded_planes(hw) -> np.ndarray:
    H, W = hw
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    return np.stack([x & 255, x >> 8, y & 255, y >> 8, np.full_like(x, 255)]).astype(np.uint8)


def event_planes(name: str, T: int, C: int) -> np.ndarray:
    """(T, B, C, H, W) uint8, values 0..10, mostly zero like a stacked histogram."""
    c = CASES[name]
    r = _rng(name, 'events')
    shape = (T, len(c['seeds']), C) + tuple(c['hw'])
    return (r.integers(0, 11, shape) * (r.random(shape) < 0.3)).astype(np.uint8)


def make_labels(name: str):
    """labels[b][t]: float32 [n][7] (t x y w h class_id class_confidence) or None; boxes inside the frame, x + w <= W - 1."""
    c = CASES[name]
    H, W = c['hw']
    r = _rng(name, 'labels')
    out = []
    for b in range(len(c['seeds'])):
        seq = []
        for t in range(T_LABELS):
            if r.random() < 0.3:
                seq.append(None)
                continue
            n = int(r.integers(1, 7))
            rows = np.zeros((n, 7), dtype=np.float32)
            for i in range(n):
                corner = r.random() < 0.25                                       # near the top-left corner: clamps the window
                x = r.uniform(0, 4) if corner else r.uniform(0, W - 4)
                y = r.uniform(0, 4) if corner else r.uniform(0, H - 4)
                w = r.uniform(1.5, max(2.0, min(W - 1 - x, W / 3)))
                h = r.uniform(1.5, max(2.0, min(H - 1 - y, H / 3)))
                w, h = min(w, W - 1 - x), min(h, H - 1 - y)
                rows[i] = (1000 * t + i, x, y, w, h, r.integers(0, 3), 1.0)
            rows[:, 3] = np.minimum(rows[:, 3], np.float32(W - 1) - rows[:, 1])   # x + w <= W - 1 holds in fp32 too
            rows[:, 4] = np.minimum(rows[:, 4], np.float32(H - 1) - rows[:, 2])
            assert (rows[:, 3] > 0).all() and (rows[:, 4] > 0).all()
            seq.append(rows)
        out.append(seq)
    return out


def states_array(states) -> np.ndarray:
    """[B][5] float64: flip, mode, x0, y0, factor."""
    return np.array([[float(s.flip), s.mode, s.x0, s.y0, s.factor] for s in states], dtype=np.float64).reshape(-1, 5)


def check_states(name: str, st: np.ndarray) -> None:
    combos = {(int(r[0]), int(r[1])) for r in st}
    assert combos == {(f, m) for f in (0, 1) for m in (0, 1, 2)}, f'{name}: flip x mode combinations {sorted(combos)}'


def clamped(st: np.ndarray) -> bool:
    return bool(((st[:, 1] == 1) & ((st[:, 2] == 0) | (st[:, 3] == 0))).any())


def check_results(per_case) -> None:
    """per_case: {name: (states [B][5], count_in [T][B], count_out [T][B])}."""
    dropped = lost_all = clamp = False
    for name, (st, cin, cout) in per_case.items():
        check_states(name, st)
        zi = st[:, 1] == 1
        dropped |= bool(((cout < cin) & zi[None, :] & (cin > 0)).any())
        lost_all |= bool(((cin > 0) & (cout == 0)).any())
        clamp |= clamped(st)
    assert dropped, 'no zoom-in drops a label'
    assert lost_all, 'no frame loses all its labels'
    assert clamp, 'no zoom-in window is clamped at the frame edge'
