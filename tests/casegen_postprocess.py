"""Deterministic detection post-processing test cases: decoded prediction tensors [B][A][5 + nc] (cx cy w h obj cls...) from numpy
seeds, so that the golden fixtures (recorded from the reference's `postprocess` by tests/make_golden_postprocess.py) store outputs only.

Boxes are clustered around a few pseudo ground truths with jitter, so that many same-class pairs overlap and NMS has work.
The reference's NMS core is torchvision, which the recorder has to stand in for (plain greedy NMS on the raw fp32 boxes); real
torchvision may shift the boxes of each class apart first, which moves IoUs by a few ulp.  So that the recorded truth does not
depend on that choice - nor on how a sort orders equal scores - the generator NUDGES its data: for each image, among the candidates
at the lowest recorded confidence threshold, the objectness of the lower-scored member is set to 0 whenever
  * a pair's IoU (any two classes: this covers the class-agnostic run) lies within 1e-4 of a recorded nms threshold,
  * two scores are closer than 1e-7,
  * a score lies within 1e-5 of a recorded confidence threshold,
repeated until nothing changes.  Every condition the fixtures rely on is asserted here; none is silently relaxed."""
import functools
import zlib

import numpy as np

CASES = {
    'pp_small': dict(B=3, hws=((6, 10), (3, 5), (2, 3)), strides=(8, 16, 32), nc=3, n_gt=(2, 5)),               # A = 81
    'pp_gen1': dict(B=4, hws=((32, 40), (16, 20), (8, 10)), strides=(8, 16, 32), nc=2, n_gt=(8, 21)),           # A = 1680 (256x320)
    'pp_1mpx': dict(B=4, hws=((48, 80), (24, 40), (12, 20)), strides=(8, 16, 32), nc=3, n_gt=(14, 21)),          # A = 5040 (384x640)
}
# (conf_thre, nms_thre, class_agnostic): the shipped configuration, its agnostic form, nearly every anchor a candidate
SETTINGS = ((0.1, 0.45, False), (0.1, 0.45, True), (0.001, 0.65, False))
# per-image minimum of candidates at SETTINGS[0]
MIN_CANDIDATES = {'pp_small': 0, 'pp_gen1': 300, 'pp_1mpx': 1500}

IOU_MARGIN, SCORE_GAP, CONF_MARGIN, NUDGE_CAP = 1e-4, 1e-7, 1e-5, 0.05


def setting_id(s) -> str:
    return f'c{s[0]}_n{s[1]}_{"agn" if s[2] else "cls"}'


def _rng(name: str, what: str):
    return np.random.default_rng(zlib.crc32(f'{name}/{what}'.encode()))


def anchors(c):
    """Anchor centres and strides [A], level by level, row-major inside a level (the head's order)."""
    xs, ys, st = [], [], []
    for (H, W), s in zip(c['hws'], c['strides']):
        gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        xs.append((gx.ravel() + 0.5) * s)
        ys.append((gy.ravel() + 0.5) * s)
        st.append(np.full(H * W, float(s)))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(st)


def num_anchors(name: str) -> int:
    return sum(h * w for h, w in CASES[name]['hws'])


def _raw(name: str) -> np.ndarray:
    c = CASES[name]
    r = _rng(name, 'pred')
    B, nc = c['B'], c['nc']
    ax, ay, st = anchors(c)
    A = ax.size
    Hi, Wi = c['hws'][0][0] * c['strides'][0], c['hws'][0][1] * c['strides'][0]
    pred = np.zeros((B, A, 5 + nc), dtype=np.float64)
    for b in range(B):
        # background: a box near each anchor, low objectness
        pred[b, :, 0] = ax + r.normal(0, 1, A) * st
        pred[b, :, 1] = ay + r.normal(0, 1, A) * st
        pred[b, :, 2] = st * r.uniform(1, 6, A)
        pred[b, :, 3] = st * r.uniform(1, 6, A)
        pred[b, :, 4] = r.beta(1, 30, A)
        pred[b, :, 5:] = r.uniform(0, 1, (A, nc))
        for _ in range(int(r.integers(*c['n_gt']))):
            k = int(r.integers(0, nc))
            w, h = r.uniform(0.06, 0.3) * Wi, r.uniform(0.08, 0.36) * Hi
            cx, cy = r.uniform(0.05 * Wi, 0.95 * Wi), r.uniform(0.05 * Hi, 0.95 * Hi)
            inside = (np.abs(ax - cx) < w / 2) & (np.abs(ay - cy) < h / 2) & (r.random(A) < 0.85)
            n = int(inside.sum())
            pred[b, inside, 0] = cx + r.normal(0, 1, n) * st[inside]
            pred[b, inside, 1] = cy + r.normal(0, 1, n) * st[inside]
            pred[b, inside, 2] = w * r.uniform(0.8, 1.25, n)
            pred[b, inside, 3] = h * r.uniform(0.8, 1.25, n)
            pred[b, inside, 4] = r.uniform(0.3, 1, n)
            cls = r.uniform(0, 0.3, (n, nc))
            cls[:, k] = r.uniform(0.5, 1, n)
            pred[b, inside, 5:] = cls
    return pred.astype(np.float32)


def scores_of(img: np.ndarray) -> np.ndarray:
    """obj * max class score of one image [A][5+nc], one fp32 multiply."""
    return (img[:, 4] * img[:, 5:].max(axis=1)).astype(np.float32)


def corners(img: np.ndarray):
    x1 = img[:, 0] - img[:, 2] / np.float32(2)
    y1 = img[:, 1] - img[:, 3] / np.float32(2)
    x2 = img[:, 0] + img[:, 2] / np.float32(2)
    y2 = img[:, 1] + img[:, 3] / np.float32(2)
    return x1, y1, x2, y2


def _nudge_image(img: np.ndarray) -> int:
    """One nudge round on one image (in place); returns the number of anchors zeroed."""
    conf_lo = min(s[0] for s in SETTINGS)
    sc = scores_of(img)
    zero = np.zeros(img.shape[0], dtype=bool)
    for conf in sorted({s[0] for s in SETTINGS}):
        zero |= (np.abs(sc.astype(np.float64) - conf) < CONF_MARGIN) & (sc > 0)
    cand = np.nonzero((sc >= np.float32(conf_lo)) & ~zero)[0]
    cand = cand[np.argsort(-sc[cand], kind='stable')]                     # descending score: in a pair the LATER one is the lower
    s = sc[cand].astype(np.float64)
    close = np.nonzero(s[:-1] - s[1:] < SCORE_GAP)[0]
    zero[cand[close + 1]] = True
    x1, y1, x2, y2 = (v[cand] for v in corners(img))
    area = (x2 - x1) * (y2 - y1)
    n = cand.size
    thrs = sorted({s[1] for s in SETTINGS})
    for i0 in range(0, n, 512):
        i1 = min(n, i0 + 512)
        iw = np.maximum(np.float32(0), np.minimum(x2[i0:i1, None], x2[None, :]) - np.maximum(x1[i0:i1, None], x1[None, :]))
        ih = np.maximum(np.float32(0), np.minimum(y2[i0:i1, None], y2[None, :]) - np.maximum(y1[i0:i1, None], y1[None, :]))
        inter = iw * ih
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = (inter / (area[i0:i1, None] + area[None, :] - inter)).astype(np.float64)
        near = np.zeros(iou.shape, dtype=bool)
        for t in thrs:
            near |= np.abs(iou - t) < IOU_MARGIN
        rows, cols = np.nonzero(near)
        rows = rows + i0
        zero[cand[np.maximum(rows, cols)[rows != cols]]] = True
    img[zero, 4] = 0
    return int(zero.sum())


@functools.lru_cache(maxsize=None)
def _case(name: str):
    pred = _raw(name)
    c = CASES[name]
    A = pred.shape[1]
    zeroed = 0
    for b in range(c['B']):
        for _round in range(50):
            z = _nudge_image(pred[b])
            zeroed += z
            if z == 0:
                break
        else:
            raise AssertionError(f'{name}[{b}]: the nudge did not converge')
    assert zeroed <= NUDGE_CAP * c['B'] * A, f'{name}: nudged {zeroed} of {c["B"] * A} anchors (cap {NUDGE_CAP:.0%})'
    top2 = np.sort(pred[:, :, 5:], axis=2)[:, :, -2:] if c['nc'] > 1 else None
    if top2 is not None:
        assert (top2[:, :, 1] > top2[:, :, 0]).all(), f'{name}: an anchor has two equal top class scores'
    conf0, conf_lo = SETTINGS[0][0], min(s[0] for s in SETTINGS)
    n_lo = 0
    for b in range(c['B']):
        sc = scores_of(pred[b])
        assert int((sc >= np.float32(conf0)).sum()) >= MIN_CANDIDATES[name], f'{name}[{b}]: too few candidates at conf {conf0}'
        n_lo += int((sc >= np.float32(conf_lo)).sum())
    if name != 'pp_small':
        assert n_lo >= 0.85 * c['B'] * A, f'{name}: only {n_lo} of {c["B"] * A} anchors are candidates at conf {conf_lo}'
    pred.setflags(write=False)
    return pred, zeroed


def make_prediction(name: str) -> np.ndarray:
    """The nudged prediction tensor of a case, float32 [B][A][5+nc] (read-only: copy before handing it to anything that writes)."""
    return _case(name)[0]


def nudged(name: str) -> int:
    return _case(name)[1]


def candidate_counts(name: str, conf: float):
    pred = make_prediction(name)
    return [int((scores_of(pred[b]) >= np.float32(conf)).sum()) for b in range(pred.shape[0])]


def check_results(name: str, counts_by_setting) -> None:
    """Conditions on the recorded results (kept rows per image and setting, keyed like SETTINGS): NMS has real work."""
    aware, agn = counts_by_setting[SETTINGS[0]], counts_by_setting[SETTINGS[1]]
    cand = candidate_counts(name, SETTINGS[0][0])
    if name != 'pp_small':
        for b, (k, n) in enumerate(zip(aware, cand)):
            assert 2 * k <= n, f'{name}[{b}]: NMS keeps {k} of {n} candidates, more than half'
    assert all(g <= a for a, g in zip(aware, agn)) and any(g < a for a, g in zip(aware, agn)), \
        f'{name}: the class-agnostic run never keeps fewer rows than the class-aware one ({aware} vs {agn})'
