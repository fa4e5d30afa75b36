"""Seeded inputs of the evaluation tests (TEST INFRASTRUCTURE): frames of ground-truth boxes and detections in the layouts the
evaluator takes - det [F][max_det][7] + count [F] as postprocess_padded returns them, label rows [F][G][7] + count [F] as
augment.pack_labels lays them out, t_us [F] - and their conversions to the restatement's per-frame arrays and to the
reference's BBOX_DTYPE structured arrays (built the way io/box_loading.py to_prophesee builds them: w = x2 - x1 in fp32)."""
import numpy as np

BBOX_DTYPE = np.dtype({'names': ['t', 'x', 'y', 'w', 'h', 'class_id', 'track_id', 'class_confidence'],
                       'formats': ['<i8', '<f4', '<f4', '<f4', '<f4', '<u4', '<u4', '<f4'],
                       'offsets': [0, 8, 12, 16, 20, 24, 28, 32], 'itemsize': 40})

# a few hundred frames each: the CPU emulator runs a workgroup as fibers on one thread
CASES = {
    'eval_gen1': dict(dataset='gen1', ds2=False, K=2, F=320, G=8, max_det=48, hw=(240, 304), seed=11),
    'eval_1mpx': dict(dataset='gen4', ds2=False, K=3, F=256, G=16, max_det=64, hw=(720, 1280), seed=12),
    'eval_1mpx_ds2': dict(dataset='gen4', ds2=True, K=3, F=256, G=16, max_det=64, hw=(360, 640), seed=13),
    'eval_edges': dict(dataset='gen4', ds2=True, K=3, F=200, G=12, max_det=320, hw=(360, 640), seed=14, edges=True),
}


def _boxes(r, n, hw, lo, hi):
    """n boxes x y w h with sides log-uniform in [lo, hi], inside the frame where they fit."""
    H, W = hw
    w = np.exp(r.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)
    h = (w * r.uniform(0.5, 2.0, n)).astype(np.float32)
    x = r.uniform(0, np.maximum(W - w, 1)).astype(np.float32)
    y = r.uniform(0, np.maximum(H - h, 1)).astype(np.float32)
    return np.stack([x, y, w, h], axis=1)


def random_case(seed, dataset, ds2, K, F, G, max_det, hw=(360, 640), edges=False, det_rate=1.0, overflow=False):
    """-> dict(det, count, rows, lcount, t_us) of numpy arrays.  Scores are drawn from a coarse grid, so exact ties occur within
    and across frames; some detections are duplicated; box sides straddle the filter limits and the 32^2 / 96^2 area limits.
    edges: also frames at t <= 500000, frames whose every label is under the size limits while they hold detections, more than 100
    detections of class 0 in a frame, class 1 without detections and class 2 without ground truth.
    overflow: count exceeds max_det in some frames (the rows beyond max_det do not exist)."""
    r = np.random.default_rng(seed)
    side = (20 if dataset == 'gen4' else 10) // (2 if ds2 else 1)
    det = np.zeros((F, max_det, 7), dtype=np.float32)
    count = np.zeros(F, dtype=np.int32)
    rows = np.zeros((F, G, 7), dtype=np.float32)
    lcount = np.full(F, -1, dtype=np.int32)
    t_us = (r.integers(600000, 60000000, F) // 1000 * 1000).astype(np.int64)
    for f in range(F):
        kind = r.integers(0, 10) if edges else 9
        if kind == 0:
            t_us[f] = [500000, 499999, 1000, 500000][r.integers(0, 4)]
        n_gt = int(r.integers(0, min(G, 7) + 1)) if G > 1 else int(r.integers(0, 2))
        if G > 1 and r.integers(0, 8) == 0:
            n_gt = G
        gt = _boxes(r, n_gt, hw, side * 0.6, 160.0)
        if kind == 1:                                                     # every label under the size limits
            gt = _boxes(r, max(n_gt, 1), hw, 2.0, side * 0.45)
            gt[:, 3] = np.minimum(gt[:, 3], np.float32(side * 0.9))
            n_gt = gt.shape[0]
        gcls = r.integers(0, K, n_gt)
        if edges:
            gcls = r.integers(0, 2, n_gt)                                 # class 2 has no ground truth
        if n_gt:
            rows[f, :n_gt, 0] = t_us[f]
            rows[f, :n_gt, 1:5] = gt
            rows[f, :n_gt, 5] = gcls
            rows[f, :n_gt, 6] = 1.0
            lcount[f] = n_gt
        elif r.integers(0, 2):
            lcount[f] = 0
        # detections: jittered copies of the labels, loose copies, false positives, duplicates
        d_boxes, d_cls = [], []
        for g in range(n_gt):
            for _ in range(int(r.integers(0, 3))):
                j = gt[g] * (1 + r.normal(0, 0.06, 4)).astype(np.float32)
                j[:2] = gt[g, :2] + r.normal(0, 0.05, 2).astype(np.float32) * gt[g, 2:]
                d_boxes.append(j if r.integers(0, 6) else gt[g].copy())    # sometimes the exact box: IoU 1
                d_cls.append(gcls[g] if r.integers(0, 8) else r.integers(0, K))
        n_fp = int(r.integers(0, 6))
        for b in _boxes(r, n_fp, hw, side * 0.5, 200.0):
            d_boxes.append(b)
            d_cls.append(r.integers(0, K))
        if kind == 2:                                                     # > 100 detections of class 0
            gsrc = gt if n_gt else _boxes(r, 1, hw, 30.0, 60.0)
            for i in range(int(r.integers(110, 150))):
                b = gsrc[i % gsrc.shape[0]] * (1 + r.normal(0, 0.15, 4)).astype(np.float32)
                d_boxes.append(b)
                d_cls.append(0)
        if d_boxes and r.integers(0, 3) == 0:
            for _ in range(int(r.integers(1, 4))):                        # duplicated detections
                i = int(r.integers(0, len(d_boxes)))
                d_boxes.append(d_boxes[i].copy())
                d_cls.append(d_cls[i])
        if r.uniform() > det_rate:
            d_boxes, d_cls = [], []
        n = len(d_boxes)
        if n:
            b = np.abs(np.stack(d_boxes)).astype(np.float32)
            c = np.asarray(d_cls)
            if edges:
                c = np.where(c == 1, 0, c)                                # class 1 has no detections
            conf = (r.integers(1, 65, n) / 64.0).astype(np.float32)       # coarse grid: exact ties
            fine = r.integers(0, 3, n) == 0
            conf[fine] = r.uniform(0.01, 1.0, int(fine.sum())).astype(np.float32)
            obj = r.uniform(0.3, 1.0, n).astype(np.float32)
            order = np.argsort(-(obj * conf), kind='stable')              # postprocess orders by obj * class_conf
            b, c, conf, obj = b[order], c[order], conf[order], obj[order]
            m = min(n, max_det)
            det[f, :m, 0:2] = b[:m, 0:2]
            det[f, :m, 2:4] = b[:m, 0:2] + b[:m, 2:4]
            det[f, :m, 4], det[f, :m, 5], det[f, :m, 6] = obj[:m], conf[:m], c[:m]
            count[f] = n if overflow else m
    return dict(det=det, count=count, rows=rows, lcount=lcount, t_us=t_us)


def make_case(name):
    c = CASES[name]
    return random_case(c['seed'], c['dataset'], c['ds2'], c['K'], c['F'], c['G'], c['max_det'], c['hw'], c.get('edges', False))


def to_frames(case):
    """-> [(gt [n][5] x y w h class, dt [m][6] x y w h score class, t)] per frame, w = x2 - x1 in fp32 as to_prophesee does."""
    out = []
    max_det = case['det'].shape[1]
    for f in range(case['det'].shape[0]):
        n, m = max(int(case['lcount'][f]), 0), min(max(int(case['count'][f]), 0), max_det)
        gt = case['rows'][f, :n][:, [1, 2, 3, 4, 5]]
        d = case['det'][f, :m]
        dt = np.stack([d[:, 0], d[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1], d[:, 5], d[:, 6]], axis=1).astype(np.float32)
        out.append((gt, dt, int(case['t_us'][f])))
    return out


def to_prophesee(case):
    """-> (labels, predictions): one BBOX_DTYPE array per frame each, the reference evaluator's input."""
    labels, preds = [], []
    for gt, dt, t in to_frames(case):
        lab = np.zeros((gt.shape[0],), dtype=BBOX_DTYPE)
        lab['t'] = t
        for i, name in enumerate(('x', 'y', 'w', 'h')):
            lab[name] = gt[:, i]
        lab['class_id'] = gt[:, 4].astype(np.uint32)
        lab['class_confidence'] = 1.0
        p = np.zeros((dt.shape[0],), dtype=BBOX_DTYPE)
        p['t'] = t
        for i, name in enumerate(('x', 'y', 'w', 'h')):
            p[name] = dt[:, i]
        p['class_confidence'] = dt[:, 4]
        p['class_id'] = dt[:, 5].astype(np.uint32)
        labels.append(lab)
        preds.append(p)
    return labels, preds
