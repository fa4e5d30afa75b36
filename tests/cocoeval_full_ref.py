"""The rest of the published COCOeval on top of tests/cocoeval_ref.py (TEST INFRASTRUCTURE, plain numpy; never imported by rvt_amd).

`COCOevalFull` subclasses the restatement and adds what it leaves out: `accumulate` also fills
`eval['recall'][t, k, a, m] = tp_sum[-1] / npig` (0 where the cell has ground truth but no detection, -1 where it has no non-ignored
ground truth) and `summarize` produces all twelve numbers of `stats` in the published order.  The precision table is the parent's,
computed by the parent's code: `accumulate` calls it first and only adds the recall loop.

`evaluate_frames` is cocoeval_ref.evaluate_frames with this class behind it, plus `recall` [10][K][4][3] and `stats` (the twelve
numbers; all 0.0 when no detection survives in any image, the reference's rule for its six)."""
import numpy as np

from tests import cocoeval_ref as ref

STAT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L', 'AR_1', 'AR_10', 'AR_100', 'AR_S', 'AR_M', 'AR_L')


class COCOevalFull(ref.COCOeval):
    def accumulate(self):
        super().accumulate()
        p = self.params
        T, K, A, M = len(p.iouThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        recall = -np.ones((T, K, A, M))
        I0 = len(p.imgIds)
        for k in range(K):
            for a in range(A):
                for m, maxDet in enumerate(p.maxDets):
                    E = [self.evalImgs[k * A * I0 + a * I0 + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    for t, tp in enumerate(tp_sum):
                        nd = len(tp)
                        rc = tp / npig
                        recall[t, k, a, m] = rc[-1] if nd else 0
        self.eval['recall'] = recall

    def summarize(self):
        p = self.params

        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
            mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    s = s[np.where(iouThr == p.iouThrs)[0]]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    s = s[np.where(iouThr == p.iouThrs)[0]]
                s = s[:, :, aind, mind]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        self.stats = np.array([_summarize(1), _summarize(1, iouThr=.5, maxDets=p.maxDets[2]), _summarize(1, iouThr=.75, maxDets=p.maxDets[2]),
                               _summarize(1, areaRng='small', maxDets=p.maxDets[2]), _summarize(1, areaRng='medium', maxDets=p.maxDets[2]),
                               _summarize(1, areaRng='large', maxDets=p.maxDets[2]),
                               _summarize(0, maxDets=p.maxDets[0]), _summarize(0, maxDets=p.maxDets[1]), _summarize(0, maxDets=p.maxDets[2]),
                               _summarize(0, areaRng='small', maxDets=p.maxDets[2]), _summarize(0, areaRng='medium', maxDets=p.maxDets[2]),
                               _summarize(0, areaRng='large', maxDets=p.maxDets[2])], dtype=np.float64)


def evaluate_frames(frames, dataset, downsample_by_2, num_classes):
    """cocoeval_ref.evaluate_frames (its filter, its image decision, its zero-detection rule) with COCOevalFull as the core; the
    result also holds `recall` [10][K][4][3] and `stats` {STAT_KEYS: float}."""
    seen = []

    class Recording(COCOevalFull):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)
    parent = ref.COCOeval
    ref.COCOeval = Recording
    try:
        out = ref.evaluate_frames(frames, dataset, downsample_by_2, num_classes)
    finally:
        ref.COCOeval = parent
    core = seen[-1]
    diag, side = ref.filter_constants(dataset, downsample_by_2)
    n_det = 0
    for gt, dt, t in frames:
        gt, dt = np.asarray(gt, dtype=np.float32).reshape(-1, 5), np.asarray(dt, dtype=np.float32).reshape(-1, 6)
        if ref._keep(gt[:, 2], gt[:, 3], t, diag, side).any():
            n_det += int(ref._keep(dt[:, 2], dt[:, 3], t, diag, side).sum())
    out['recall'] = core.eval['recall']
    out['stats'] = {k: (float(v) if n_det > 0 else 0.0) for k, v in zip(STAT_KEYS, core.stats)}
    assert all(out['stats'][k] == out['metrics'][k] for k in ref.OUT_KEYS)
    return out


def install_standin():
    """cocoeval_ref.install_standin with COCOevalFull as pycocotools.cocoeval.COCOeval."""
    import sys
    ref.install_standin()
    sys.modules['pycocotools.cocoeval'].COCOeval = COCOevalFull
