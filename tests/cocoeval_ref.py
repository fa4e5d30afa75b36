"""Plain numpy restatement of the evaluation the reference's PropheseeEvaluator performs (TEST INFRASTRUCTURE).

Two layers:
  * `COCO` / `COCOeval`: the part of the pycocotools API that utils/evaluation/prophesee/metrics/coco_eval.py uses (bbox mode),
    restated from the published algorithm: loadRes (area = w * h of the given numbers), computeIoU (the bbIou formula in double,
    detections by descending score, mergesort, the first maxDets[-1]), evaluateImg (ground truth ordered non-ignored first, the
    greedy matching per threshold), accumulate (stable sort by score, cumulative tp / fp, precision made monotone from the right,
    sampled at the 101 recall levels with searchsorted) and summarize's first six numbers.  `install_standin()` puts them into
    sys.modules as pycocotools.coco / pycocotools.cocoeval, which is how tests/make_golden_evaluation.py runs the UNMODIFIED
    reference evaluator in a container without pycocotools.
  * `evaluate_frames`: the whole chain on per-frame arrays (Prophesee filter in fp32, image decision, zero-detection case,
    COCOeval), for cases that have no fixture.  tests/test_evaluation.py pins it to the fixtures recorded from the reference.
"""
import sys
import types
from collections import defaultdict

import numpy as np

OUT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')


class Params:
    def __init__(self):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1


class COCO:
    def __init__(self, annotation_file=None):
        assert annotation_file is None
        self.dataset, self.anns, self.imgs, self.cats = dict(), dict(), dict(), dict()

    def createIndex(self):
        self.anns = {a['id']: a for a in self.dataset.get('annotations', [])}
        self.imgs = {i['id']: i for i in self.dataset.get('images', [])}
        self.cats = {c['id']: c for c in self.dataset.get('categories', [])}

    def getCatIds(self):
        return [c['id'] for c in self.dataset['categories']]

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadRes(self, results):
        res = COCO()
        res.dataset['images'] = [img for img in self.dataset['images']]
        anns = results
        assert isinstance(anns, list)
        assert set(a['image_id'] for a in anns) <= set(self.getImgIds()), 'Results do not correspond to current coco set'
        res.dataset['categories'] = list(self.dataset['categories'])
        for i, ann in enumerate(anns):
            bb = ann['bbox']
            ann['area'] = bb[2] * bb[3]
            ann['id'] = i + 1
            ann['iscrowd'] = 0
        res.dataset['annotations'] = anns
        res.createIndex()
        return res


def bb_iou(d, g):
    """maskUtils.iou for boxes without crowd: d [D][4], g [G][4] (x y w h) -> double [D][G]."""
    d, g = np.asarray(d, dtype=np.float64).reshape(-1, 4), np.asarray(g, dtype=np.float64).reshape(-1, 4)
    da, ga = d[:, 2] * d[:, 3], g[:, 2] * g[:, 3]
    w = np.minimum(d[:, None, 2] + d[:, None, 0], g[None, :, 2] + g[None, :, 0]) - np.maximum(d[:, None, 0], g[None, :, 0])
    h = np.minimum(d[:, None, 3] + d[:, None, 1], g[None, :, 3] + g[None, :, 1]) - np.maximum(d[:, None, 1], g[None, :, 1])
    ok = (w > 0) & (h > 0)
    i = np.where(ok, w * h, 0.0)
    u = da[:, None] + ga[None, :] - i
    return np.where(ok, i / np.where(ok, u, 1.0), 0.0)


class COCOeval:
    def __init__(self, cocoGt=None, cocoDt=None, iouType='segm'):
        assert iouType == 'bbox'
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.getImgIds())
        self.params.catIds = sorted(cocoGt.getCatIds())
        self.evalImgs, self.eval, self.stats, self.ious = [], {}, [], {}
        self._gts, self._dts = defaultdict(list), defaultdict(list)

    def _prepare(self):
        p = self.params
        imgs, cats = set(p.imgIds), set(p.catIds)
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for gt in self.cocoGt.dataset['annotations']:
            if gt['image_id'] in imgs and gt['category_id'] in cats:
                gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
                self._gts[gt['image_id'], gt['category_id']].append(gt)
        for dt in self.cocoDt.dataset['annotations']:
            if dt['image_id'] in imgs and dt['category_id'] in cats:
                self._dts[dt['image_id'], dt['category_id']].append(dt)

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        self.ious = {(i, c): self.computeIoU(i, c) for i in p.imgIds for c in p.catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(i, c, a, maxDet) for c in p.catIds for a in p.areaRng for i in p.imgIds]

    def computeIoU(self, imgId, catId):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        if len(gt) == 0 or len(dt) == 0:
            return []
        return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt])

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g['_ignore'] = 1 if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]) else 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T, G, D = len(p.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    if not (ious[dind] >= iou).any():                     # shortcut only: no ground truth can pass the test below
                        continue
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'category_id': catId, 'aRng': aRng, 'maxDet': maxDet, 'dtMatches': dtm,
                'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def accumulate(self):
        p = self.params
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        self.npig = np.zeros((K, A), dtype=np.int64)
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
                    self.npig[k, a] = npig
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,)).tolist()
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds2 = np.searchsorted(rc, p.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds2):
                                q[ri] = pr[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
        self.eval = {'params': p, 'counts': [T, R, K, A, M], 'precision': precision}

    def summarize(self):
        p = self.params

        def _summarize(iouThr=None, areaRng='all', maxDets=100):
            aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
            mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
            s = self.eval['precision']
            if iouThr is not None:
                s = s[np.where(iouThr == p.iouThrs)[0]]
            s = s[:, :, :, aind, mind]
            return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        self.stats = np.array([_summarize(), _summarize(iouThr=.5), _summarize(iouThr=.75), _summarize(areaRng='small'),
                               _summarize(areaRng='medium'), _summarize(areaRng='large')])


def install_standin():
    """pycocotools.coco.COCO / pycocotools.cocoeval.COCOeval -> the classes above (only where pycocotools is missing)."""
    pkg, coco, cocoeval = types.ModuleType('pycocotools'), types.ModuleType('pycocotools.coco'), types.ModuleType('pycocotools.cocoeval')
    coco.COCO, cocoeval.COCOeval = COCO, COCOeval
    pkg.coco, pkg.cocoeval = coco, cocoeval
    sys.modules.update({'pycocotools': pkg, 'pycocotools.coco': coco, 'pycocotools.cocoeval': cocoeval})


def filter_constants(dataset, downsample_by_2):
    diag, side = (60, 20) if dataset == 'gen4' else (30, 10)
    return (diag // 2, side // 2) if downsample_by_2 else (diag, side)


def _keep(w, h, t, diag, side):
    w, h = np.asarray(w, dtype=np.float32), np.asarray(h, dtype=np.float32)
    return (t > 500000) * (w ** 2 + h ** 2 >= diag ** 2) * (w >= side) * (h >= side)


def evaluate_frames(frames, dataset, downsample_by_2, num_classes):
    """frames: list of (gt [n][5] fp32 x y w h class, dt [m][6] fp32 x y w h score class, t).  Returns metrics, precision
    [10][101][K][4], npig [K][4], images, and per image the COCOeval results in `per_image[(image index, category, area)]`."""
    diag, side = filter_constants(dataset, downsample_by_2)
    images, anns, results = [], [], []
    n_det = 0
    for gt, dt, t in frames:
        gt, dt = np.asarray(gt, dtype=np.float32).reshape(-1, 5), np.asarray(dt, dtype=np.float32).reshape(-1, 6)
        gt, dt = gt[_keep(gt[:, 2], gt[:, 3], t, diag, side)], dt[_keep(dt[:, 2], dt[:, 3], t, diag, side)]
        if gt.shape[0] == 0:
            continue
        im_id = len(images) + 1
        images.append({'id': im_id})
        n_det += dt.shape[0]
        for b in gt:
            anns.append({'area': float(b[2] * b[3]), 'iscrowd': False, 'image_id': im_id, 'bbox': [b[0], b[1], b[2], b[3]],
                         'category_id': int(b[4]) + 1, 'id': len(anns) + 1})
        for b in dt:
            results.append({'image_id': im_id, 'category_id': int(b[5]) + 1, 'score': float(b[4]), 'bbox': [b[0], b[1], b[2], b[3]]})
    out = {'images': len(images), 'metrics': {k: 0.0 for k in OUT_KEYS}, 'precision': None, 'npig': None, 'per_image': {}}
    gt_api = COCO()
    gt_api.dataset = {'images': images, 'annotations': anns, 'categories': [{'id': c + 1} for c in range(num_classes)]}
    gt_api.createIndex()
    ev = COCOeval(gt_api, gt_api.loadRes(results), 'bbox')
    ev.params.imgIds = np.arange(1, len(images) + 1, dtype=int)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    out['precision'], out['npig'] = ev.eval['precision'][..., -1], ev.npig
    if n_det > 0:
        out['metrics'] = {k: float(v) for k, v in zip(OUT_KEYS, ev.stats)}
    A, I0 = 4, len(images)
    for k in range(num_classes):
        for a in range(A):
            for i in range(I0):
                e = ev.evalImgs[k * A * I0 + a * I0 + i]
                if e is not None:
                    out['per_image'][i, k, a] = e
    return out
