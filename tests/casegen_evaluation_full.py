"""Inputs of the recall / full-summary tests (TEST INFRASTRUCTURE): the cases of tests/casegen_evaluation.py plus 'eval_ranks', a
hand-made case of seven frames that holds every way the rank logic behind the recall table can go wrong.  Same layouts as
casegen_evaluation (det [F][max_det][7] + count, label rows [F][G][7] + count, t_us)."""
import numpy as np

from tests import casegen_evaluation as cg

RANKS = dict(dataset='gen4', ds2=True, K=3, F=7, G=4, max_det=16, hw=(360, 640))
CASES = dict(cg.CASES, eval_ranks=RANKS)
TIE_SCORE = 0.96875                                  # the score two detections of different frames share (exact in fp32)


def golden_name(name):
    return 'evalfull_' + name[len('eval_'):]


def _miss(i):
    """The i-th false positive: 30 x 30 boxes in a corner no label reaches."""
    return (200 + 4 * i, 180, 30, 30)


def ranks_case():
    """What each frame is there for (labels x y w h class; detections x y w h class score):
      0  class 0: eleven misses above the one match, which ranks 12th (counted at maxDets 100 only); class 1: a miss at .9 above the
         match at .8 (counted from maxDets 10 on); class 1's records start at slot 12 of the row
      1  three classes in one row, the class-2 detections first in `det`; class 2 has no label in any frame; the class-0 match has
         the score TIE_SCORE
      2  no labels: not an image, its detections leave no record
      3  count > max_det: a full row, the frame counts as truncated; the class-0 match is the second of its class
      4  a class-0 miss with the score TIE_SCORE: behind frame 1's match by arrival; its match has IoU 31 / 40: thresholds up to .75 only
      5  labels under the size limits only: not an image
      6  t = 500000: filtered as a whole"""
    c = RANKS
    F, G, D = c['F'], c['G'], c['max_det']
    det, rows = np.zeros((F, D, 7), np.float32), np.zeros((F, G, 7), np.float32)
    count, lcount = np.zeros(F, np.int32), np.full(F, -1, np.int32)
    t_us = np.array([600000, 700000, 800000, 900000, 1000000, 1100000, 500000], dtype=np.int64)
    labels = {0: [(10, 10, 40, 40, 0), (100, 100, 50, 50, 1)],
              1: [(20, 20, 40, 40, 0), (120, 30, 30, 60, 1)],
              3: [(10, 10, 40, 40, 0), (100, 20, 30, 30, 0)],
              4: [(30, 30, 40, 40, 0)],
              5: [(10, 10, 5, 40, 0)],
              6: [(10, 10, 40, 40, 0)]}
    dets = {0: [_miss(i) + (0, 0.95 - 0.05 * i) for i in range(11)] + [(10, 10, 40, 40, 0, 0.3)]
               + [(150, 20, 50, 50, 1, 0.9), (100, 100, 50, 50, 1, 0.8)],
            1: [_miss(0) + (2, 0.5), _miss(3) + (2, 0.4), (120, 30, 30, 60, 1, 0.6), (20, 20, 40, 40, 0, TIE_SCORE)],
            2: [(10, 10, 40, 40, 0, 0.9), _miss(1) + (1, 0.8)],
            3: [_miss(i) + (i % 2, 0.9 - 0.03 * i) for i in range(12)] + [(10, 10, 40, 40, 0, 0.89), (100, 20, 30, 30, 0, 0.2),
                                                                          _miss(5) + (1, 0.1), _miss(6) + (0, 0.05)],
            4: [_miss(2) + (0, TIE_SCORE), (30, 30, 40, 31, 0, 0.5)],
            5: [(10, 10, 40, 40, 0, 0.9)],
            6: [(10, 10, 40, 40, 0, 0.9)]}
    for f, gts in labels.items():
        for g, (x, y, w, h, k) in enumerate(gts):
            rows[f, g] = (t_us[f], x, y, w, h, k, 1.0)
        lcount[f] = len(gts)
    for f, ds in dets.items():
        assert len(ds) <= D
        for j, (x, y, w, h, k, s) in enumerate(ds):
            det[f, j] = (x, y, x + w, y + h, 0.5, s, k)
        count[f] = len(ds)
    assert count[3] == D
    count[3] = D + 5                                                      # the rows beyond max_det do not exist
    return dict(det=det, count=count, rows=rows, lcount=lcount, t_us=t_us)


def make_case(name):
    return ranks_case() if name == 'eval_ranks' else cg.make_case(name)


def ranks_properties(case, want):
    """The properties 'eval_ranks' is there for, checked on the inputs and on the restatement's result `want`
    (cocoeval_full_ref.evaluate_frames); returns nothing, asserts."""
    from tests import cocoeval_ref as ref
    c = RANKS
    frames = cg.to_frames(case)
    diag, side = ref.filter_constants(c['dataset'], c['ds2'])
    per = want['per_image']
    images = [f for f, (gt, _, t) in enumerate(frames) if gt.shape[0] and ref._keep(gt[:, 2], gt[:, 3], t, diag, side).any()]
    assert len(images) == want['images'] and c['F'] <= 8 and c['G'] <= 16 and c['max_det'] <= 64
    tp = {key: (e['dtMatches'][0] != 0) & ~e['dtIgnore'][0].astype(bool) for key, e in per.items() if key[2] == 0}
    # a (frame, category) with more than 10 detections whose only match ranks 11th or later
    assert any(v.size > 10 and v.sum() == 1 and np.nonzero(v)[0][0] >= 10 for v in tp.values())
    # one whose best detection is a miss and whose second is the match
    assert any(v.size >= 2 and not v[0] and v[1] for v in tp.values())
    # several categories with records in one frame: category offsets inside a row are non-zero
    assert any(sum(1 for k in range(c['K']) if (i, k, 0) in per and len(per[i, k, 0]['dtScores'])) >= 3 for i in range(len(images)))
    # a truncated frame, a frame that is not an image although it holds detections, a category without ground truth
    assert (case['count'] > c['max_det']).any()
    assert any(f not in images and dt.shape[0] and t > 500000 and gt.shape[0] == 0 for f, (gt, dt, t) in enumerate(frames))
    assert (want['npig'][2] == 0).all() and (want['npig'][:2, 0] > 0).all()
    assert (want['recall'][:, 2] == -1).all() and (want['recall'][:, :2, 0] >= 0).all()
    assert any(key[1] == 2 and len(e['dtScores']) for key, e in per.items())          # ... which still has records
    # two exactly equal scores in different images of one category, a match and a miss
    tied = [(key[0], bool(tp[key][j])) for key, e in per.items() if key[2] == 0 and key[1] == 0
            for j, s in enumerate(e['dtScores']) if np.float32(s) == np.float32(TIE_SCORE)]
    assert len({i for i, _ in tied}) >= 2 and {hit for _, hit in tied} == {True, False}
    s = want['stats']
    assert s['AR_1'] < s['AR_10'] < s['AR_100'], s
