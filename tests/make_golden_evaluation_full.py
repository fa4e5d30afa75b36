"""Golden fixtures of the recall table and the full COCO summary, recorded from the UNMODIFIED reference
`PropheseeEvaluator.evaluate_buffer` (utils/evaluation/prophesee/evaluator.py, imported from /root/reference) the way
tests/make_golden_evaluation.py records the precision table: its box filter, its time windowing and its COCO-dictionary conversion
run as shipped, and only the pycocotools core behind it is a stand-in - here tests/cocoeval_full_ref.COCOevalFull, the numpy
restatement with the published recall accumulation and the twelve-number summarize.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_evaluation_full.py

Cases: those of tests/casegen_evaluation.py plus the hand-made 'eval_ranks' (tests/casegen_evaluation_full.py), whose properties
are checked on the restatement before anything is recorded.  Stored per case in tests/golden/evalfull_<case>.npz: recall
[10][K][4][3] (COCOeval.eval['recall']), stats [12] (COCOeval.stats after summarize), the image count and npig [K][4].  Only
numerical outputs are stored."""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402

from tests import casegen_evaluation as cg  # noqa: E402
from tests import casegen_evaluation_full as cgf  # noqa: E402
from tests import cocoeval_full_ref as full  # noqa: E402


def main():
    case = cgf.ranks_case()
    c = cgf.RANKS
    cgf.ranks_properties(case, full.evaluate_frames(cg.to_frames(case), c['dataset'], c['ds2'], c['K']))
    full.install_standin()
    seen = []

    class Recording(full.COCOevalFull):                                   # keeps the evaluator object the reference builds and drops
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)
    sys.modules['pycocotools.cocoeval'].COCOeval = Recording
    with contextlib.redirect_stdout(io.StringIO()):
        from utils.evaluation.prophesee.evaluator import PropheseeEvaluator
    for name, c in cgf.CASES.items():
        labels, preds = cg.to_prophesee(cgf.make_case(name))
        ev = PropheseeEvaluator(dataset=c['dataset'], downsample_by_2=c['ds2'])
        ev.add_labels(labels)
        ev.add_predictions(preds)
        del seen[:]
        with contextlib.redirect_stdout(io.StringIO()):
            metrics = ev.evaluate_buffer(img_height=c['hw'][0], img_width=c['hw'][1])
        core = seen[-1]
        recall, stats = core.eval['recall'], np.asarray(core.stats, dtype=np.float64)
        assert recall.shape == (10, c['K'], 4, 3) and stats.shape == (12,)
        assert all(metrics[k] == stats[i] for i, k in enumerate(full.STAT_KEYS[:6]))
        out = {'recall': recall, 'stats': stats, 'images': np.array(len(core.params.imgIds), dtype=np.int64),
               'npig': core.npig.astype(np.int64)}
        print(f"{name}: images {int(out['images'])} of {c['F']} frames, "
              + ' '.join(f'{k} {v:.4f}' for k, v in zip(full.STAT_KEYS, stats)))
        np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', f'{cgf.golden_name(name)}.npz'), **out)


if __name__ == '__main__':
    main()
