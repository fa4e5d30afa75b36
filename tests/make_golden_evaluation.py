"""Golden fixtures of the detection evaluation recorded from the UNMODIFIED reference `PropheseeEvaluator.evaluate_buffer`
(utils/evaluation/prophesee/evaluator.py, imported from /root/reference): its box filter, its time windowing and its
COCO-dictionary conversion run as shipped.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_evaluation.py

The reference's matching / accumulation core is pycocotools, which is not installed.  This recorder installs a stand-in
pycocotools.coco.COCO / pycocotools.cocoeval.COCOeval into sys.modules at run time, backed by tests/cocoeval_ref.py (a plain
numpy restatement of the published COCOeval algorithm), the way tests/make_golden_postprocess.py stands in for torchvision's NMS.
Stored per case in tests/golden/<case>.npz: the six metrics, the precision table [10][101][K][4] at maxDets = 100, the image
count and npig [K][4].  Only numerical outputs are stored."""
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
from tests import cocoeval_ref  # noqa: E402

OUT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')


def main():
    cocoeval_ref.install_standin()
    seen = []

    class Recording(cocoeval_ref.COCOeval):                               # keeps the evaluator object the reference builds and drops
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self)
    sys.modules['pycocotools.cocoeval'].COCOeval = Recording
    with contextlib.redirect_stdout(io.StringIO()):
        from utils.evaluation.prophesee.evaluator import PropheseeEvaluator
    for name, c in cg.CASES.items():
        labels, preds = cg.to_prophesee(cg.make_case(name))
        ev = PropheseeEvaluator(dataset=c['dataset'], downsample_by_2=c['ds2'])
        ev.add_labels(labels)
        ev.add_predictions(preds)
        del seen[:]
        with contextlib.redirect_stdout(io.StringIO()):
            metrics = ev.evaluate_buffer(img_height=c['hw'][0], img_width=c['hw'][1])
        core = seen[-1]
        precision = core.eval['precision'][..., -1]
        assert precision.shape == (10, 101, c['K'], 4)
        out = {'metrics': np.array([metrics[k] for k in OUT_KEYS], dtype=np.float64), 'precision': precision,
               'images': np.array(len(core.params.imgIds), dtype=np.int64), 'npig': core.npig.astype(np.int64)}
        print(f"{name}: images {int(out['images'])} of {c['F']} frames, npig {out['npig'].tolist()}, "
              + ' '.join(f'{k} {metrics[k]:.4f}' for k in OUT_KEYS))
        np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', f'{name}.npz'), **out)


if __name__ == '__main__':
    main()
