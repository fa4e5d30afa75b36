"""Golden fixture of tests/test_host.py::test_dropin_through_reference_registry_and_detector, recorded from the UNMODIFIED
reference's own YoloXDetector (its torch implementation).

TEST INFRASTRUCTURE; needs a checkout of the reference.  Usage: python oracle/make_golden_dropin.py <reference checkout>
The detector of tests/casegen_dropin.model_cfg with the seeded weights of casegen_dropin.seeded_state: backbone features of a
3-step sequence with carried ConvLSTM states, the final states, eval-mode detections, then (training mode, on the last step's
features) the losses and the gradient of `loss` with respect to the backbone features.  Stored: the state_dict names and shapes, its
integer buffers and those outputs (tests/golden/dropin_detector.npz)."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(HERE, '_stubs'))
sys.path.insert(1, os.path.abspath(sys.argv[1]))
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from omegaconf import OmegaConf  # noqa: E402
from models.detection.yolox_extension.models.detector import YoloXDetector  # noqa: E402

from tests import casegen_dropin as cg  # noqa: E402


def main():
    torch.set_num_threads(4)
    ref = YoloXDetector(OmegaConf.create(cg.model_cfg())).eval()
    sd = ref.state_dict()
    ints = {n: t for n, t in sd.items() if not t.is_floating_point()}
    ref.load_state_dict(cg.seeded_state(sd, ints), strict=True)
    out = {'names': np.array(list(sd)), 'shapes': np.array([','.join(map(str, t.shape)) for t in sd.values()])}
    out.update({'int:' + n: t.numpy() for n, t in ints.items()})
    xs = cg.make_inputs()
    st = None
    with torch.no_grad():
        for t in range(xs.shape[0]):
            feats, st = ref.forward_backbone(F.pad(xs[t].float(), [0, 6, 0, 4]), st)      # modules/detection.py:133-134
            out.update({f'feat_t{t}_s{s}': v.numpy() for s, v in feats.items()})
        for i, (h, c) in enumerate(st):
            out[f'h{i}'], out[f'c{i}'] = h.numpy(), c.numpy()
        out['detections'] = ref.forward_detect(backbone_features=feats)[0].numpy()
    ref.train()
    fg = {s: v.detach().clone().requires_grad_(True) for s, v in feats.items()}
    _, losses = ref.forward_detect(backbone_features=fg, targets=cg.make_targets())
    out.update({'loss:' + k: np.float64(float(v.detach())) for k, v in losses.items()})
    losses['loss'].backward()
    out.update({f'feat_grad_s{s}': fg[s].grad.numpy() for s in (2, 3, 4)})
    path = os.path.join(ROOT, 'tests', 'golden', cg.GOLDEN + '.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {len(out)} arrays, losses {dict((k, round(float(v.detach()), 4)) for k, v in losses.items())}')


if __name__ == '__main__':
    main()
