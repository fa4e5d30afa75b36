"""Golden fixtures of the spatial augmentation recorded from the UNMODIFIED reference RandomSpatialAugmentorGenX
(data/utils/augmentor.py, data/genx_utils/labels.py, imported from /root/reference), driven through its __call__ with the shipped
probabilities, one seeded sequence at a time.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_augment.py

The reference imports torchvision.transforms (InterpolationMode, functional.rotate), which is not installed, and the stub under
oracle/_stubs has no `transforms`: this recorder registers in-memory torchvision.transforms / .functional modules at run time;
`rotate` in them raises (rotate.prob is 0 in every shipped config).  The zoom-in window and factor are drawn while the state
is applied and are not kept in augm_state, so the recorder wraps the reference's _zoom_in_and_rescale_tensor with a spy that notes
its arguments and calls the original.
Stored per case in tests/golden/<case>.npz (numerical data only): states [B][5] (flip, mode, x0, y0, factor; float64), coded
[B][5][H][W] uint8 (the reference's output on casegen_augment.coded_planes: its source map), rows_out [T][B][G][7], count_out
[T][B] (-1 where the reference holds None, 0 where it keeps an empty label set), yolox [T][B][G][5] (get_labels_as_tensors)."""
import enum
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torchvision  # noqa: E402  (the stub)

from tests import casegen_augment as cg  # noqa: E402


def _register_transforms():
    tr = types.ModuleType('torchvision.transforms')
    fn = types.ModuleType('torchvision.transforms.functional')

    class InterpolationMode(enum.Enum):
        NEAREST = 'nearest'

    def rotate(*a, **k):
        raise NotImplementedError('torchvision stand-in: rotate is outside the recorded scope (rotate.prob = 0)')
    tr.InterpolationMode, fn.rotate, tr.functional = InterpolationMode, rotate, fn
    torchvision.transforms = tr
    sys.modules['torchvision.transforms'], sys.modules['torchvision.transforms.functional'] = tr, fn


def main():
    _register_transforms()
    from omegaconf import DictConfig
    from data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    from data.utils import augmentor as A
    from data.utils.types import DataType

    spy = {}
    orig = A.RandomSpatialAugmentorGenX._zoom_in_and_rescale_tensor

    def spying(input_, zoom_coordinates_x0y0, zoom_in_factor, datatype):
        spy['x0y0'], spy['factor'] = tuple(zoom_coordinates_x0y0), zoom_in_factor
        return orig(input_=input_, zoom_coordinates_x0y0=zoom_coordinates_x0y0, zoom_in_factor=zoom_in_factor, datatype=datatype)
    A.RandomSpatialAugmentorGenX._zoom_in_and_rescale_tensor = staticmethod(spying)

    per_case = {}
    for name, c in cg.CASES.items():
        hw = c['hw']
        labels = cg.make_labels(name)
        B, T = len(c['seeds']), cg.T_LABELS
        G = max(a.shape[0] for seq in labels for a in seq if a is not None)
        coded = torch.from_numpy(cg.coded_planes(hw))
        states = np.zeros((B, 5), dtype=np.float64)
        coded_out = np.zeros((B,) + tuple(coded.shape), dtype=np.uint8)
        rows_out = np.zeros((T, B, G, 7), dtype=np.float32)
        yolox = np.zeros((T, B, G, 5), dtype=np.float32)
        count_in = np.full((T, B), -1, dtype=np.int32)
        count_out = np.full((T, B), -1, dtype=np.int32)
        for b, seed in enumerate(c['seeds']):
            torch.manual_seed(seed)
            aug = A.RandomSpatialAugmentorGenX(dataset_hw=hw, automatic_randomization=True, augm_config=DictConfig(cg.AUGM_CONFIG))
            objs = [None if a is None else ObjectLabels(torch.from_numpy(a.copy()), input_size_hw=hw) for a in labels[b]]
            data = {DataType.EV_REPR: [coded.clone()], DataType.OBJLABELS_SEQ: SparselyBatchedObjectLabels(objs)}
            spy.clear()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                out = aug(data)
            st = aug.augm_state
            states[b] = (float(st.apply_h_flip), 0, 0, 0, 1.0)
            if st.apply_zoom_in and spy:
                states[b, 1:] = (1, spy['x0y0'][0], spy['x0y0'][1], spy['factor'])
            elif st.zoom_out.active and st.zoom_out.zoom_out_factor != 1:
                states[b, 1:] = (2, st.zoom_out.x0, st.zoom_out.y0, st.zoom_out.zoom_out_factor)
            coded_out[b] = out[DataType.EV_REPR][0].numpy()
            for t, lab in enumerate(out[DataType.OBJLABELS_SEQ]):
                count_in[t, b] = -1 if labels[b][t] is None else labels[b][t].shape[0]
                if lab is None:
                    continue
                k = len(lab)
                count_out[t, b] = k
                rows_out[t, b, :k] = lab.object_labels.numpy()
                yolox[t, b, :k] = lab.get_labels_as_tensors().numpy()
        per_case[name] = (states, count_in, np.where((count_out < 0) & (count_in > 0), 0, count_out))
        print(f'{name}: states (flip, mode) {[(int(s[0]), int(s[1])) for s in states]}')
        print(f'{name}: labels in {int(np.maximum(count_in, 0).sum())} out {int(np.maximum(count_out, 0).sum())}')
        path = os.path.join(ROOT, 'tests', 'golden', f'{name}.npz')
        np.savez_compressed(path, states=states, coded=coded_out, rows_out=rows_out, count_out=count_out, yolox=yolox)
        print(f'{name}: {os.path.getsize(path)} bytes')
    cg.check_results(per_case)


if __name__ == '__main__':
    main()
