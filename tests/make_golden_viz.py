"""Records tests/golden/viz_evimg.npz: inputs and outputs of the reference's own `VizCallbackBase.ev_repr_to_img`
(callbacks/viz_base.py:164-174), unmodified, for three event tensors.  Data only: the arrays the function read and returned.

    python tests/make_golden_viz.py /path/to/reference

The reference module imports packages this stack does not carry (pytorch_lightning, wandb, ...); empty stand-in modules take
their place in sys.modules for the import.  The function itself needs numpy and einops only, which are real."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'golden', 'viz_evimg.npz')


class _Anything(types.ModuleType):
    """A module whose every attribute is a class that accepts any subscript, call and subclassing."""

    __version__ = '1.8.6'

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        cls = type(name, (), {'__class_getitem__': classmethod(lambda c, k: c), '__init__': lambda self, *a, **k: None})
        setattr(self, name, cls)
        return cls


def load_reference(root: str):
    sys.path.insert(0, root)
    for _ in range(64):                              # one stand-in per missing import, until the module loads
        try:
            return importlib.import_module('callbacks.viz_base').VizCallbackBase
        except ImportError as e:
            missing = e.name
            if not missing or missing.startswith('callbacks'):
                raise
            parts = missing.split('.')
            for k in range(1, len(parts) + 1):
                name = '.'.join(parts[:k])
                if name not in sys.modules:
                    mod = _Anything(name)
                    mod.__path__ = []
                    sys.modules[name] = mod
            for mod_name in [n for n in sys.modules if n.startswith('callbacks')]:
                del sys.modules[mod_name]
    raise RuntimeError('callbacks.viz_base did not load')


def tensors():
    rng = np.random.default_rng(20240611)
    a = (rng.integers(0, 4, size=(20, 12, 16)) * (rng.random((20, 12, 16)) < 0.2)).astype(np.uint8)
    a[:, 0, 0] = 0
    a[:10, 0, 1] = 25
    a[10:, 0, 1] = 25                                # sums that cancel
    a[:, 0, 2] = 255                                 # 2550 on either side
    b = rng.integers(0, 3, size=(2, 3, 5)).astype(np.uint8)
    c = (rng.integers(-3, 4, size=(10, 7, 33)) * (rng.random((10, 7, 33)) < 0.3)).astype(np.int8)
    c[:, 0, 0] = -128
    c[:5, 0, 1] = -128
    c[5:, 0, 1] = 127
    c[:5, 0, 2] = 127
    c[5:, 0, 2] = -128
    return {'u8_c20': a, 'u8_c2': b, 'i8_c10': c}


def main():
    ref = load_reference(sys.argv[1])
    rec = {}
    for name, x in tensors().items():
        img = ref.ev_repr_to_img(x.copy())
        assert img.dtype == np.uint8 and img.shape == x.shape[1:] + (3,)
        rec['in_' + name], rec['out_' + name] = x, img
    np.savez_compressed(OUT, **rec)
    print('wrote', OUT, {k: v.shape for k, v in rec.items()})


if __name__ == '__main__':
    main()
