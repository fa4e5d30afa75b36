"""Golden fixtures of the mixed-density event stack, recorded on the CPU from the UNMODIFIED reference MixedDensityEventStack
(data/utils/representations.py:130-218, imported from /root/reference).

Single windows (tests/golden/mdstack_<case>.npz): one ``construct`` call.
Sequences (tests/golden/evseq_md_<case>.npz): composed exactly as the reference's preprocessing does.  preprocess_dataset.py itself
needs h5py and numba, so its steps are restated by hand, as in tests/make_golden_evseq.py: numpy searchsorted side='right' /
'left' (or max(end - N, 0)) over the stream's timestamps (scripts/genx/preprocess_dataset.py:511-516), the reader's clip of the
polarity to >= 0 (:181), one construct per window (:518-523) and, when down-sampling, ``downsample_ev_repr`` (:467-477): int8 ->
int16 + 128 -> uint8 -> interpolate(scale_factor=0.5, mode='nearest-exact') -> int16 - 128 -> int8.

Every window must span at most 2^20 us: that is the range over which the reference's fp32 ``log`` quotient equals the exact
``bins + floor(log2(tn))`` the device computes (rvt_amd/representations.py); the recorder asserts it.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_mixed_density.py

Stored (numerical data only): mdstack_<case>.npz: x, y, p (int16), t (int64), out int8 (bins, H, W).  evseq_md_<case>.npz:
ts_end, bounds int64 [B][T][2], planes int8 (T, B, bins, H', W'); the streams are those of tests/golden/evseq_<case>.npz (the
recorder checks that the generator still produces exactly them), so they are not stored twice."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import casegen_mixed_density as cm  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')


def downsample_ev_repr(x: torch.Tensor, scale_factor: float) -> torch.Tensor:
    """preprocess_dataset.py:467-477 for int8 input, step by step."""
    assert x.dtype == torch.int8
    x = torch.asarray(x, dtype=torch.int16)
    x = torch.asarray(x + 128, dtype=torch.uint8)
    x = torch.nn.functional.interpolate(x, scale_factor=scale_factor, mode='nearest-exact')
    x = torch.asarray(x, dtype=torch.int16)
    return torch.asarray(x - 128, dtype=torch.int8)


def span_ok(t):
    return t.size == 0 or int(t[-1] - t[0]) <= cm.MAX_SPAN_US


def main():
    from data.utils.representations import MixedDensityEventStack

    for name in cm.SINGLE:
        c, x, y, p, t = cm.make_single(name)
        assert np.all(t[:-1] <= t[1:]) and span_ok(t), name
        rep = MixedDensityEventStack(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=c['cutoff'])
        out = rep.construct(x=torch.from_numpy(x), y=torch.from_numpy(y), pol=torch.from_numpy(p), time=torch.from_numpy(t)).numpy()
        assert out.dtype == np.int8 and out.shape == (c['bins'], c['H'], c['W'])
        path = os.path.join(GOLD, f'mdstack_{name}.npz')
        np.savez_compressed(path, x=x.astype(np.int16), y=y.astype(np.int16), p=p.astype(np.int16), t=t, out=out)
        print(f'{name}: {t.size} events, out min {int(out.min())} max {int(out.max())} nonzero {int((out != 0).sum())}, '
              f'{os.path.getsize(path)} bytes')

    for name in cm.SEQUENCE:
        c, streams, ts_end = cm.make_sequence(name)
        have = np.load(os.path.join(GOLD, f'evseq_{name}.npz'))
        rep = MixedDensityEventStack(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=c['cutoff'])
        B, T = len(streams), ts_end.shape[-1]
        Ho, Wo = (c['H'] // 2, c['W'] // 2) if c['ds'] else (c['H'], c['W'])
        planes = np.zeros((T, B, c['bins'], Ho, Wo), dtype=np.int8)
        bounds = np.zeros((B, T, 2), dtype=np.int64)
        assert np.array_equal(have['ts_end'], ts_end)
        for b, (x, y, p, t) in enumerate(streams):
            assert np.all(t[:-1] <= t[1:])
            for k, a in (('x', x), ('y', y), ('p', p), ('t', t)):
                assert np.array_equal(have[f'{k}{b}'], a), (name, k, b)       # the stored streams are the generator's
            te = ts_end if ts_end.ndim == 1 else ts_end[b]
            end = np.searchsorted(t, te, side='right')
            if c.get('window_events') is not None:
                start = np.maximum(end - c['window_events'], 0)
            else:
                start = np.searchsorted(t, te - c['window_us'], side='left')
            for w, (i0, i1) in enumerate(zip(start, end)):
                assert span_ok(t[i0:i1]), (name, b, w)
                pw = np.clip(p[i0:i1], a_min=0, a_max=None)
                ev = rep.construct(x=torch.from_numpy(x[i0:i1]), y=torch.from_numpy(y[i0:i1]), pol=torch.from_numpy(pw),
                                   time=torch.from_numpy(t[i0:i1]))
                if c['ds']:
                    ev = downsample_ev_repr(ev.unsqueeze(0), 0.5)[0]
                planes[w, b] = ev.numpy()
                bounds[b, w] = (i0, i1)
        assert np.array_equal(have['bounds'], bounds)
        path = os.path.join(GOLD, f'evseq_md_{name}.npz')
        np.savez_compressed(path, ts_end=ts_end, bounds=bounds, planes=planes)
        assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLD, 'evseq_gen1_like.npz'))
        sizes = (bounds[..., 1] - bounds[..., 0]).reshape(-1)
        print(f'{name}: windows {sizes.tolist()} events, planes min {int(planes.min())} max {int(planes.max())} '
              f'nonzero {int((planes != 0).sum())}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
