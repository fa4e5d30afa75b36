"""Golden fixtures of the event-sequence builder, recorded on the CPU from the UNMODIFIED reference StackedHistogram
(data/utils/representations.py, imported from /root/reference), composed exactly as the reference's preprocessing does
(scripts/genx/preprocess_dataset.py:511-531): numpy searchsorted side='right' / 'left' (or max(end - N, 0)) over the stream's
timestamps, the reader's clip of the polarity to >= 0 (:181), one construct per window and, when down-sampling,
torch.nn.functional.interpolate(scale_factor=0.5, mode='nearest-exact') of the full-size histogram.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_evseq.py

Stored per case in tests/golden/evseq_<case>.npz (numerical data only): x<b>, y<b>, p<b> (int16) and t<b> (int64) of every
stream, ts_end, bounds int64 [B][T][2], planes uint8 (T, B, 2*bins, H', W')."""
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

from tests import casegen_evseq as cg  # noqa: E402


def main():
    from data.utils.representations import StackedHistogram

    for name in cg.CASES:
        c, streams, ts_end = cg.make_case(name)
        rep = StackedHistogram(bins=c['bins'], height=c['H'], width=c['W'], count_cutoff=c['cutoff'], fastmode=c['fastmode'])
        B, T = len(streams), ts_end.shape[-1]
        Ho, Wo = (c['H'] // 2, c['W'] // 2) if c['ds'] else (c['H'], c['W'])
        planes = np.zeros((T, B, 2 * c['bins'], Ho, Wo), dtype=np.uint8)
        bounds = np.zeros((B, T, 2), dtype=np.int64)
        data = {'ts_end': ts_end}
        for b, (x, y, p, t) in enumerate(streams):
            assert np.all(t[:-1] <= t[1:])
            te = ts_end if ts_end.ndim == 1 else ts_end[b]
            end = np.searchsorted(t, te, side='right')
            if c.get('window_events') is not None:
                start = np.maximum(end - c['window_events'], 0)
            else:
                start = np.searchsorted(t, te - c['window_us'], side='left')
            for w, (i0, i1) in enumerate(zip(start, end)):
                pw = np.clip(p[i0:i1], a_min=0, a_max=None)
                ev = rep.construct(x=torch.from_numpy(x[i0:i1]), y=torch.from_numpy(y[i0:i1]), pol=torch.from_numpy(pw),
                                   time=torch.from_numpy(t[i0:i1]))
                if c['ds']:
                    ev = torch.nn.functional.interpolate(ev.unsqueeze(0), scale_factor=0.5, mode='nearest-exact')[0]
                planes[w, b] = ev.numpy()
                bounds[b, w] = (i0, i1)
            for k, a in (('x', x), ('y', y), ('p', p)):
                assert a.min(initial=0) >= -2 ** 15 and a.max(initial=0) < 2 ** 15
                data[f'{k}{b}'] = a.astype(np.int16)
            data[f't{b}'] = t
        path = os.path.join(ROOT, 'tests', 'golden', f'evseq_{name}.npz')
        np.savez_compressed(path, bounds=bounds, planes=planes, **data)
        sizes = (bounds[..., 1] - bounds[..., 0]).reshape(-1)
        print(f'{name}: windows {sizes.tolist()} events, planes sum {int(planes.sum())} max {int(planes.max())}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
