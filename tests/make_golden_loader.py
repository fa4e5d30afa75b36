"""Golden fixtures of the loader's index rules recorded from the UNMODIFIED reference (data/genx_utils/sequence_rnd.py,
sequence_for_streaming.py, data/utils/stream_sharded_datapipe.py, imported from /root/reference).

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_loader.py

The reference imports torchdata, h5py and torchvision.transforms, none of which is installed.  This recorder registers in-memory
stand-ins at run time: torchdata with empty MapDataPipe / IterDataPipe base classes and Concater / ZipperLongest / Zipper that only
keep their arguments; an h5py.File that serves a .npy stored under the .h5 name; torchvision.transforms as make_golden_augment.py
does.  Each case of tests/casegen_loader.py is written as a temporary sequence directory (event_representations_v2/<name>/
{event_representations.h5, objframe_idx_2_repr_idx.npy}, labels_v2/labels.npz) and read through the reference's classes.

Stored per sequence case in tests/golden/<case>.npz (arrays only), for each of rnd (SequenceForRandomAccess), rnd_end (the same
with only_load_end_labels), it (SequenceForIter) and guar (get_sequences_with_guaranteed_labels, items of all sub-sequences one
behind the other): <p>_windows [n][T] (read back from the frames; -1 = a padded frame), <p>_first [n], <p>_padded [n][T],
<p>_label_n [n][T] (-1 = None) and <p>_rows [sum][7] (the label rows in item and step order); guar_seq [n] (the item's
sub-sequence) and guar_ranges [k][2].  tests/golden/loader_sharding.npz: assign_W<w>_R<r> (positions of the streams of rank r of w)
and slots_W<w>_R<r>_B<b> [b][*] (positions per batch slot, -1 padded; an empty array where the reference's assertion fires)."""
import enum
import os
import sys
import tempfile
import types
from pathlib import Path

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, '/root/reference')
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torchvision  # noqa: E402  (the stub)

from tests import casegen_loader as cg  # noqa: E402

EV_NAME = 'stacked_histogram_test'


def _register_stand_ins():
    tr = types.ModuleType('torchvision.transforms')
    fn = types.ModuleType('torchvision.transforms.functional')

    class InterpolationMode(enum.Enum):
        NEAREST = 'nearest'

    def rotate(*a, **k):
        raise NotImplementedError('torchvision stand-in: rotate is outside the recorded scope')
    tr.InterpolationMode, fn.rotate, tr.functional = InterpolationMode, rotate, fn
    torchvision.transforms = tr
    sys.modules['torchvision.transforms'], sys.modules['torchvision.transforms.functional'] = tr, fn

    class MapDataPipe:
        def to_iter_datapipe(self):
            return self

    class IterDataPipe:
        pass

    class _Keeps(IterDataPipe):
        def __init__(self, *args, **kwargs):
            self.args, self.kwargs = args, kwargs

    td, dp = types.ModuleType('torchdata'), types.ModuleType('torchdata.datapipes')
    it, mp = types.ModuleType('torchdata.datapipes.iter'), types.ModuleType('torchdata.datapipes.map')
    it.IterDataPipe, mp.MapDataPipe = IterDataPipe, MapDataPipe
    it.Concater, it.ZipperLongest, it.Zipper, it.IterableWrapper = (type(n, (_Keeps,), {}) for n in ('Concater', 'ZipperLongest', 'Zipper', 'IterableWrapper'))
    td.datapipes, dp.iter, dp.map = dp, it, mp
    sys.modules.update({'torchdata': td, 'torchdata.datapipes': dp, 'torchdata.datapipes.iter': it, 'torchdata.datapipes.map': mp})

    h5 = types.ModuleType('h5py')

    class File:
        def __init__(self, path, mode='r'):
            assert mode == 'r'
            self._data = {'data': np.load(path)}

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def __getitem__(self, key):
            return self._data[key]
    h5.File = File
    sys.modules['h5py'] = h5
    return MapDataPipe


def _write_sequence(root: Path, name: str) -> Path:
    c = cg.SEQ_CASES[name]
    seq = root / name
    ev = seq / 'event_representations_v2' / EV_NAME
    ev.mkdir(parents=True)
    (seq / 'labels_v2').mkdir()
    with open(ev / 'event_representations.h5', 'wb') as f:
        np.save(f, cg.frames(name))
    np.save(ev / 'objframe_idx_2_repr_idx.npy', np.asarray(c['o2r'], dtype=np.int64))
    lab, idx = cg.structured_labels(name)
    np.savez(seq / 'labels_v2' / 'labels.npz', labels=lab, objframe_idx_2_label_idx=idx)
    return seq


def _record_items(prefix, items, DataType, out, seq_ids=None):
    wins, first, padded, label_n, rows = [], [], [], [], [np.zeros((0, 7), dtype=np.float32)]
    for item in items:
        ev = np.stack([e.numpy() for e in item[DataType.EV_REPR]])
        wins.append(cg.windows_of(ev))
        first.append(bool(item[DataType.IS_FIRST_SAMPLE]))
        padded.append(np.asarray(item[DataType.IS_PADDED_MASK], dtype=bool))
        n = []
        for lab in item[DataType.OBJLABELS_SEQ]:
            n.append(-1 if lab is None else len(lab))
            if lab is not None:
                rows.append(lab.object_labels.numpy().astype(np.float32))
        label_n.append(n)
    T = cg.T
    out[prefix + '_windows'] = np.asarray(wins, dtype=np.int64).reshape(-1, T)
    out[prefix + '_first'] = np.asarray(first, dtype=bool)
    out[prefix + '_padded'] = np.asarray(padded, dtype=bool).reshape(-1, T)
    out[prefix + '_label_n'] = np.asarray(label_n, dtype=np.int64).reshape(-1, T)
    out[prefix + '_rows'] = np.concatenate(rows)
    if seq_ids is not None:
        out[prefix + '_seq'] = np.asarray(seq_ids, dtype=np.int64)


def main():
    MapDataPipe = _register_stand_ins()
    from data.genx_utils.sequence_for_streaming import SequenceForIter
    from data.genx_utils.sequence_rnd import SequenceForRandomAccess
    from data.utils.stream_sharded_datapipe import ShardedStreamingDataPipe
    from data.utils.types import DatasetType, DataType

    golden = os.path.join(ROOT, 'tests', 'golden')
    kw = dict(ev_representation_name=EV_NAME, sequence_length=cg.T, dataset_type=DatasetType.GEN1, downsample_by_factor_2=False)
    with tempfile.TemporaryDirectory() as tmp:
        for name in cg.SEQ_CASES:
            path = _write_sequence(Path(tmp), name)
            out = {}
            for prefix, end in (('rnd', False), ('rnd_end', True)):
                seq = SequenceForRandomAccess(path=path, only_load_end_labels=end, **kw)
                _record_items(prefix, [seq[i] for i in range(len(seq))], DataType, out)
            seq = SequenceForIter(path=path, **kw)
            _record_items('it', [seq[i] for i in range(len(seq))], DataType, out)
            subs = SequenceForIter.get_sequences_with_guaranteed_labels(path=path, **kw)
            _record_items('guar', [s[i] for s in subs for i in range(len(s))], DataType, out,
                          seq_ids=[k for k, s in enumerate(subs) for _ in range(len(s))])
            out['guar_ranges'] = np.asarray([(s.start_indices[0], s.stop_indices[-1]) for s in subs], dtype=np.int64).reshape(-1, 2)
            filler = seq.get_fully_padded_sample()
            out['filler_first'] = np.asarray(bool(filler[DataType.IS_FIRST_SAMPLE]))
            out['filler_padded'] = np.asarray(filler[DataType.IS_PADDED_MASK], dtype=bool)
            np.savez_compressed(os.path.join(golden, name + '.npz'), **out)
            print(f"{name}: rnd {len(out['rnd_first'])} items, it {len(out['it_first'])} chunks, guar {out['guar_ranges'].tolist()}")

    class Stream(MapDataPipe):
        def __init__(self, pos, length):
            self.pos, self.length = pos, length

        def __len__(self):
            return self.length

    out = {}
    pipes = [Stream(i, n) for i, n in enumerate(cg.SHARD_LENGTHS)]
    for w in cg.SHARD_WORLDS:
        for b in cg.SHARD_BATCH_SIZES:
            sharded = ShardedStreamingDataPipe(datapipe_list=pipes, batch_size=b, fill_value=None)
            for r in range(w):
                mine = ShardedStreamingDataPipe.assign_datapipes_to_worker(sorted_datapipe_list=sharded.datapipe_list, total_num_workers=w,
                                                                           global_worker_id=r)
                out[f'assign_W{w}_R{r}'] = np.asarray([p.pos for p in mine], dtype=np.int64)
                try:
                    zipped = sharded.get_zipped_stream_from_worker_datapipes(datapipe_list=mine, batch_size=b)
                    slots = [[p.pos for p in c.args] for c in zipped.args]
                    arr = np.full((b, max(len(s) for s in slots)), -1, dtype=np.int64)
                    for k, s in enumerate(slots):
                        arr[k, :len(s)] = s
                except AssertionError:
                    arr = np.zeros((0, 0), dtype=np.int64)
                out[f'slots_W{w}_R{r}_B{b}'] = arr
    np.savez_compressed(os.path.join(golden, 'loader_sharding.npz'), **out)
    print({k: v.tolist() for k, v in out.items()})


if __name__ == '__main__':
    main()
