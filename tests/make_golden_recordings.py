"""Golden fixtures of the raw-recording path (tests/golden/rec_dat_<case>.npz, rec_labels_<case>.npz), recorded on the CPU from the
UNMODIFIED reference (imported from /root/reference) on the inputs of tests/casegen_recordings.py:

  * utils/evaluation/prophesee/io/dat_events_tools.py: parse_header and load_td_data on the generated DAT files;
  * scripts/genx/preprocess_dataset.py: H5Reader._correct_time on the loaded timestamps, apply_filters and
    labels_and_ev_repr_timestamps on the generated box arrays, and the offsets save_labels computes;
  * data/genx_utils/labels.py: ObjectLabelFactory.from_structured_array(...)[frame] at full and at half scale.

preprocess_dataset.py imports h5py, numba and omegaconf.MISSING, none of which this container has; none of them is touched by the
functions above.  The recorder puts throwaway modules of its own into sys.modules (an h5py that holds nothing but the name its
annotations mention, a numba whose jit hands the function back, MISSING on the omegaconf stand-in of oracle/_stubs) and loads the
file by path.  The vendored write_header names
an undefined EV_STRINGS, so the DAT header bytes come from the case generator.  The inputs must satisfy the reference's own asserts;
where they do not, the reference raises and so does this script.

TEST INFRASTRUCTURE; runs only in the authoring container and is not collected by pytest.
Usage: python tests/make_golden_recordings.py

Stored (numerical data only, written with fixed zip timestamps so that a rerun gives the same bytes):
  rec_dat_<case>.npz: raw uint8 (the file), header int64 [offset, ev_type, ev_size, height, width] (-1 = absent), x, y, p int16,
    t int64 (load_td_data's uint32), t_repaired int64.
  rec_labels_<case>.npz: inp (box records in), filtered (apply_filters), labels + objframe_idx_2_label_idx, frame_ts_us,
    ev_repr_ts_end_us, frameidx_2_repridx, rows_full / rows_half fp32 [n][7] of all frames with rows_full_off / rows_half_off
    int64 [frames + 1]; no_labels = 1 and only inp where the reference raises NoLabelsException.
  rec_rows_edge.npz: labels + objframe_idx_2_label_idx of casegen_recordings.make_edge_labels and the factory's rows_full /
    rows_half (+ _off) for them: boxes that go flat at half scale, one frame left empty."""
import importlib.util
import io
import os
import sys
import tempfile
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = '/root/reference'
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_stubs'))
sys.path.insert(1, REF)
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import casegen_recordings as cr  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 64 * 1024


def load_reference():
    import omegaconf
    if not hasattr(omegaconf, 'MISSING'):
        omegaconf.MISSING = '???'
    h5py = types.ModuleType('h5py')
    h5py.File = type('File', (), {})                     # named in annotations only
    sys.modules.setdefault('h5py', h5py)
    numba = types.ModuleType('numba')
    numba.jit = lambda *a, **k: (lambda f: f)
    sys.modules.setdefault('numba', numba)
    spec = importlib.util.spec_from_file_location('ref_preprocess_dataset', os.path.join(REF, 'scripts', 'genx', 'preprocess_dataset.py'))
    pre = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pre)
    from utils.evaluation.prophesee.io import dat_events_tools
    from data.genx_utils.labels import ObjectLabelFactory
    return pre, dat_events_tools, ObjectLabelFactory


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed timestamp on every member: the same arrays give the same file."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))


def record_dat(pre, dat, tmp):
    for name in cr.DAT_CASES:
        c, raw = cr.make_dat(name)
        path = os.path.join(tmp, f'{name}_td.dat')
        raw.tofile(path)
        with open(path, 'rb') as f:
            bod, ev_type, ev_size, size = dat.parse_header(f)
        ev = dat.load_td_data(path)
        assert ev.shape[0] == c['n'] and (ev_type, ev_size) == (0, 8), name
        t = ev['t'].astype(np.int64)
        fixed = t.copy()
        pre.H5Reader._correct_time(fixed)
        header = np.array([bod, ev_type, ev_size] + [-1 if s is None else s for s in size], dtype=np.int64)
        out = os.path.join(GOLD, f'rec_dat_{name}.npz')
        save_npz(out, raw=raw, header=header, x=ev['x'], y=ev['y'], p=ev['p'], t=t, t_repaired=fixed)
        print(f'dat {name}: {t.size} events, header {header.tolist()}, {int((fixed != t).sum())} timestamps repaired, p in '
              f'{sorted(set(ev["p"].tolist()))}, x {int(ev["x"].min())}..{int(ev["x"].max())}, t max {int(t.max())}, {os.path.getsize(out)} bytes')


def record_labels(pre, factory, tmp):
    from omegaconf import DictConfig
    for name in cr.LABEL_CASES:
        c, inp = cr.make_labels(name)
        path = os.path.join(tmp, f'{name}_bbox.npy')
        np.save(path, inp)
        split = pre.split_name_2_type[c['split']]
        cfg = DictConfig(dict(apply_psee_bbox_filter=c['psee'], apply_faulty_bbox_filter=c['faulty']))
        filtered = pre.apply_filters(labels=inp.copy(), split_type=split, filter_cfg=cfg, dataset_type=c['dataset'])
        out = os.path.join(GOLD, f'rec_labels_{name}.npz')
        from pathlib import Path
        try:
            per_frame, frame_ts, ends, f2r = pre.labels_and_ev_repr_timestamps(
                npy_file=Path(path), split_type=split, filter_cfg=cfg, align_t_ms=c['align_t_ms'], ts_step_ev_repr_ms=c['step_ms'],
                dataset_type=c['dataset'])
        except pre.NoLabelsException:
            assert filtered.size == 0
            save_npz(out, inp=inp, no_labels=np.array(1))
            print(f'labels {name}: {inp.size} boxes in, none survives, {os.path.getsize(out)} bytes')
            continue
        assert np.array_equal(np.load(path), inp)                        # the file on disk is what the reference was given
        labels = np.concatenate(per_frame)
        offsets = np.cumsum([0] + [len(x) for x in per_frame[:-1]]).astype(np.int64)   # save_labels' objframe_idx_2_label_idx
        H, W = cr.HW[c['dataset']]
        rows = factory_rows(factory, labels, offsets, (H, W))
        save_npz(out, inp=inp, filtered=filtered, labels=labels, objframe_idx_2_label_idx=offsets, frame_ts_us=frame_ts,
                 ev_repr_ts_end_us=ends, frameidx_2_repridx=f2r.astype(np.int64), rows_full=rows['full'], rows_full_off=rows['full_off'],
                 rows_half=rows['half'], rows_half_off=rows['half_off'])
        print(f'labels {name}: {inp.size} boxes in, {filtered.size} filtered, {labels.size} in {len(frame_ts)} frames of '
              f'{np.unique(filtered["t"]).size} label times, {ends.size} windows, frame->window {f2r.tolist()}, '
              f'half-scale rows {rows["half"].shape[0]}, {os.path.getsize(out)} bytes')


def factory_rows(factory, labels, offsets, hw):
    rows = {}
    for key, factor in (('full', None), ('half', 2)):
        fac = factory.from_structured_array(labels, offsets, hw, factor)
        per = [fac[i].object_labels.numpy() for i in range(len(fac))]
        rows[key] = np.concatenate(per).astype(np.float32)
        rows[key + '_off'] = np.cumsum([0] + [len(x) for x in per]).astype(np.int64)
    return rows


def record_edge_rows(factory):
    """The label factory alone on boxes that go flat at half scale (no filter lets such a box through, so no recording case has one)."""
    dataset, labels, offsets = cr.make_edge_labels()
    rows = factory_rows(factory, labels, offsets, cr.HW[dataset])
    assert rows['half'].shape[0] < rows['full'].shape[0] and rows['half_off'][-1] == rows['half_off'][-2], 'no box went flat'
    out = os.path.join(GOLD, 'rec_rows_edge.npz')
    save_npz(out, labels=labels, objframe_idx_2_label_idx=offsets, rows_full=rows['full'], rows_full_off=rows['full_off'],
             rows_half=rows['half'], rows_half_off=rows['half_off'])
    print(f'rows edge: {rows["full"].shape[0]} rows at full size, {rows["half"].shape[0]} at half scale, offsets {rows["half_off"].tolist()}, '
          f'{os.path.getsize(out)} bytes')


def main():
    pre, dat, factory = load_reference()
    with tempfile.TemporaryDirectory() as tmp:
        record_dat(pre, dat, tmp)
        record_labels(pre, factory, tmp)
    record_edge_rows(factory)
    assert not os.path.exists(os.path.join(REF, 'scripts', 'genx', '__pycache__')), 'bytecode leaked into the reference tree'


if __name__ == '__main__':
    main()
