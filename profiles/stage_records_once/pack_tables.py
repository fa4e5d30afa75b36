"""Throw-away check of issue test 6: dump the pack tables ModelWeights (`micro`, need_grad) and the PAFPN's ConvPack (`fpn_micro`) upload,
every pointer as (region, byte offset), so that the dumps of two checkouts can be diffed.  Run from a checkout's root on the emulator:
    python profiles/stage_records_once/pack_tables.py > dump.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from rvt_amd import _lib  # noqa: E402
from rvt_amd.weights import ModelWeights  # noqa: E402
from tests.backends import emu_library  # noqa: E402
from tests.test_backbone import build_model  # noqa: E402
from tests.test_fpn import _build  # noqa: E402

_lib._install_test_library(emu_library())
dev = torch.device('cpu')


def dump(title, tab, regions):
    def where(ptr):
        if ptr == 0:
            return 'NULL'
        for name, t in regions:
            off = ptr - t.data_ptr()
            if 0 <= off < t.numel() * t.element_size():
                return f'{name}+{off}'
        raise SystemExit(f'{title}: pointer {ptr} in no known region')
    lines = []
    for r in tab.rows:
        lines.append(' '.join(f'{k}={where(int(v)) if k in ("src", "dst", "scale", "S", "cs", "W", "b", "gamma", "dW", "db", "dgamma") else v}'
                              for k, v in r.items()))
    raw = tab.dev.numpy().tobytes()
    print(f'== {title}: {len(tab)} rows, {tab.blocks} blocks, {len(raw)} uploaded bytes')
    print('\n'.join(lines))
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


for dtype in (torch.bfloat16, torch.float32):
    m = build_model('micro', dev, dtype)
    params = [p for _, p in m.named_parameters()]
    p = dict(zip(m._param_names, params))
    mw = ModelWeights(m, p, m.stage_geoms(64, 96), dtype, True)
    regions = [('bufT', mw.bufT), ('buf32', mw.buf32)] + [(n, t) for n, t in p.items()] + [(f'grads{i}', sg.flat) for i, sg in enumerate(mw.grads)]
    print(dump(f'micro {dtype} pack', mw.table, regions))
    for i, sg in enumerate(mw.grads):
        print(dump(f'micro {dtype} stage {i} layerscale', sg.ls_table, regions))
        print(dump(f'micro {dtype} stage {i} unpack', sg.unpack_table, regions))
    f, _ = _build('fpn_micro', dev, dtype)
    f._pack._build(dtype, dev)
    fr = [('bufT', f._pack.bufT), ('buf32', f._pack.buf32)] + [(n, t) for n, t in f.named_parameters()]
    print(dump(f'fpn_micro {dtype} pack', f._pack.table, fr))
