"""Throw-away check of the detector-tail refactor: dump the pack tables ModelWeights (`micro`, need_grad) and the ConvPacks of the
PAFPN (`fpn_micro`) and of the YOLOX head (`head_micro`) upload, every pointer as (region, byte offset), with the arena sizes, the
statistics extent and where every unit's views lie, so that the dumps of two checkouts can be diffed.  The ConvPacks are built the way
a forward builds them (ConvPack.refresh), not through a private builder.  Run from a checkout's root on the emulator:
    python profiles/detector_tail_once/pack_tables.py [--full] > dump.txt
Default: per table its size and the SHA-256 of its rows, per ConvPack the arenas, the statistics extent and the SHA-256 of the unit views;
--full prints every row and every unit as well (529 lines)."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from rvt_amd import _lib  # noqa: E402
from rvt_amd.weights import ModelWeights  # noqa: E402
from tests.backends import emu_library  # noqa: E402
from tests.test_backbone import build_model  # noqa: E402
from tests.test_fpn import _build as build_fpn  # noqa: E402
from tests.test_head import _build as build_head  # noqa: E402

_lib._install_test_library(emu_library())
dev = torch.device('cpu')
FULL = '--full' in sys.argv
POINTERS = ('src', 'dst', 'scale', 'S', 'cs', 'W', 'b', 'gamma', 'dW', 'db', 'dgamma')


def where(title, ptr, regions):
    if ptr == 0:
        return 'NULL'
    for name, t in regions:
        off = ptr - t.data_ptr()
        if 0 <= off < t.numel() * t.element_size():
            return f'{name}+{off}'
    raise SystemExit(f'{title}: pointer {ptr} in no known region')


def dump(title, tab, regions):
    lines = [' '.join(f'{k}={where(title, int(v), regions) if k in POINTERS else v}' for k, v in r.items()) for r in tab.rows]
    raw = tab.dev.numpy().tobytes()
    print(f'== {title}: {len(tab)} rows, {tab.blocks} blocks, {len(raw)} uploaded bytes')
    if FULL:
        print('\n'.join(lines))
    return hashlib.sha256('\n'.join(lines).encode()).hexdigest()


def dump_convpack(title, mod, dtype):
    pack = mod._pack
    pack.refresh(dtype, False)
    regions = [('bufT', pack.bufT), ('buf32', pack.buf32)] + [(n, t) for n, t in mod.named_parameters()]
    print(dump(f'{title} pack', pack.table, regions))
    print(f'== {title} arenas: bufT {pack.bufT.dtype} x {pack.bufT.numel()}, buf32 {pack.buf32.dtype} x {pack.buf32.numel()}, '
          f'statistics extent {where(title, pack.stats_all.data_ptr(), regions)} x {pack.stats_all.numel()}, {len(pack.counters)} counters')
    units = []
    for i, c in enumerate(pack.convs):
        pk = c._pk
        units.append(f'unit {i}: ' + ' '.join(f'{k}={where(title, getattr(pk, k).data_ptr(), regions)}x{getattr(pk, k).numel()}:{getattr(pk, k).dtype}'
                                       for k in ('stats', 'wp', 'wd', 'dwp')) + f' dtype={pk.dtype} cin={pk.cin}')
    if FULL:
        print('\n'.join(units))
    print(f'== {title} views: {len(units)} units {hashlib.sha256(chr(10).join(units).encode()).hexdigest()}')


for dtype in (torch.bfloat16, torch.float32):
    m = build_model('micro', dev, dtype)
    params = [p for _, p in m.named_parameters()]
    p = dict(zip(m._param_names, params))
    mw = ModelWeights(m, p, m.stage_geoms(64, 96), dtype, True)
    regions = [('bufT', mw.bufT), ('buf32', mw.buf32)] + [(n, t) for n, t in p.items()] + [(f'grads{i}', sg.flat) for i, sg in enumerate(mw.grads)]
    print(dump(f'micro {dtype} pack', mw.table, regions))
    print(f'== micro {dtype} arenas: bufT {mw.bufT.dtype} x {mw.bufT.numel()}, buf32 {mw.buf32.dtype} x {mw.buf32.numel()}')
    for i, sg in enumerate(mw.grads):
        print(dump(f'micro {dtype} stage {i} layerscale', sg.ls_table, regions))
        print(dump(f'micro {dtype} stage {i} unpack', sg.unpack_table, regions))
    dump_convpack(f'fpn_micro {dtype}', build_fpn('fpn_micro', dev, dtype)[0].eval(), dtype)
    dump_convpack(f'head_micro {dtype}', build_head('head_micro', dev, dtype)[0].eval(), dtype)
