"""rvt_stage_seq_fwd_ws_bytes / rvt_stage_seq_bwd_ws_bytes over the grid of tests/test_route_record.py::test_planner_invariants, for two builds
of the library (the CPU emulator build: the size functions are host code).  `save` as each function needs it: the forward size plans
a no-grad forward itself, the backward size reads the routes of rvt_stage_routes(save = 1).
usage: python profiles/stage_drivers_once/ws_bytes.py <parent librvt_emu.so> <this tree's librvt_emu.so>"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from rvt_amd import _lib, stage_driver, tuning  # noqa: E402
from tests.test_route_record import _desc  # noqa: E402


def table(path):
    lib = _lib._bind(ctypes.CDLL(path))
    _lib._install_test_library(lib)
    out = {}
    for tun, fields in (('production', {}), ('test_geometry', tuning.TEST_GEOMETRY)):
        tuning.use(**fields)
        for dtype in (torch.bfloat16, torch.float32):
            for C in (32, 64, 128, 256, 512):
                for T, tokens in ((1, 2560), (21, 2560), (21, 92160)):
                    d, keep, B = _desc(dtype, C, T, tokens)
                    tr, saved = stage_driver.RvtStageTrain(), (stage_driver.RvtBlockSaved * 2)()
                    tr.struct_bytes, tr.saved = ctypes.sizeof(tr), ctypes.cast(saved, ctypes.POINTER(stage_driver.RvtBlockSaved))
                    assert lib.rvt_stage_routes(ctypes.byref(d), T, B, 1, 0, 0, ctypes.byref(tr.routes)) == 0
                    out[(tun, str(dtype)[6:], C, T, tokens)] = (int(lib.rvt_stage_seq_fwd_ws_bytes(ctypes.byref(d), T, B)),
                                                                int(lib.rvt_stage_seq_bwd_ws_bytes(ctypes.byref(d), ctypes.byref(tr), T, B)))
    tuning.production()
    _lib._install_test_library(None)
    return out


if __name__ == '__main__':
    old, new = table(sys.argv[1]), table(sys.argv[2])
    print(f'{"record":14s} {"dtype":9s} {"C":>4s} {"T":>3s} {"tokens":>7s} {"fwd parent":>13s} {"fwd new":>13s} {"bwd parent":>13s} {"bwd new":>13s}  grows')
    grown = 0
    for k in old:
        g = new[k][0] > old[k][0] or new[k][1] > old[k][1]
        grown += g
        print(f'{k[0]:14s} {k[1]:9s} {k[2]:4d} {k[3]:3d} {k[4]:7d} {old[k][0]:13d} {new[k][0]:13d} {old[k][1]:13d} {new[k][1]:13d}  {"YES" if g else "no"}')
    print(f'{len(old)} entries, {grown} grow; sum forward {sum(v[0] for v in old.values())} -> {sum(v[0] for v in new.values())}, '
          f'backward {sum(v[1] for v in old.values())} -> {sum(v[1] for v in new.values())}')
    sys.exit(1 if grown else 0)
