"""The host loop's launches are pinned: entry point, integer / float arguments and NULL-ness of every pointer, in order, must equal
the traces in tests/golden/launch_trace.json, recorded by tests/make_golden_launch_trace.py on the revision before the stage
routes moved into one record (rvt_stage_routes).  Host-code refactors must not move a launch."""
import json

import pytest
import torch

from rvt_amd import _lib
from tests import make_golden_launch_trace as LT

GOLD = json.load(open(LT.GOLDEN))


def _check(key, seq, rbs):
    got, want = LT.summary(seq), GOLD[key]
    assert got['hist'] == want['hist'], f'{key}: launches per entry point differ'
    assert got['count'] == want['count'] and got['sha256'] == want['sha256'], f'{key}: same launches, different order or arguments'
    lib = _lib.get_lib()
    for name, C, rb in rbs:              # the one argument the golden does not carry: must be the tuned tile factor
        assert rb == lib.rvt_lstm_scan3_rb(C), (key, name, C, rb)


@pytest.mark.parametrize('key,name,dt,tun,mode', LT.emu_cases(), ids=[c[0] for c in LT.emu_cases()])
def test_launch_trace_emu(key, name, dt, tun, mode):
    from tests.backends import emu_library
    _lib._install_test_library(emu_library())
    try:
        _check(key, *LT.trace_emu(name, dt, tun, mode))
    finally:
        _lib._install_test_library(None)


@pytest.mark.gpu
@pytest.mark.parametrize('key,model,mode', LT.hip_cases(), ids=[c[0] for c in LT.hip_cases()])
def test_launch_trace_gpu(production_route, key, model, mode):
    _check(key, *LT.trace_hip(model, mode))


def test_op_by_op_route_is_the_production_route_tests():
    from tests.test_production_route import OP_BY_OP
    assert LT.OP_BY_OP == OP_BY_OP


def test_golden_covers_every_case():
    assert sorted(GOLD) == sorted([c[0] for c in LT.emu_cases()] + [c[0] for c in LT.hip_cases()])
