"""The detector tail's launches are pinned like the backbone's (tests/test_launch_trace.py): entry point, integer / float arguments
and NULL-ness of every pointer, in order, of the PAFPN and the YOLOX head at their smallest fixtures must equal the traces in
tests/golden/tail_launch_trace.json, recorded by `python -m tests.make_golden_launch_trace --backend emu --suite tail` on the revision
before the tail's weight caches moved onto the backbone's builder and cache protocol.  The tail's Python decides nothing by backend:
the MI355X cases compare against the same golden."""
import json

import pytest
import torch

from rvt_amd import _lib
from tests import make_golden_launch_trace as LT

GOLD = json.load(open(LT.TAIL_GOLDEN))
CASES = LT.tail_cases()


def _check(key, seq):
    got, want = LT.summary(seq), GOLD[key]
    assert got['hist'] == want['hist'], f'{key}: launches per entry point differ'
    assert got['count'] == want['count'] and got['sha256'] == want['sha256'], f'{key}: same launches, different order or arguments'


@pytest.mark.parametrize('key,name,dt,mode', CASES, ids=[c[0] for c in CASES])
def test_tail_launch_trace_emu(key, name, dt, mode):
    from tests.backends import emu_library
    _lib._install_test_library(emu_library())
    try:
        _check(key, LT.trace_tail(name, dt, mode)[0])
    finally:
        _lib._install_test_library(None)


@pytest.mark.gpu
@pytest.mark.parametrize('name', LT.TAIL_FIXTURES)
def test_tail_launch_trace_gpu(name):
    for key, n, dt, mode in CASES:
        if n == name:
            _check(key, LT.trace_tail(n, dt, mode, torch.device('cuda', 0))[0])


def test_tail_golden_covers_every_case():
    assert sorted(GOLD) == sorted(c[0] for c in CASES)
