"""The DRN forward makes exactly the Engine calls, in the order and with the arguments, and adds exactly the FLOP / byte
counters that tests/drn_routes.json recorded before drn.py's dispatch was split into choose / count / launch (tests/drn_trace.py:
both architectures, every arithmetic mode, narrow maps, rows that fill the direct kernels' tiles, and the smallest batch
whose 56 x 56 maps exceed 2^20 pixels)."""
import importlib
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drn_trace  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def drn():
    return importlib.import_module('superpixel-align_amd.drn')


@pytest.fixture(scope='module')
def models(drn):
    return drn_trace.models(drn)


@pytest.fixture(scope='module')
def recorded():
    with open(drn_trace.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('cid,arch,mode,shape', drn_trace.cases(), ids=[c[0] for c in drn_trace.cases()])
def test_forward_makes_the_recorded_calls_and_counts(drn, models, recorded, cid, arch, mode, shape):
    got = json.loads(json.dumps(drn_trace.record(drn, models[(arch, drn_trace.MODES[mode][0])], mode, shape)))
    want = recorded[cid]
    assert [c[0] for c in got['calls']] == [c[0] for c in want['calls']]
    for i, (g, w) in enumerate(zip(got['calls'], want['calls'])):
        assert g == w, 'call %d' % i
    assert got['library_convs'] == want['library_convs']
    assert got['counters'] == want['counters']
