"""-m gpu: which C entry points each convolution route of u2pl_amd/nn.py issues, and in which order, pinned against
tests/golden/conv_routes.json (recorded by tools/gen_conv_routes.py; cases and recording function: tests/conv_routes.py).
A layer that changes route -- or a host-path edit that reorders, drops or doubles a launch -- shows up here as a diff of names."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_routes as CR  # noqa: E402
from conftest import GOLDEN  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "conv_routes.json")) as f:
        return json.load(f)


@pytest.fixture
def switches():
    from u2pl_amd import nn as Kn
    saved = (dict(Kn.CONV_ALGO), dict(Kn.CONV_WS), dict(Kn.CONV_H))
    yield Kn
    Kn.CONV_ALGO.update(saved[0])
    Kn.CONV_WS.update(saved[1])
    Kn.CONV_H.update(saved[2])


def test_fixture_covers_the_cases(pinned):
    assert sorted(pinned) == sorted(c["name"] for c in CR.CASES)
    for c in CR.CASES:
        assert sorted(pinned[c["name"]]) == sorted(CR.setting_key(h, w) for h, w in CR.SETTINGS)
        for per_mode in pinned[c["name"]].values():
            assert sorted(per_mode) == sorted(CR.modes(c))


@pytest.mark.parametrize("h,wino", CR.SETTINGS, ids=[CR.setting_key(h, w) for h, w in CR.SETTINGS])
@pytest.mark.parametrize("case", CR.CASES, ids=[c["name"] for c in CR.CASES])
def test_route(switches, pinned, case, h, wino):
    want = pinned[case["name"]][CR.setting_key(h, wino)]
    for mode in CR.modes(case):
        got = CR.record(switches, case, h, wino, mode)
        print(case["name"], CR.setting_key(h, wino), mode, got)
        assert got == want[mode], mode
