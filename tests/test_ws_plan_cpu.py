"""The tile plan of the pre-split GEMMs (csrc/igemm_ws.hip plan_igemm_ws), queried through u2pl_igemm_ws_plan, against its restatement in
tests/igemm_ref.py -- over a sweep that crosses every boundary of the cost model, in every switch state.  U2PL_WS_NARROW, U2PL_WS_MIX2
and U2PL_WS_FIX2 are read once per process: the default state is checked in this process, each forced value in a child of its own."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import igemm_ref as R  # noqa: E402

EINVAL = 1001
SWITCHES = ("U2PL_WS_NARROW", "U2PL_WS_MIX2", "U2PL_WS_FIX2")
PERSIST = "U2PL_WS_PERSIST"          # (read at the first use, then held by u2pl_igemm_ws_set_persist)


def _query(L, M, K, Cout, batch, np_):
    out = (ctypes.c_int * 3)()
    assert L.u2pl_igemm_ws_plan(M, K, Cout, batch, np_, out) == 0, (M, K, Cout, batch, np_)
    return tuple(out)


def _atof(s):
    """C's atof on a decimal string: the longest numeric prefix, 0.0 where there is none"""
    m = re.match(r"\s*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?)", s)
    return float(m.group(0)) if m else 0.0


def _state(env):
    """the restatement's switch arguments for an environment (the library's atoi / atof of a set, non-empty variable)"""
    e = {k: env.get(k) or None for k in SWITCHES + (PERSIST,)}
    return dict(narrow=None if e[SWITCHES[0]] is None else R._atoi(e[SWITCHES[0]]), mix2=0 if e[SWITCHES[1]] is None else int(R._atoi(e[SWITCHES[1]]) != 0),
                fix2=2.0 if e[SWITCHES[2]] is None else _atof(e[SWITCHES[2]]), persist=1 if e[PERSIST] is None else int(R._atoi(e[PERSIST]) != 0))


def _library_plans():
    from u2pl_amd._lib import lib
    L = lib()
    return [[_query(L, *c, np_) for np_ in (3, 2)] for c in R.ws_plan_sweep()]


def _compare(plans, **state):
    kinds = set()
    for c, got in zip(R.ws_plan_sweep(), plans):
        for np_, g in zip((3, 2), got):
            want = tuple(R.plan_igemm_ws(*c, np_, **state))
            assert tuple(g) == want, (c, np_, state, tuple(g), want)
            kinds.add(want[0])
    return kinds


def test_default_plan_and_persist_switch_against_the_restatement():
    from u2pl_amd._lib import lib
    L = lib()
    state = _state(os.environ)
    old = L.u2pl_igemm_ws_set_persist(state["persist"])          # (another test of the process may have left the switch either way)
    try:
        kinds = _compare(_library_plans(), **state)
    finally:
        L.u2pl_igemm_ws_set_persist(old)
    if state == dict(narrow=None, mix2=0, fix2=2.0, persist=1):
        assert kinds == {R.WS_WIDE, R.WS_NARROW, R.WS_MIXED}                  # the sweep reaches every default plan
        # the boundaries by name: the first chunk count at which 257 wide tiles run mixed
        assert _query(L, 257 * 128, 416, 256, 1, 3)[0] == R.WS_NARROW and _query(L, 257 * 128, 448, 256, 1, 3) == (R.WS_MIXED, 256, 2)
        assert _query(L, 257 * 128, 832, 256, 1, 2)[0] == R.WS_NARROW and _query(L, 257 * 128, 864, 256, 1, 2) == (R.WS_MIXED, 256, 2)
        assert _query(L, 384 * 128, 2304, 256, 1, 3) == (R.WS_MIXED, 256, 256)                # 2 rem = 256: the largest mixable remainder
        assert _query(L, 385 * 128, 2304, 256, 1, 3)[0] != R.WS_MIXED                         # 2 rem = 258
        assert _query(L, 257 * 128, 2304, 384, 1, 3)[0] != R.WS_MIXED                         # three narrow column tiles for two wide ones
        assert _query(L, 1000 * 128, 4608, 128, 1, 3) == (R.WS_NARROW, 0, 1000)
    old = L.u2pl_igemm_ws_set_persist(0)
    try:
        assert R.WS_MIXED not in _compare(_library_plans(), **dict(state, persist=0))   # one block per tile: nothing to hand the CUs over to
    finally:
        L.u2pl_igemm_ws_set_persist(old)


@pytest.mark.parametrize("name,value", [(SWITCHES[0], "0"), (SWITCHES[0], "1"), (SWITCHES[0], "2"), (SWITCHES[1], "1")])
def test_forced_plans_against_the_restatement(name, value):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env[name] = value
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kinds = _compare(json.loads(r.stdout), **_state(env))
    if name == SWITCHES[1] and not os.environ.get(SWITCHES[0]) and _state(env)["persist"]:
        assert R.WS_MIXED2 in kinds and R.WS_MIXED not in kinds
        # two launches cost 8 fixed units instead of 2: on 257 tiles the plan is chosen from 54 chunks (np 3) and 107 (np 2, U2PL_WS_FIX2 = 2)
        if not os.environ.get(SWITCHES[2]):
            assert [tuple(R.plan_igemm_ws(257 * 128, K, 256, 1, np_, mix2=1))[0] for K, np_ in ((1696, 3), (1728, 3), (3392, 2), (3424, 2))] == [
                R.WS_NARROW, R.WS_MIXED2, R.WS_NARROW, R.WS_MIXED2]
    elif name == SWITCHES[0]:
        assert R.WS_MIXED not in kinds and R.WS_MIXED2 not in kinds


def test_query_refusals():
    from u2pl_amd._lib import lib
    L = lib()
    out = (ctypes.c_int * 3)()
    for args in ((0, 256, 256, 1, 3), (128, 0, 256, 1, 3), (128, 256, 0, 1, 3), (128, 256, 256, 0, 3), (128, 256, 256, 1, 1), (128, 256, 256, 1, 4)):
        assert L.u2pl_igemm_ws_plan(*args, out) == EINVAL, args
    assert L.u2pl_igemm_ws_plan(128, 256, 256, 1, 3, None) == EINVAL
    # what would not fit the int results: the launches refuse 2^31 rows and 2^30 tiles as well
    assert L.u2pl_igemm_ws_plan(1 << 31, 256, 256, 1, 3, out) == EINVAL
    assert L.u2pl_igemm_ws_plan(1 << 30, 256, 256, 128, 3, out) == EINVAL and L.u2pl_igemm_ws_plan(1 << 30, 256, 256, 64, 3, out) == 0
    assert L.u2pl_igemm_ws_plan(1 << 30, 256, 128, 128, 3, out) == EINVAL                 # narrow tiles


if __name__ == "__main__":          # the child of test_forced_plans_against_the_restatement: this process's plans, as JSON
    sys.path.insert(0, ROOT)
    print(json.dumps(_library_plans()))
