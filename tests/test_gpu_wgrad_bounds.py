"""-m gpu: every weight-gradient kernel through the C ABI, element-wise against float64, at each slab and tile edge.

Entry points: u2pl_conv2d_wgrad_h_f32, u2pl_conv2d_wgrad_f32, u2pl_conv2d_wgrad_bf16op_f32, u2pl_wgrad_batched_h_f32,
u2pl_wgrad_batched_f32, under the four states of u2pl_conv_set_split x u2pl_wgrad_set_tr.  The table of edges, the reference, the bound
per arithmetic and the planner restatement live in tests/wgrad_ref.py; tests/test_wgrad_cpu.py shows on an emulation that the bound
rejects a kernel that drops a slab, a chunk, a guard, a piece product or the pitch.  Every case asserts through
u2pl_wgrad_batched_splits and the restatement that it hits the edge it is named for.  On every launch: the workspace is NaN before the
call (a slab element the reduce reads and nobody wrote makes dw NaN), 64 NaN floats behind the slabs and 0xA5 bytes around dw must
survive, dw sits once 16 bytes past a 256-byte boundary, the second call gives the first one's bits, and accumulate = 1 adds onto a
previous dw of the gradient's own size.  Refusals are CPU tests (test_wgrad_cpu.py): nothing here passes an invalid pointer or size.
Each test prints its excess (pytest -s); U2PL_WGRAD_RECORD=path writes the worst |got - f64| / bound per (kernel family, arithmetic)
as JSON (profiles/wgrad_bounds.json is one such run: a record, not a threshold)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 64
WORST = {}


def _call(name, *args):
    from u2pl_amd._lib import call
    call(name, *args)


def _query(name, *args):
    from u2pl_amd._lib import query
    return query(name, *args)


def _note(family, e):
    WORST[family] = max(WORST.get(family, 0.0), e)


@pytest.fixture(scope="module", autouse=True)
def _records():
    yield
    path = os.environ.get("U2PL_WGRAD_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(WORST.items())}, f, indent=1)
            f.write("\n")


class Switches:
    """u2pl_conv_set_split / u2pl_wgrad_set_tr, set and verified; restore() puts both back"""
    def __init__(self):
        self.old = (_query("u2pl_conv_get_split"), _query("u2pl_wgrad_set_tr", 1))
        _query("u2pl_wgrad_set_tr", self.old[1])

    def set(self, split, tr):
        _query("u2pl_conv_set_split", split)
        _query("u2pl_wgrad_set_tr", tr)
        assert _query("u2pl_conv_get_split") == split
        assert _query("u2pl_wgrad_h_eligible", 128, 128) == int(bool(split and tr))
        assert _query("u2pl_wgrad_h_eligible", 64, 128) == 0

    def restore(self):
        _query("u2pl_conv_set_split", self.old[0])
        _query("u2pl_wgrad_set_tr", self.old[1])


@pytest.fixture()
def switches():
    s = Switches()
    try:
        yield s
    finally:
        s.restore()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=R.F32)).to(DEV)


def _nan(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)


def _sentinel(n):
    return torch.full((n * 4,), 0xA5, dtype=torch.uint8, device=DEV).view(torch.float32)


def _intact(t):
    return bool((t.view(torch.int32) == torch.tensor(0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=DEV)).all())


def launch(g, pad, choice, plan, arith, dy, lddy, x, ldx, g_obj=None, x_obj=None, prev=None, shift=0):
    """one direct weight-gradient call with every per-launch check -> dw [Cout][R][S][Cin] float32 (numpy).
    arith picks the entry point; shift: floats between a 256-byte boundary and dw"""
    taps = g.R * g.S
    ns, wsz = plan[1], g.Cout * taps * g.Cin
    assert _query("u2pl_conv2d_wgrad_workspace_bytes", g.N, g.Hout, g.Wout, g.Cin, g.Cout, g.R, g.S) >= ns * wsz * 4
    ws = _nan(ns * wsz + MARGIN)
    buf = _sentinel(MARGIN + wsz + MARGIN + 4)
    assert buf.data_ptr() % 256 == 0
    off = MARGIN + shift
    dw = buf[off:off + wsz]
    assert dw.data_ptr() % 256 == 4 * shift
    if prev is not None:
        dw.copy_(_dev(prev).reshape(-1))
    geo = (g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout, g.R, g.S, g.mul, pad, g.step)
    acc = int(prev is not None)
    if arith == "h":
        _call("u2pl_conv2d_wgrad_h_f32", dy, lddy, g_obj, x, ldx, x_obj, dw, ws, acc, *geo)
    elif arith == "bf16op":
        _call("u2pl_conv2d_wgrad_bf16op_f32", dy, lddy, x, ldx, dw, ws, acc, *geo)
    else:
        _call("u2pl_conv2d_wgrad_f32", dy, lddy, x, ldx, dw, ws, acc, *geo)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[ns * wsz:]).all()), "wrote behind the last slab"
    assert not bool(torch.isnan(ws[:ns * wsz]).any()), "a slab element was not written"
    assert _intact(buf[:off]) and _intact(buf[off + wsz:]), "wrote outside dw"
    return dw.cpu().numpy().reshape(g.Cout, g.R, g.S, g.Cin)


@functools.lru_cache(maxsize=None)
def _case(name, pair):
    g, pad, dy, x = R.case_operands(name, pair)
    return g, pad, dy, x


@functools.lru_cache(maxsize=None)
def _ref(name, pair, arith):
    g, pad, dy, x = _case(name, pair)
    ref, bound = R.case_ref(name, pair, arith, dy, x)
    cap = R.case_ref(name, pair, "six", dy, x)[1] if arith == "fp32" else None
    return ref, bound, cap


def _plan(name, pair, state, bf16op=False, bn=0):
    """the kernel and slab plan of a case under a switch state, asserted against the library and against the edge the case is named
    for -> (Geo, pad, Choice, plan)"""
    arith, split, tr, h = state
    g, pad, _, _ = _case(name, pair)
    Cin, Cout = pair
    taps, M = g.R * g.S, g.N * g.Hout * g.Wout
    choice = R.kernel_choice(Cin, Cout, split, tr, h, R.is_pointwise(g), bf16op, bn)
    plan = R.plan_for(choice, M, Cin, Cout, taps)
    assert _query("u2pl_wgrad_batched_splits", M, Cin, Cout, taps) == plan[1], (name, pair, state)
    assert plan[0] == R.cdiv(Cin, choice.BN) and (plan[1] - 1) * plan[2] + plan[3] == R.cdiv(M, R.BK)
    one_tile = max(pair) <= 128
    if choice.family == "k_wgrad_tr":
        assert plan[1:] == R.EDGE[name], (name, pair, plan)
    elif choice.family != "k_wgrad_tr" and one_tile and name in R.EDGE_CONV:
        assert plan[1:] == R.EDGE_CONV[name], (name, pair, plan)
    want = "k_wgrad_tr" if (split and tr and pair in R.WIDE and not bf16op) else "k_conv_wgrad_bf16" if (split or bf16op) else "k_conv_wgrad"
    assert choice.family == want and choice.NP == {"h": 2, "six": 3}.get("bf16op" if bf16op else arith, 1)
    assert choice.PW == (choice.family == "k_wgrad_tr" and GEOM_PW[name])
    return g, pad, choice, plan


GEOM_PW = {name: (k == 1 and stride == 1) for name, (_, _, _, k, stride, _) in R.GEOMS.items()}


def _held(tag, family, got, ref, bound, cap=None):
    e = R.excess(got, ref, bound)
    print("excess %-40s %-28s %.3f" % (tag, family, e))
    _note(family, e)
    if cap is not None:                     # the fp32 matrix instruction against the 64-unit cap: a record, not an assertion
        ec = R.excess(got, ref, cap)
        print("       over the 64-unit cap %.3f" % ec)
        _note(family + " / 64-unit cap", ec)
    assert e <= 1.0, (tag, family, e)
    return e


def run_case(name, pair, state, pitch=False, bf16op=False, bn=0):
    """dense (or pitched) operands of one table case under one switch state: twice (the second time 16 bytes past alignment) with the
    same bits, then accumulate = 1"""
    arith = "bf16op" if bf16op else state[0]
    g, pad, choice, plan = _plan(name, pair, state, bf16op, bn)
    _, _, dy, x = _case(name, pair)
    lddy, ldx = (g.Cout + 24, g.Cin + 40) if pitch else (g.Cout, g.Cin)
    dyd, xd = _dev(R.pitched(dy, lddy)), _dev(R.pitched(x, ldx))
    objs = (_dev(R.amax_obj(np.abs(dy).max())), _dev(R.amax_obj(np.abs(x).max()))) if arith == "h" else (None, None)
    ref, bound, cap = _ref(name, pair, arith)
    family = "%s %s" % (choice.family, arith)
    tag = "%s %dx%d %s%s" % (name, pair[0], pair[1], choice.tmpl, " pitched" if pitch else "")
    got = launch(g, pad, choice, plan, arith, dyd, lddy, xd, ldx, *objs)
    _held(tag, family, got, ref, bound, cap)
    assert float(np.abs(got).max()) > 0
    if name == "dil12":                     # eight taps lie outside the map for every pixel
        outside = np.ones((3, 3), dtype=bool)
        outside[1, 1] = False
        assert (bound.numpy()[:, outside] == 0).all() and (got[:, outside] == 0).all()
    again = launch(g, pad, choice, plan, arith, dyd, lddy, xd, ldx, *objs, shift=4)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "the second call must give the same bits"
    prev = (np.random.default_rng(5).standard_normal(ref.shape) * float(ref.abs().mean())).astype(R.F32)
    pv = torch.from_numpy(prev.astype(np.float64))
    got = launch(g, pad, choice, plan, arith, dyd, lddy, xd, ldx, *objs, prev=prev)
    _held(tag + " accumulate", family + " accumulate", got, pv + ref, bound + R.EPS * (pv.abs() + ref.abs()))


TABLE = [(n, p, s) for n, p in R.cases() for s in R.states(p)]
_ID = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize("name,pair,state", TABLE, ids=["%s-%dx%d-%s-tr%d" % (n, p[0], p[1], s[0], s[2]) for n, p, s in TABLE])
def test_every_edge_under_every_switch_state(switches, name, pair, state):
    switches.set(state[1], state[2])
    run_case(name, pair, state)


PITCH_TABLE = [(n, p, s) for n in R.PITCHED for p in ((128, 128), (260, 132), (68, 20)) for s in R.states(p)]


@pytest.mark.parametrize("name,pair,state", PITCH_TABLE, ids=["%s-%dx%d-%s-tr%d" % (n, p[0], p[1], s[0], s[2]) for n, p, s in PITCH_TABLE])
def test_pitched_operands_with_nan_in_the_gap(switches, name, pair, state):
    """dy with lddy = Cout + 24 and x with ldx = Cin + 40: slices of wider buffers, NaN in the gap and behind the last pixel"""
    switches.set(state[1], state[2])
    run_case(name, pair, state, pitch=True)


@pytest.mark.parametrize("name,pair", R.BF16OP, ids=["%s-%dx%d" % (n, p[0], p[1]) for n, p in R.BF16OP])
def test_bf16_rounded_operands(switches, name, pair):
    switches.set(1, 0)
    run_case(name, pair, ("six", 1, 0, 0), bf16op=True)
    run_case(name, pair, ("six", 1, 0, 0), bf16op=True, pitch=True)


# ---- the maxima of the h form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pair", [("nk3", (128, 128)), ("g3x3", (260, 132))], ids=["nk3-128x128", "g3x3-260x132"])
def test_maxima_of_the_h_form(switches, name, pair):
    state = ("h", 1, 1, 1)
    switches.set(1, 1)
    g, pad, choice, plan = _plan(name, pair, state)
    _, _, dy, x = _case(name, pair)
    family, tag = "k_wgrad_tr h", "%s %dx%d" % (name, pair[0], pair[1])

    def go(dy_, x_, gm, xm, shard=None):
        return launch(g, pad, choice, plan, "h", _dev(dy_), g.Cout, _dev(x_), g.Cin, _dev(R.amax_obj(gm, shard)), _dev(R.amax_obj(xm, shard)))
    gm, xm = float(np.abs(dy).max()), float(np.abs(x).max())
    ref, bound, _ = _ref(name, pair, "h")
    base = go(dy, x, gm, xm)
    # the true maximum in shard 63 alone: the same scale, the same bits
    got = go(dy, x, gm, xm, shard=63)
    _held(tag + " maximum in shard 63", family, got, ref, bound)
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    # an upper bound 2^8 above the truth: the floor of the bound uses the value handed over
    ref8, bound8 = R.case_ref(name, pair, "h", dy, x, gm * 256, xm * 256)
    _held(tag + " maxima 2^8 above", family, go(dy, x, gm * 256, xm * 256), ref8, bound8)
    # all zero with zero maxima
    got = go(np.zeros_like(dy), np.zeros_like(x), 0.0, 0.0)
    assert np.isfinite(got).all() and (got == 0).all()
    # dy at 1e-30, x at 1e4
    dys, xs = (dy * R.F32(1e-30)).astype(R.F32), (x * R.F32(1e4)).astype(R.F32)
    refs, bounds = R.case_ref(name, pair, "h", dys, xs)
    got = go(dys, xs, float(np.abs(dys).max()), float(np.abs(xs).max()))
    _held(tag + " dy 1e-30, x 1e4", family, got, refs, bounds)
    assert float(np.abs(got).max()) > 0


# ---- the batched form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["h", "six"])
@pytest.mark.parametrize("pair", [(128, 128), (260, 132)], ids=_ID)
@pytest.mark.parametrize("M", [5, 32, 81, 1330])
@pytest.mark.parametrize("batch", [16, 36])
def test_batched_form(switches, batch, M, pair, arith):
    """per component and slab against its own float64 product, and the slab sum against the whole; components zdy / zx apart with NaN
    between them"""
    switches.set(1, 1)
    Cin, Cout = pair
    choice = R.kernel_choice(Cin, Cout, 1, 1, arith == "h", True)
    ct, ns, cps, last = R.plan_for(choice, M, Cin, Cout, batch)
    assert _query("u2pl_wgrad_batched_splits", M, Cin, Cout, batch) == ns and choice.family == "k_wgrad_tr" and choice.PW
    assert _query("u2pl_wgrad_batched_workspace_bytes", M, Cin, Cout, batch) == ns * Cout * batch * Cin * 4
    assert (ns, cps, last) == (1, R.cdiv(M, R.BK), R.cdiv(M, R.BK)) if M <= 81 else ns >= 3     # one slab of 1 / 1 / 3 chunks; several slabs
    dY = R.rows("six_decade_rows", batch * M, Cout, 11 + M).reshape(batch, M, Cout)
    X = R.rows("relu_heavy_tail", batch * M, Cin, 12 + M).reshape(batch, M, Cin)
    gm, xm = float(np.abs(dY).max()), float(np.abs(X).max())
    lddy, ldx = Cout + 8, Cin + 4
    zdy, zx = M * lddy + 72, M * ldx + 36
    dyb, xb = (np.full(batch * z, np.nan, dtype=R.F32) for z in (zdy, zx))
    for z in range(batch):
        dyb[z * zdy:z * zdy + M * lddy].reshape(M, lddy)[:, :Cout] = dY[z]
        xb[z * zx:z * zx + M * ldx].reshape(M, ldx)[:, :Cin] = X[z]
    n = ns * Cout * batch * Cin
    parts = []
    for _ in range(2):
        part = _nan(n + MARGIN)
        if arith == "h":
            _call("u2pl_wgrad_batched_h_f32", _dev(dyb), lddy, zdy, _dev(R.amax_obj(gm)), _dev(xb), ldx, zx, _dev(R.amax_obj(xm)), part, M, Cin,
                  Cout, batch)
        else:
            _call("u2pl_wgrad_batched_f32", _dev(dyb), lddy, zdy, _dev(xb), ldx, zx, part, M, Cin, Cout, batch)
        torch.cuda.synchronize()
        assert bool(torch.isnan(part[n:]).all()), "wrote behind the last slab"
        parts.append(part[:n].cpu().numpy().reshape(ns, Cout, batch, Cin))
    got = parts[0]
    assert np.array_equal(got.view(np.uint32), parts[1].view(np.uint32))
    assert not np.isnan(got).any(), "a slab element was not written"
    ref, bound = R.batched_ref(dY, X, M, batch, ns, cps, gm, xm, arith)
    family = "k_wgrad_tr %s batched" % arith
    _held("batch %d M %d %dx%d slabs" % (batch, M, Cin, Cout), family, got, ref, bound)
    _held("batch %d M %d %dx%d slab sum" % (batch, M, Cin, Cout), family, got.astype(np.float64).sum(0), ref.sum(0), bound.sum(0))


# ---- the forced tile width: one fresh child process ----------------------------------------------------------------------------------
CHILD_CASES = ("nk3", "ns9", "g3x3", "g3x3_s2", "ns16_short")


def _bn_probe():
    """(M, taps) at which the plan of (260, 132) differs between the forced 128-wide tile and the default: shows the library read it"""
    for M in range(6 * 32, 40000, 32 * 7):
        a, b = R.wgrad_tr_plan(M, 260, 132, 36, bn=128), R.wgrad_tr_plan(M, 260, 132, 36)
        if a[1] != b[1]:
            return M, 36, a[1]
    raise AssertionError("no probe")


def _child():
    assert os.environ.get("U2PL_WT_BN") == "128"
    sw = Switches()
    try:
        sw.set(1, 1)
        M, taps, ns = _bn_probe()
        assert _query("u2pl_wgrad_batched_splits", M, 260, 132, taps) == ns, "U2PL_WT_BN=128 was not read"
        for name in CHILD_CASES:
            for state in (("h", 1, 1, 1), ("six", 1, 1, 0)):
                g, pad, choice, plan = _plan(name, (260, 132), state, bn=128)
                assert choice.BN == 128 and plan[0] == 3                    # TN = 1 with three column tiles, the last 4 wide
                run_case(name, (260, 132), state, bn=128)
                run_case(name, (260, 132), state, pitch=True, bn=128)
    finally:
        sw.restore()
    print("RECORD " + json.dumps(WORST))


def test_forced_tile_width_in_a_fresh_process():
    """U2PL_WT_BN is read once per process: TN = 1 with several column tiles at Cin = 260"""
    env = dict(os.environ, PYTHONPATH=ROOT, U2PL_WT_BN="128")
    env.pop("U2PL_WGRAD_RECORD", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORD ")][-1][7:])
    assert rec and all(v <= 1.0 for v in rec.values())
    for fam, e in rec.items():
        _note(fam + " (TN = 1, three column tiles)", e)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    _child()
