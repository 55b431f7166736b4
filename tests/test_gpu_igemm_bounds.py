"""-m gpu: k_conv_igemm through the C ABI, element-wise against float64, at every tile, loop, gather and pitch edge.

Entry points: u2pl_conv2d_fwd_f32, _fwd_bnstats_f32, _fwd_bnact_f32, _dgrad_f32, the three _bf16op_ forms, u2pl_gemm_batched_f32, and on
their own u2pl_weight_transpose_f32 and u2pl_im2col_f32 (bit for bit).  The table of edges, the reference, the bound per arithmetic and
the planner restatement live in tests/igemm_ref.py; tests/test_igemm_cpu.py shows on an emulation that the bounds reject a kernel that
drops a guard, a chunk, a piece product, a pitch or a statistics slot.  Before every launch the restated planner's block count is
asserted against u2pl_conv2d_fwd_stat_blocks, so a case cannot silently run another kernel; the (TM, TN, WM, BF) expected per launch
is printed.  On every launch: NaN in the gaps of x and behind it, a sentinel in the gaps of y, in front of it and in three rows behind it,
two sentinel blocks behind the statistics partials.  Each test prints its excess (pytest -s); U2PL_IGEMM_RECORD=path writes the worst
|got - f64| / bound per (entry, arithmetic, tile shape) as JSON (profiles/igemm_bounds.json is one such run: a record, not a threshold)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import igemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
WAVES = 4 if os.environ.get("U2PL_IGEMM_WAVES", "").strip() == "4" else 8


def _call(name, *args):
    from u2pl_amd._lib import call
    call(name, *args)


def _query(name, *args):
    from u2pl_amd._lib import query
    return query(name, *args)


def _note(key, e):
    WORST[key] = max(WORST.get(key, 0.0), e)


@pytest.fixture(scope="module", autouse=True)
def _records():
    yield
    for key in sorted(WORST):
        print("worst  %-72s %.3f" % (key, WORST[key]))
    path = os.environ.get("U2PL_IGEMM_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({k: round(v, 4) for k, v in sorted(WORST.items())}, f, indent=1)
            f.write("\n")


class State:
    """u2pl_conv_set_split and U2PL_IGEMM_TAIL (read by the planner on every call), set and verified; restore() puts both back"""
    def __init__(self):
        self.split, self.tail = _query("u2pl_conv_get_split"), os.environ.get("U2PL_IGEMM_TAIL")

    def set(self, split, tail):
        _query("u2pl_conv_set_split", split)
        assert _query("u2pl_conv_get_split") == split
        if tail is None:
            os.environ.pop("U2PL_IGEMM_TAIL", None)
        else:
            os.environ["U2PL_IGEMM_TAIL"] = tail

    def restore(self):
        self.set(self.split, self.tail)


@pytest.fixture()
def state():
    s = State()
    try:
        yield s
    finally:
        s.restore()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=R.F32)).to(DEV)


def _held(tag, key, got_excess, cap=None):
    print("excess %-44s %-36s %.3f" % (tag, key, got_excess))
    _note(key, got_excess)
    if cap is not None:                     # the fp32 instruction against the 64-unit cap: a record, not an assertion
        print("       over the 64-unit cap %.3f" % cap)
        _note(key + " / 64-unit cap", cap)
    assert got_excess <= 1.0, (tag, key, got_excess)


@functools.lru_cache(maxsize=None)
def _data(r):
    d = R.run_data(r)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref(r, arith):
    d = _data(r)
    return R.product_ref(r.case, r.ncol, d["A"], d["W"], arith)


def _planned(state, r, arith, tail="table"):
    """switches set; the restated launches, asserted against the library's block count -> launches"""
    split, bf = R.state_of(arith)
    if tail == "table":
        tail = R.SHAPES[r.shape][0] if r.shape else None
    state.set(split, tail)
    g = R.geo(r.case, r.ncol)
    ls = R.run_igemm(R.rows_out(g), r.ncol, split, bf, tail, WAVES)
    assert _query("u2pl_conv2d_fwd_stat_blocks", g.N, g.Hout, g.Wout, g.Cout) == R.stat_blocks(ls), (R.run_id(r), arith, ls)
    print("expect %-44s %s" % (R.run_id(r), " + ".join(R.shape_of(l) for l in ls)))
    return ls


def _weights(r, d):
    """the weight operand on the device; the data gradient's goes through u2pl_weight_transpose_f32, checked bit for bit"""
    if r.case.kind == "fwd":
        return _dev(d["W"].reshape(-1))
    taps = r.case.k ** 2
    layer = np.ascontiguousarray(d["W"].transpose(2, 1, 0))                 # [Cout = C][taps][Cin = ncol]
    wt = torch.full((r.ncol * taps * r.case.C + 8,), float("nan"), device=DEV)
    _call("u2pl_weight_transpose_f32", _dev(layer.reshape(-1)), wt, r.case.C, taps, r.ncol)
    torch.cuda.synchronize()
    assert np.array_equal(wt[:-8].cpu().numpy().view(np.uint32), d["W"].reshape(-1).view(np.uint32)) and bool(torch.isnan(wt[-8:]).all())
    return wt


def launch(state, r, arith, entry="fwd", tail="table", pivot=True, res=True, ldr_extra=0, relu=1):
    """one run through its entry point with every per-launch check; entry: fwd (the data gradient for a dgrad case) | stats | bnact"""
    d, c = _data(r), r.case
    g, M, K = d["g"], d["M"], d["g"].R * d["g"].S * d["g"].Cin
    ls = _planned(state, r, arith, tail)
    ref, cond = _ref(r, arith)
    v, bv = R.y_ref_bound(ref, cond, K, arith, d["bias"])
    x, w, bias = _dev(d["x"]), _weights(r, d), _dev(d["bias"])
    ybuf = _dev(d["y"])
    y = ybuf[r.yshift:]
    assert ybuf.data_ptr() % 256 == 0
    sfx = "_bf16op_f32" if arith == "bf16op" else "_f32"
    geom = (c.N, c.H, c.W, c.C, g.Hout, g.Wout, r.ncol, c.k, c.k, c.stride, c.pad, c.dil)
    nstat, st = R.stat_blocks(ls), None
    if c.kind == "dgrad":
        assert entry == "fwd" and bias is None
        Ho, Wo = g.Hin, g.Win
        _call("u2pl_conv2d_dgrad" + sfx, x, d["ldx"], w, y, d["ldy"], c.N, c.H, c.W, r.ncol, Ho, Wo, c.C, c.k, c.k, c.stride, c.pad, c.dil)
    elif entry == "fwd":
        _call("u2pl_conv2d_fwd" + sfx, x, d["ldx"], w, bias, y, d["ldy"], *geom)
    elif entry == "stats":
        piv = (np.random.default_rng(3).standard_normal(r.ncol) * 0.3).astype(R.F32) if pivot else None
        st = torch.full(((nstat + 2) * 2 * r.ncol,), float(R.SENT), device=DEV)
        _call("u2pl_conv2d_fwd_bnstats" + sfx, x, d["ldx"], w, bias, y, d["ldy"], *geom, _dev(piv), st)
    else:
        epi = R.bn_params(r.ncol, M, ldr_extra, 17, res, relu)
        _call("u2pl_conv2d_fwd_bnact_f32", x, d["ldx"], w, bias, y, d["ldy"], *geom, _dev(epi.mean), _dev(epi.invstd), _dev(epi.gamma), _dev(epi.beta),
              _dev(epi.res), epi.ldr, relu)
        rs = None if epi.res is None else R.unpitch(epi.res, M, r.ncol, epi.ldr)
        v, bv = R.bnact_ref_bound(v, bv, epi.mean, epi.invstd, epi.gamma, epi.beta, rs, relu)
    torch.cuda.synchronize()
    yflat = ybuf.cpu().numpy()
    assert R.outside_intact(yflat, M, r.ncol, d["ldy"], r.yshift), "wrote outside the output"
    got = R.unpitch(yflat, M, r.ncol, d["ldy"], r.yshift)
    what = {"fwd": c.kind, "stats": "fwd_bnstats", "bnact": "fwd_bnact"}[entry]
    key = "%s %s %s" % (what, arith, " + ".join(R.shape_of(l) for l in ls))
    cap = R.excess(got, v, R.cap_bound(cond) + (0 if d["bias"] is None else R.EPS * np.abs(v))) if (arith == "fp32" and entry != "bnact") else None
    _held(R.run_id(r), key, R.excess(got, v, bv), cap)
    if entry != "bnact" and (bv == 0).any():                    # every tap outside the map: the bias, or exactly zero
        assert np.array_equal(got[bv == 0], v[bv == 0].astype(R.F32))
    if st is not None:
        s = st.cpu().numpy().reshape(nstat + 2, 2, r.ncol)
        assert (s[nstat:] == R.SENT).all(), "wrote behind the last statistics block"
        sref, sb = R.stats_ref_bound(v, R.product_bound(cond, K, arith), d["bias"], piv, ls)
        _held(R.run_id(r) + " partials", key + " partials", R.excess(s[:nstat], sref, sb))
    return got


RUNS = R.runs()


@pytest.mark.parametrize("r", RUNS, ids=[R.run_id(r) for r in RUNS])
def test_every_edge_in_every_arithmetic(state, r):
    """each run of the table forced onto its tile shape, in the six-product form, with the fp32 instruction and with bf16 operands: the
    plain entry point, and for a forward case the one with fused statistics (pivot and bias)"""
    for arith in R.ARITHS:
        a = launch(state, r, arith)
        if r.case.kind == "fwd":
            b = launch(state, r, arith, "stats")
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the statistics entry must store the same y"


@pytest.mark.parametrize("arith,split,tail", R.BODY_TAIL_STATES, ids=[s[0] for s in R.BODY_TAIL_STATES])
def test_body_and_tail_launch_together(state, arith, split, tail):
    """Cout = 1024 on one 65 x 65 image: 32 body blocks and a 129-row tail on <1, 1, 2>, its partials from slot 32"""
    r = R.BODY_TAIL_RUN
    assert R.state_of(arith)[0] == split
    ls = R.run_launches(r, arith, tail, WAVES)
    assert [(l.m0, l.m1, l.slot, l.BM) for l in ls] == [(0, 4096, 0, 128), (4096, 4225, 32, 64)]
    launch(state, r, arith, "fwd", tail=tail)
    launch(state, r, arith, "stats", tail=tail)
    launch(state, r, arith, "stats", tail=tail, pivot=False)


EDGE_RUNS = [next(r for r in RUNS if r.shape == shape and r.case.name == "rows%d" % (BM + 1)) for shape, (_, BM, _, _) in R.SHAPES.items()]


@pytest.mark.parametrize("r", EDGE_RUNS, ids=[R.run_id(r) for r in EDGE_RUNS])
def test_eval_batchnorm_epilogue_and_null_pivot(state, r):
    """u2pl_conv2d_fwd_bnact_f32 with bias on every tile shape, one row past a tile: residual dense and pitched, with and without ReLU, no
    residual; and the statistics with a null pivot, the last row block holding one row"""
    assert r.bias and r.ncol % 4 == 0
    for arith in ("six", "fp32"):
        launch(state, r, arith, "bnact", res=True, relu=1)
        launch(state, r, arith, "bnact", res=True, relu=0, ldr_extra=4)
        launch(state, r, arith, "bnact", res=False, relu=1)
        launch(state, r, arith, "bnact", res=False, relu=0)
    for arith in R.ARITHS:
        launch(state, r, arith, "stats", pivot=False)


@pytest.mark.parametrize("arith", ["six", "fp32"])
@pytest.mark.parametrize("batch,M,K,Nn", R.BATCHED, ids=["b%d-m%d-k%d-n%d" % b for b in R.BATCHED])
def test_batched_products(state, batch, M, K, Nn, arith):
    """u2pl_gemm_batched_f32: the components zx / zw / zy apart with NaN (x, w) and a sentinel (y) between them"""
    split, _ = R.state_of(arith)
    state.set(split, None)
    ls = R.run_igemm(M, Nn, split, False, None, WAVES, batch)
    print("expect batch %d M %d K %d Nn %d: %s" % (batch, M, K, Nn, " + ".join(R.shape_of(l) for l in ls)))
    rng = np.random.default_rng(batch + K + Nn)
    X = rng.standard_normal((batch, M, K)).astype(R.F32)
    W = (rng.standard_normal((batch, Nn, K)) / np.sqrt(K)).astype(R.F32)
    ldx, ldy = K + 4, Nn + 4
    zx, zw, zy = M * ldx + 40, Nn * K + 24, M * ldy + 12
    xb, wb = np.full(batch * zx, np.nan, dtype=R.F32), np.full(batch * zw, np.nan, dtype=R.F32)
    mask = np.ones(batch * zy, dtype=bool)
    for z in range(batch):
        xb[z * zx:z * zx + M * ldx].reshape(M, ldx)[:, :K] = X[z]
        wb[z * zw:z * zw + Nn * K] = W[z].reshape(-1)
        mask[z * zy:z * zy + M * ldy].reshape(M, ldy)[:, :Nn] = False
    y = torch.full((batch * zy,), float(R.SENT), device=DEV)
    _call("u2pl_gemm_batched_f32", _dev(xb), ldx, zx, _dev(wb), zw, y, ldy, zy, M, K, Nn, batch)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    assert (yh[mask] == R.SENT).all(), "wrote outside the outputs"
    got = np.stack([yh[z * zy:z * zy + M * ldy].reshape(M, ldy)[:, :Nn] for z in range(batch)])
    ref, cond = R.gemm_ref(X, W, arith)
    _held("batch %d M %d K %d Nn %d" % (batch, M, K, Nn), "gemm_batched %s %s" % (arith, " + ".join(R.shape_of(l) for l in ls)),
          R.excess(got, ref, R.product_bound(cond, K, arith)))


@pytest.mark.parametrize("Cout,Cin,RS", [(37, 50, 1), (37, 50, 9), (68, 20, 9), (33, 31, 1), (1, 65, 9)])
def test_weight_transpose_bit_for_bit(Cout, Cin, RS):
    w = np.random.default_rng(Cout + Cin + RS).standard_normal((Cout, RS, Cin)).astype(R.F32)
    wt = torch.full((Cout * RS * Cin + 16,), float(R.SENT), device=DEV)
    _call("u2pl_weight_transpose_f32", _dev(w.reshape(-1)), wt, Cout, RS, Cin)
    torch.cuda.synchronize()
    h = wt.cpu().numpy()
    assert np.array_equal(h[:-16].view(np.uint32), np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(-1).view(np.uint32))
    assert (h[-16:] == R.SENT).all()


def _im2col_ref(x, N, H, W, C, k, stride, pad, Kp):
    Ho, Wo = R.out_size(H, k, stride, pad, 1), R.out_size(W, k, stride, pad, 1)
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), dtype=R.F32)
    xp[:, pad:pad + H, pad:pad + W] = x
    col = np.zeros((N, Ho, Wo, Kp), dtype=R.F32)
    for r in range(k):
        for s in range(k):
            col[..., (r * k + s) * C:(r * k + s + 1) * C] = xp[:, r:r + stride * Ho:stride, s:s + stride * Wo:stride][:, :Ho, :Wo]
    return col.reshape(-1, Kp), Ho, Wo


@pytest.mark.parametrize("N,H,W,k,pad,ldx", [(2, 9, 7, 3, 1, 3), (2, 9, 7, 3, 1, 5), (1, 11, 13, 7, 3, 3), (2, 15, 9, 7, 3, 8), (2, 459, 459, 7, 3, 3)],
                         ids=["3x3", "3x3-ldx5", "7x7", "7x7-ldx8", "7x7-past-the-grid-stride"])
def test_im2col_bit_for_bit(N, H, W, k, pad, ldx):
    """the stem's patch matrix: Cin = 3 at stride 2 on odd maps, the padding to Kp exactly zero, NaN in the gaps of a pitched x; the last
    case has more elements than the grid has threads"""
    C, stride = 3, 2
    Kp = R.cdiv(k * k * C, 32) * 32
    x = np.random.default_rng(H + k + ldx).standard_normal((N, H, W, C)).astype(R.F32)
    ref, Ho, Wo = _im2col_ref(x, N, H, W, C, k, stride, pad, Kp)
    total = N * Ho * Wo * Kp
    assert (total > 65536 * 256) == (H == 459)
    col = torch.full((total + 64,), float(R.SENT), device=DEV)
    _call("u2pl_im2col_f32", _dev(R.pitched(x.reshape(-1, C), ldx)), ldx, col, Kp, N, H, W, C, Ho, Wo, k, k, stride, pad, 1)
    torch.cuda.synchronize()
    h = col.cpu().numpy()
    assert np.array_equal(h[:total].view(np.uint32), ref.reshape(-1).view(np.uint32)) and (h[total:] == R.SENT).all()
    assert (ref[:, k * k * C:] == 0).all() and float(np.abs(ref).max()) > 0


# ---- the four-wave body: one fresh child process -------------------------------------------------------------------------------------
CHILD_RUNS = ("rows129-68-124-bias", "cols129-132-124-bias", "nk5-68-124")


def _child():
    assert WAVES == 4
    s = State()
    try:
        for rid in CHILD_RUNS:
            r = next(q for q in RUNS if R.run_id(q) == rid)
            for arith in ("six", "fp32"):
                ls = R.run_launches(r, arith, "0", 4)
                assert [(l.TM, l.TN, l.WM) for l in ls] == [(2, 2, 2)]
                launch(s, r, arith, "fwd", tail="0")
                launch(s, r, arith, "stats", tail="0")
        for arith, split, tail in R.BODY_TAIL_STATES[:2]:
            launch(s, R.BODY_TAIL_RUN, arith, "stats", tail=tail)
    finally:
        s.restore()
    print("RECORD " + json.dumps(WORST))


def test_four_wave_body_in_a_fresh_process():
    """U2PL_IGEMM_WAVES is read once per process: the <2, 2, 2> body with the fp32 instruction and in the six-product form"""
    env = dict(os.environ, PYTHONPATH=ROOT, U2PL_IGEMM_WAVES="4")
    env.pop("U2PL_IGEMM_RECORD", None)
    env.pop("U2PL_IGEMM_TAIL", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORD ")][-1][7:])
    assert rec and all(v <= 1.0 for k, v in rec.items() if "64-unit cap" not in k)
    assert any("<2, 2, 2, 0>" in k for k in rec) and any("<2, 2, 2, 3>" in k for k in rec)
    for key, e in rec.items():
        _note(key + " (U2PL_IGEMM_WAVES=4)", e)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--child"]
    _child()
