"""The contract of tests/wgrad_ref.py, checked on the CPU: the slab planners' invariants, the library's planners and switches against
the restatement, the refusals of the weight-gradient entry points (no launch is reachable from them), the fp32 emulation of the kernels
within its bound on every case of the GPU table (tests/test_gpu_wgrad_bounds.py), and every switchable fault rejected at a named case
-- a fault that no case rejects means a case is missing from the table."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

EINVAL = 1001
TRIPLES = [(128, 128, 1), (2048, 256, 9), (132, 260, 1), (64, 64, 9), (4, 4, 1), (256, 256, 36)]       # (Cin, Cout, taps)
SWEEP = range(1, 40001, 7)


# ---- planners -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout,taps", TRIPLES)
def test_planner_sweep(Cin, Cout, taps):
    for M in SWEEP:
        nchunks = R.cdiv(M, R.BK)
        for which, (ct, ns, cps, last) in (("tr", R.wgrad_tr_plan(M, Cin, Cout, taps)), ("conv", R.wgrad_plan(M, Cin, Cout, taps))):
            assert ns >= 1 and cps >= 1 and 1 <= last <= cps, (which, M)                    # every slab has at least one chunk
            assert (ns - 1) * cps + last == nchunks, (which, M)                             # the slabs cover the chunks exactly
            assert cps == R.cdiv(nchunks, ns), (which, M)
            assert ct >= 1
            if which == "tr":
                assert ns <= 96, M


def test_the_table_names_its_edges():
    """every geometry of the table is the edge it is named for under the restated planners"""
    for name, (N, H, W, k, stride, dil) in R.GEOMS.items():
        g, _ = R.conv_geo(N, H, W, 128, 128, k, stride, dil)
        M = g.N * g.Hout * g.Wout
        assert R.wgrad_tr_plan(M, 128, 128, k * k)[1:] == R.EDGE[name], name
        if name in R.EDGE_CONV:
            assert R.wgrad_plan(M, 128, 128, k * k)[1:] == R.EDGE_CONV[name], name
    assert R.conv_geo(*R.GEOMS["m25"][:3], 128, 128, 1, 1, 1)[0].Hout * 5 == 25
    assert R.wgrad_tr_plan(3420, 260, 132, 1)[0] == 2 and R.wgrad_tr_plan(3420, 260, 132, 1, bn=128)[0] == 3
    assert not R.is_pointwise(R.conv_geo(*R.GEOMS["pw_s2"][:3], 128, 128, 1, 2, 1)[0])      # 1x1 at stride 2: the gather kernel
    assert R.is_pointwise(R.conv_geo(*R.GEOMS["nk3"][:3], 128, 128, 1, 1, 1)[0])
    fam = {(R.kernel_choice(ci, co, 1, 0, 0).BM, R.kernel_choice(ci, co, 1, 0, 0).BN) for ci, co in R.NARROW}
    assert fam == {(64, 64), (128, 64), (64, 128)} and R.kernel_choice(128, 128, 1, 0, 0).tmpl == "<2, 2, 3>"
    assert R.kernel_choice(128, 128, 0, 1, 0).tmpl == "<1, 2, 4>" and R.kernel_choice(260, 132, 1, 1, 1, True).tmpl == "<2, true, 2>"


# ---- the library against the restatement -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from u2pl_amd._lib import lib
    return lib().cdll


@pytest.fixture()
def switches(L):
    """-> set(split, tr); both switches restored afterwards"""
    old_split, old_tr = L.u2pl_conv_get_split(), L.u2pl_wgrad_set_tr(1)
    L.u2pl_wgrad_set_tr(old_tr)

    def set_(split, tr):
        L.u2pl_conv_set_split(split)
        L.u2pl_wgrad_set_tr(tr)
    try:
        yield set_
    finally:
        L.u2pl_conv_set_split(old_split)
        L.u2pl_wgrad_set_tr(old_tr)


def _restated(M, Cin, Cout, taps, split, tr):
    bn = int(os.environ.get("U2PL_WT_BN") or 0)                                 # (a forced tile width changes the plan's tile count)
    return R.plan_for(R.kernel_choice(Cin, Cout, split, tr, 0, bn=bn), M, Cin, Cout, taps)


@pytest.mark.parametrize("split,tr", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_library_planners_against_the_restatement(L, switches, split, tr):
    switches(split, tr)
    assert L.u2pl_conv_get_split() == split
    for Cin, Cout, taps in TRIPLES:
        assert L.u2pl_wgrad_h_eligible(Cin, Cout) == int(bool(split) and R.tr_eligible(Cin, Cout, tr))
        for M in SWEEP:
            ns = _restated(M, Cin, Cout, taps, split, tr)[1]
            assert L.u2pl_wgrad_batched_splits(M, Cin, Cout, taps) == ns, (M, Cin, Cout, taps)
    # the workspace query covers the plan in force (it is asked before the arithmetic switch may change: the larger of the two plans)
    for Cin, Cout, taps in TRIPLES:
        k = {1: 1, 9: 3, 36: 6}[taps]
        for N, Ho, Wo in ((1, 1, 1), (1, 5, 5), (1, 18, 21), (1, 57, 60), (2, 65, 65), (4, 129, 129)):
            ns = _restated(N * Ho * Wo, Cin, Cout, taps, split, tr)[1]
            assert L.u2pl_conv2d_wgrad_workspace_bytes(N, Ho, Wo, Cin, Cout, k, k) >= ns * Cout * taps * Cin * 4, (N, Ho, Wo, Cin, Cout)
    for Cin, Cout, want in ((128, 128, 1), (124, 128, 0), (128, 124, 0), (130, 128, 0), (128, 130, 0), (132, 260, 1), (64, 256, 0)):
        assert L.u2pl_wgrad_h_eligible(Cin, Cout) == int(want and split and tr), (Cin, Cout)


# ---- refusals: U2PL_EINVAL before any launch ---------------------------------------------------------------------------------------
def _direct(L, form, Cin, Cout, lddy=None, ldx=None, gmax=None, xmax=None, geom=(1, 35, 38)):
    N, H, W = geom
    lddy, ldx = lddy or Cout, ldx or Cin
    tail = (None, None, 0, N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1, None)       # dw, workspace, accumulate, geometry, stream
    if form == "h":
        return L.u2pl_conv2d_wgrad_h_f32(None, lddy, gmax, None, ldx, xmax, *tail)
    fn = L.u2pl_conv2d_wgrad_f32 if form == "f32" else L.u2pl_conv2d_wgrad_bf16op_f32
    return fn(None, lddy, None, ldx, *tail)


def _batched(L, form, M, Cin, Cout, batch=16, lddy=None, ldx=None, gmax=None, xmax=None):
    lddy, ldx = lddy or Cout, ldx or Cin
    if form == "h":
        return L.u2pl_wgrad_batched_h_f32(None, lddy, M * lddy, gmax, None, ldx, M * ldx, xmax, None, M, Cin, Cout, batch, None)
    return L.u2pl_wgrad_batched_f32(None, lddy, M * lddy, None, ldx, M * ldx, None, M, Cin, Cout, batch, None)


def test_refusals(L, switches):
    obj = (ctypes.c_float * (R.AMAX_SHARDS * R.AMAX_STRIDE))()                  # never read: every call below returns before a launch
    mx = ctypes.addressof(obj)
    BIG = 404000                                                                # (1330 - 1) * 404000 * 4 bytes >= 2^31
    assert 1329 * BIG * 4 >= 2 ** 31
    for split, tr in ((1, 1), (1, 0), (0, 1), (0, 0)):
        switches(split, tr)
        for Cin, Cout in ((130, 128), (128, 130), (66, 64), (64, 18)):
            for form in ("f32", "bf16op", "h"):
                assert _direct(L, form, Cin, Cout, gmax=mx, xmax=mx) == EINVAL, (form, Cin, Cout)
            for form in ("f32", "h"):
                assert _batched(L, form, 81, Cin, Cout, gmax=mx, xmax=mx) == EINVAL, (form, Cin, Cout)
        for gmax, xmax in ((None, mx), (mx, None), (None, None)):               # a NULL maximum
            assert _direct(L, "h", 128, 128, gmax=gmax, xmax=xmax) == EINVAL
            assert _batched(L, "h", 81, 128, 128, gmax=gmax, xmax=xmax) == EINVAL
        for Cin, Cout in ((64, 64), (64, 128), (128, 64), (68, 20)) + (((128, 128), (260, 132)) if not (split and tr) else ()):
            assert _direct(L, "h", Cin, Cout, gmax=mx, xmax=mx) == EINVAL, (split, tr, Cin, Cout)      # not an eligible layer
            assert _batched(L, "h", 81, Cin, Cout, gmax=mx, xmax=mx) == EINVAL, (split, tr, Cin, Cout)
        for M in (0, -1, -1330):
            assert _batched(L, "f32", M, 128, 128) == EINVAL and _batched(L, "h", M, 128, 128, gmax=mx, xmax=mx) == EINVAL
        # operand extents of 2^31 bytes or more, at M = 1330
        for Cin, Cout in ((128, 128), (64, 64), (260, 132)):
            for kw in (dict(lddy=BIG), dict(ldx=BIG)):
                assert _direct(L, "f32", Cin, Cout, **kw) == EINVAL, (split, tr, Cin, Cout, kw)
                assert _direct(L, "bf16op", Cin, Cout, **kw) == EINVAL, (split, tr, Cin, Cout, kw)
                assert _batched(L, "f32", 1330, Cin, Cout, **kw) == EINVAL, (split, tr, Cin, Cout, kw)
                if split and tr and Cin >= 128:
                    assert _direct(L, "h", Cin, Cout, gmax=mx, xmax=mx, **kw) == EINVAL
                    assert _batched(L, "h", 1330, Cin, Cout, gmax=mx, xmax=mx, **kw) == EINVAL


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(name, pair):
    g, pad, dy, x = R.case_operands(name, pair)
    for a in (dy, x):
        a.setflags(write=False)
    return g, dy, x


def emu_excess(name, pair, state, pitch=False, accumulate=0, amax="true", bf16op=False, scale=None, fault=None):
    """excess of the (faulty) emulation of one case over its bound.  state: (arith, split, tr, h) of wgrad_ref.states; pitch: dy / x as
    slices of wider buffers with NaN in the gap and behind; amax: true | shard63 | upper (2^8 above the truth)"""
    arith, split, tr, h = state
    g, dy, x = _data(name, pair)
    if scale:                                       # (dy, x) scaled: operands at the ends of the fp32 range
        dy, x = (dy * R.F32(scale[0])).astype(R.F32), (x * R.F32(scale[1])).astype(R.F32)
    ch = R.kernel_choice(pair[0], pair[1], split, tr, h, R.is_pointwise(g), bf16op)
    arith = "bf16op" if bf16op else arith
    plan = R.plan_for(ch, g.N * g.Hout * g.Wout, pair[0], pair[1], g.R * g.S)
    lddy, ldx = (g.Cout + 24, g.Cin + 40) if pitch else (g.Cout, g.Cin)
    gm, xm = float(np.abs(dy).max()), float(np.abs(x).max())
    if amax == "upper":
        gm, xm = gm * 256, xm * 256
    shard = 63 if amax == "shard63" else None
    prev = None
    if accumulate:
        ref0 = R.case_ref(name, pair, arith, dy, x)[0].numpy()
        prev = (np.random.default_rng(5).standard_normal(ref0.shape) * np.abs(ref0).mean()).astype(R.F32)
    ref, bound = R.case_ref(name, pair, arith, dy, x, gm, xm, prev)
    got = R.emulate(R.pitched(dy, lddy), lddy, R.pitched(x, ldx), ldx, g, plan, ch, arith, R.amax_obj(gm, shard), R.amax_obj(xm, shard),
                    prev, accumulate, fault=fault)
    if name == "dil12":                             # eight taps outside the map for every pixel: those rows exactly zero
        outside = np.ones((3, 3), dtype=bool)
        outside[1, 1] = False
        assert (bound.numpy()[:, outside] == 0).all()
        if fault is None:
            assert (got[:, outside] == 0).all()
    return R.excess(got, ref, bound)


def _family(pair, state, bf16op=False):
    arith, split, tr, h = state
    return "%s %s" % (R.kernel_choice(pair[0], pair[1], split, tr, h, bf16op=bf16op).family, "bf16op" if bf16op else arith)


def test_faithful_emulation_meets_its_bound_on_every_case():
    worst = {}
    for name, pair in R.cases():
        for state in R.states(pair):
            e = emu_excess(name, pair, state)
            assert e <= 1.0, (name, pair, state, e)
            fam = _family(pair, state)
            worst[fam] = max(worst.get(fam, 0.0), e)
    for name, pair in R.BF16OP:
        e = emu_excess(name, pair, R.states(pair)[-1], bf16op=True)
        assert e <= 1.0, (name, pair, e)
        worst[_family(pair, R.states(pair)[-1], True)] = max(worst.get(_family(pair, R.states(pair)[-1], True), 0.0), e)
    for fam in sorted(worst):
        print("largest excess  %-28s %.3f" % (fam, worst[fam]))
        assert worst[fam] < 0.7, (fam, worst[fam])      # the arithmetic alone leaves room under the bound at the largest M of the table


H, SIX, SIXC, FP32 = ("h", 1, 1, 1), ("six", 1, 1, 0), ("six", 1, 0, 0), ("fp32", 0, 0, 0)
FAULTS = [
    ("drop_last_slab", ("two_slabs", (128, 128), SIX), {}), ("drop_last_slab", ("ns9", (68, 20), SIXC), {}),
    ("skip_odd_tail", ("nk3", (128, 128), H), {}), ("skip_odd_tail", ("m25", (128, 128), SIX), {}),
    ("unmasked_rows", ("m25", (128, 128), SIX), dict(pitch=True)), ("unmasked_rows", ("g3x3", (64, 64), FP32), dict(pitch=True)),
    ("pitch_ignored", ("nk3", (132, 128), H), dict(pitch=True)), ("pitch_ignored", ("g3x3_s2", (128, 128), SIXC), dict(pitch=True)),
    ("swap_rs", ("g3x3", (128, 128), H), {}), ("swap_rs", ("g3x3_s2", (128, 128), SIX), {}),
    ("stride_as_dil", ("dil12", (128, 128), H), {}), ("stride_as_dil", ("g3x3_s2", (128, 128), SIXC), {}),
    ("store_ci_past", ("g3x3", (132, 128), SIX), {}), ("store_ci_past", ("nk3", (260, 132), H), {}), ("store_ci_past", ("g3x3", (68, 20), SIXC), {}),
    ("store_co_past", ("ns9", (260, 132), SIX), {}), ("store_co_past", ("ns9", (68, 20), SIXC), {}),
    ("no_accumulate", ("nk3", (128, 128), H), dict(accumulate=1)), ("no_accumulate", ("ns9", (64, 128), SIXC), dict(accumulate=1)),
    ("scale_back_dy", ("nk3", (128, 128), H), {}),
    ("amax_shard0", ("nk3", (128, 128), H), dict(amax="shard63")),
    ("drop_piece", ("ns9", (128, 128), H), {}), ("drop_piece", ("nk3", (128, 128), H), dict(amax="upper")),
    ("pass_bf16_once", ("ns9", (128, 128), SIX), {}), ("pass_bf16_once", ("g3x3", (32, 64), SIXC), {}),
]


def test_every_fault_has_a_named_case():
    assert {f for f, _, _ in FAULTS} == set(R.FAULTS)


@pytest.mark.parametrize("fault,case,kw", FAULTS, ids=["%s-%s-%dx%d-%d" % (f, c[0], c[1][0], c[1][1], i) for i, (f, c, _) in enumerate(FAULTS)])
def test_faulty_emulation_is_rejected(fault, case, kw):
    assert emu_excess(*case, **kw) <= 1.0                       # the named case passes without the fault ...
    assert emu_excess(*case, fault=fault, **kw) > 1.0           # ... and the bound sees the fault


def test_variants_of_the_gpu_test_hold_in_emulation():
    """the pitched, accumulating and amax variants the GPU test runs, on the faithful emulation"""
    for name in R.PITCHED:
        for pair in ((128, 128), (260, 132), (68, 20)):
            for state in R.states(pair):
                assert emu_excess(name, pair, state, pitch=True) <= 1.0, (name, pair, state)
    for amax in ("shard63", "upper"):
        assert emu_excess("nk3", (128, 128), H, amax=amax) <= 1.0
        assert emu_excess("g3x3", (260, 132), H, amax=amax, accumulate=1) <= 1.0
    for name, pair in (("nk3", (128, 128)), ("g3x3", (260, 132))):
        assert emu_excess(name, pair, H, scale=(1e-30, 1e4)) <= 1.0


def test_batched_reference_layout():
    """batched_ref's slabs add up to the whole product, and the emulation's slabs [nsplit][Cout][batch][Cin] meet them one by one"""
    M, batch, Cin, Cout = 1330, 4, 132, 128
    ct, ns, cps, last = R.wgrad_tr_plan(M, Cin, Cout, batch)
    dY = R.rows("six_decade_rows", batch * M, Cout, 3).reshape(batch, M, Cout)
    X = R.rows("relu_heavy_tail", batch * M, Cin, 4).reshape(batch, M, Cin)
    gm, xm = float(np.abs(dY).max()), float(np.abs(X).max())
    zdy, zx = M * Cout + 72, M * Cin + 8
    dyb, xb = (np.full(batch * z, np.nan, dtype=R.F32) for z in (zdy, zx))
    for z in range(batch):
        dyb[z * zdy:z * zdy + M * Cout] = dY[z].reshape(-1)
        xb[z * zx:z * zx + M * Cin] = X[z].reshape(-1)
    g = R.batched_geo(M, Cin, Cout, batch, zdy, zx)
    assert R.is_pointwise(g)
    for arith, h in (("h", 1), ("six", 0)):
        ref, bound = R.batched_ref(dY, X, M, batch, ns, cps, gm, xm, arith)
        whole = np.einsum("zmo,zmi->ozi", dY.astype(np.float64), X.astype(np.float64))
        assert np.abs(ref.sum(0) - whole).max() <= 1e-12 * np.abs(whole).max()
        ch = R.kernel_choice(Cin, Cout, 1, 1, h, True)
        got = R.emulate(dyb, Cout, xb, Cin, g, (ct, ns, cps, last), ch, arith, R.amax_obj(gm), R.amax_obj(xm), reduce=False)
        assert got.shape == ref.shape and R.excess(got, ref, bound) <= 1.0
