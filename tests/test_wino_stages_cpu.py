"""The stage contract of tests/wino_stage_ref.py, checked against itself on the CPU: the faithful fp32 emulation of every Winograd
transform kernel meets its stage bound against the float64 reference on every case of the GPU test's shape list (excess <= 1; the
largest excess per stage is printed and recorded in DESIGN.md), and every faulty emulation -- two precision faults and seven
geometry / bookkeeping faults -- is rejected by the bound at a case named here.  The two precision faults are what shows that a
bound is tight enough to see a transform that is merely sloppy: each stage bound rejects them on the heavy-tail data kind (rounding
G's constants to bf16 applies to the two stages that use them at F(4x4): the filter transform and the weight-gradient finish; at
F(2x2) G's constants are exact in bf16)."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as BB  # noqa: E402
import wino_stage_ref as R  # noqa: E402

F32 = np.float32


# ---- one function per stage: (case, kind, fault) -> excess of the emulation over the stage bound -------------------------------------
def _seed(*k):
    return zlib.crc32(repr(k).encode())


def input_excess(case, mt, kind, fault=None):
    N, H, W, C, dil = case
    x = R.rows(kind, N * H * W, C, _seed("in", case, mt))
    ref, bound = R.ref_input(x, N, H, W, C, dil, mt)
    return R.stage_excess(R.emu_input(x, N, H, W, C, dil, mt, fault), ref, bound)


def gy_excess(case, mt, kind, fault=None):
    N, H, W, C, dil = case
    g = R.rows(kind, N * H * W, C, _seed("gy", case, mt))
    ref, bound = R.ref_gy(g, N, H, W, C, dil, mt)
    return R.stage_excess(R.emu_gy(g, N, H, W, C, dil, mt, fault), ref, bound)


def weight_excess(shape, mt, transposed, fault=None):
    O, C = shape
    w = R.weights((O, 3, 3, C), 5 + O)
    ref, bound = R.ref_weight(w, transposed, mt)
    return R.stage_excess(R.emu_weight(w, transposed, mt, fault), ref, bound)


def _epilogue(N, H, W, O, seed):
    rng = np.random.default_rng(seed)
    bn = (rng.standard_normal(O), 0.5 + rng.random(O), rng.standard_normal(O), 50.0 * rng.standard_normal(O))
    return [v.astype(F32) for v in bn], rng.standard_normal((N * H * W, O)).astype(F32), rng.standard_normal(O).astype(F32)


def output_excess(case, mt, kind, mode, fault=None):
    """mode: plain | bias | bn (bias + eval BatchNorm + residual + ReLU)"""
    N, H, W, O, dil = case
    a2, tiles = (mt + 2) ** 2, R.geom(N, H, W, dil, mt)[2]
    Mb = R.rows(kind, a2 * tiles, O, _seed("out", case, mt)).reshape(a2, tiles, O)
    bn, res, bias = _epilogue(N, H, W, O, 3)
    kw = {} if mode == "plain" else {"bias": bias} if mode == "bias" else {"bias": bias, "bn": bn, "res": res, "relu": 1}
    ref, bound = R.ref_output(Mb, N, H, W, O, dil, mt, **kw)
    got = R.emu_output(Mb, N, H, W, O, dil, mt, fault=fault, **kw)
    if got.shape[0] != ref.shape[0]:                # a faulty variant that writes behind the last pixel: those rows are not written
        pad = got.shape[0] - ref.shape[0]
        ref, bound = (np.concatenate([v, np.zeros((pad, O))]) for v in (ref, bound))
        return R.stage_excess(got, ref, bound, np.arange(got.shape[0])[:, None].repeat(O, 1) < N * H * W)
    return R.stage_excess(got, ref, bound)


def stats_excess(case, pivot_on):
    N, H, W, O, dil, mt = case
    a2, tiles = (mt + 2) ** 2, R.geom(N, H, W, dil, mt)[2]
    Mb = R.rows("relu_heavy_tail", a2 * tiles, O, _seed("st", case)).reshape(a2, tiles, O)
    pivot = np.random.default_rng(4).standard_normal(O).astype(F32) if pivot_on else None
    y, part = R.emu_output(Mb, N, H, W, O, dil, mt, stats=True, pivot=pivot)
    assert part.shape[0] == -(-tiles // BB.wino_tpb(O))
    ref, bound = R.ref_stats(y, pivot, N, H, W, O, dil, mt, BB.L_wino(mt, O))
    return R.stage_excess(part, ref, bound)


def finish_excess(shape, mt, nsplit, accumulate, fault=None):
    O, C = shape
    a2 = (mt + 2) ** 2
    part = R.rows("relu_heavy_tail", nsplit * O * a2, C, _seed("fin", shape, mt, nsplit)).reshape(nsplit, O, a2, C)
    part = part * np.where(np.random.default_rng(8).random(part.shape) < 0.5, F32(-1), F32(1))
    dw0 = R.weights((O, 3, 3, C), 9) * F32(100) if accumulate else None
    ref, bound = R.ref_finish(part, mt, dw0)
    return R.stage_excess(R.emu_finish(part, mt, accumulate, dw0, fault), ref, bound)


# ---- the faithful emulation ------------------------------------------------------------------------------------------------------
def test_faithful_emulation_meets_every_stage_bound():
    worst = {}

    def note(stage, e, what):
        assert e <= 1.0, (stage, what, e)
        worst[stage] = max(worst.get(stage, 0.0), e)

    for mt in R.MTS:
        for case in R.GEOMS:
            for kind in R.KINDS:
                note("input F(%dx%d)" % (mt, mt), input_excess(case, mt, kind), (case, kind))
                note("gy F(%dx%d)" % (mt, mt), gy_excess(case, mt, kind), (case, kind))
                for mode in ("plain", "bias", "bn"):
                    note("output F(%dx%d) %s" % (mt, mt, mode), output_excess(case, mt, kind, mode), (case, kind))
        for shape in R.WEIGHT_SHAPES:
            for tr in (0, 1):
                note("filter F(%dx%d)" % (mt, mt), weight_excess(shape, mt, tr), (shape, tr))
        for shape in R.FINISH_SHAPES:
            for ns in R.NSPLITS:
                for acc in (0, 1):
                    note("finish F(%dx%d)" % (mt, mt), finish_excess(shape, mt, ns, acc), (shape, ns, acc))
    for case in R.STAT_CASES:
        for pv in (False, True):
            note("statistics", stats_excess(case, pv), (case, pv))
    for stage in sorted(worst):
        print("largest excess  %-24s %.3f" % (stage, worst[stage]))


# ---- the faulty emulations: (fault, stage function, arguments of the NAMED case that must reject it) --------------------------------
HT = "relu_heavy_tail"
G311 = (3, 9, 11, 64, 1)        # Ty = 5, Tx = 6 at mt = 2; the map ends inside the last tiles
G2D2 = (2, 9, 11, 20, 2)        # two phases per axis, sub-images 5 x 6 and 4 x 5
FAULTS = [
    # precision: every stage, heavy-tail data
    ("pass_bf16", input_excess, (G311, 4, HT)), ("pass_bf16", input_excess, (G311, 2, HT)),
    ("pass_bf16", gy_excess, (G311, 4, HT)), ("pass_bf16", gy_excess, (G311, 2, HT)),
    ("pass_bf16", output_excess, (G311, 4, HT, "plain")), ("pass_bf16", output_excess, (G311, 2, HT, "bn")),
    ("pass_bf16", weight_excess, ((96, 32), 4, 0)), ("pass_bf16", weight_excess, ((96, 32), 2, 1)),
    ("pass_bf16", finish_excess, ((64, 64), 4, 7, 1)), ("pass_bf16", finish_excess, ((64, 64), 2, 7, 1)),
    ("g_bf16", weight_excess, ((96, 32), 4, 0)), ("g_bf16", weight_excess, ((1, 1), 4, 1)),
    ("g_bf16", finish_excess, ((64, 64), 4, 7, 1)), ("g_bf16", finish_excess, ((1, 4), 4, 1, 0)),
    # geometry and bookkeeping
    ("edge_inside", input_excess, (G311, 4, HT)), ("edge_inside", gy_excess, (G311, 4, HT)),
    ("edge_inside", output_excess, (G311, 4, HT, "plain")),
    ("swap_phase", input_excess, (G2D2, 4, HT)), ("swap_phase", gy_excess, (G2D2, 2, HT)),
    ("swap_phase", output_excess, (G2D2, 4, HT, "bias")),
    ("ty_for_tx", input_excess, (G311, 2, HT)), ("ty_for_tx", gy_excess, ((2, 5, 13, 8, 1), 4, HT)),
    ("ty_for_tx", output_excess, ((2, 5, 13, 8, 1), 4, HT, "plain")),
    ("no_rotation", weight_excess, ((12, 20), 4, 1)), ("no_rotation", weight_excess, ((12, 20), 2, 1)),
    ("drop_last_slab", finish_excess, ((5, 20), 4, 2, 0)), ("drop_last_slab", finish_excess, ((5, 20), 2, 7, 1)),
    ("no_accumulate", finish_excess, ((5, 20), 4, 1, 1)), ("no_accumulate", finish_excess, ((64, 64), 2, 2, 1)),
    ("bias_outside", output_excess, (G311, 4, HT, "bias")), ("bias_outside", output_excess, ((1, 1, 1, 4, 1), 2, HT, "bias")),
    ("bias_outside", output_excess, (G2D2, 2, HT, "bn")),
]


@pytest.mark.parametrize("fault,fn,args", FAULTS, ids=["%s-%s-%d" % (f, fn.__name__, i) for i, (f, fn, _) in enumerate(FAULTS)])
def test_faulty_emulation_is_rejected(fault, fn, args):
    assert fn(*args) <= 1.0                         # the named case passes without the fault ...
    assert fn(*args, fault=fault) > 1.0             # ... and the bound sees the fault


@pytest.mark.parametrize("mt", R.MTS)
def test_precision_faults_are_rejected_at_every_heavy_tail_case(mt):
    """not only at the named cases: one pass rounded to bf16 fails every stage on every listed geometry with heavy-tail data"""
    for case in R.GEOMS:
        for fn in (input_excess, gy_excess):
            assert fn(case, mt, HT, fault="pass_bf16") > 1.0, (fn.__name__, case)
        assert output_excess(case, mt, HT, "plain", fault="pass_bf16") > 1.0, case
    for shape in R.WEIGHT_SHAPES:
        assert weight_excess(shape, mt, 0, fault="pass_bf16") > 1.0, shape
        if mt == 4:
            assert weight_excess(shape, mt, 0, fault="g_bf16") > 1.0, shape
    for shape in R.FINISH_SHAPES:
        assert finish_excess(shape, mt, 2, 0, fault="pass_bf16") > 1.0, shape
        if mt == 4:
            assert finish_excess(shape, mt, 2, 0, fault="g_bf16") > 1.0, shape
