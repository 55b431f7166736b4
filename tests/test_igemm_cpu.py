"""The contract of tests/igemm_ref.py, checked on the CPU: the restated planner against the library's in every switch state, the plan
and the launches agreeing for every arithmetic, the refusals of the implicit-GEMM entry points (none reaches a launch), the fp32
emulation of k_conv_igemm within its bound on every run of the GPU table (tests/test_gpu_igemm_bounds.py), and every switchable fault
rejected at a named case -- a fault that no case rejects means a case is missing from the table."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import igemm_ref as R  # noqa: E402

EINVAL = 1001
COUTS = (20, 64, 65, 68, 128, 132, 256, 1024, 2048)


def _grid(Cout):
    """row counts across the first two 256-block round boundaries of this column count, and a coarse sweep"""
    nt = R.cdiv(Cout, 128)
    out = set(range(1, 70000, 397)) | {1, 63, 64, 65, 127, 128, 129, 261}
    for rounds in (1, 2):
        edge = rounds * R.NUM_CUS // nt * 128
        out |= {edge + q for q in (-129, -128, -1, 0, 1, 63, 64, 65, 127, 128, 129, 130, 257)}
    return sorted(m for m in out if m > 0)


# ---- the planner --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from u2pl_amd._lib import lib
    return lib().cdll


@pytest.fixture()
def split(L):
    old = L.u2pl_conv_get_split()
    try:
        yield L.u2pl_conv_set_split
    finally:
        L.u2pl_conv_set_split(old)


@pytest.mark.parametrize("tail", R.TAILS, ids=[str(t) for t in R.TAILS])
@pytest.mark.parametrize("on", [1, 0])
def test_library_planner_against_the_restatement(L, split, monkeypatch, on, tail):
    """u2pl_conv2d_fwd_stat_blocks = nblk_body + nblk_tail of the restated plan; plan_igemm reads U2PL_IGEMM_TAIL on every call"""
    split(on)
    assert L.u2pl_conv_get_split() == on
    if tail is None:
        monkeypatch.delenv("U2PL_IGEMM_TAIL", raising=False)
    else:
        monkeypatch.setenv("U2PL_IGEMM_TAIL", tail)
    for Cout in COUTS:
        for M in _grid(Cout):
            p = R.plan_igemm(M, Cout, on, tail)
            N = 2 if M % 2 == 0 else 1
            assert L.u2pl_conv2d_fwd_stat_blocks(N, 1, M // N, Cout) == p.nblk_body + p.nblk_tail, (M, Cout, on, tail, p)


def test_plan_and_launches_agree_in_every_arithmetic():
    """the launches cover the rows exactly once, and their row blocks are the plan's statistic blocks -- for bf16 operands too (the
    128 x 64 tail of U2PL_IGEMM_TAIL=14 once ran as 64-row blocks there: twice the partial blocks the plan had counted)"""
    seen = set()
    for on in (1, 0):
        for tail in R.TAILS:
            for bf in (False, True):
                for Cout in COUTS:
                    for M in _grid(Cout):
                        p = R.plan_igemm(M, Cout, on, tail)
                        ls = R.run_igemm(M, Cout, on, bf, tail)
                        assert R.stat_blocks(ls) == p.nblk_body + p.nblk_tail, (M, Cout, on, tail, bf)
                        assert ls[0].m0 == 0 and ls[-1].m1 == M and all(a.m1 == b.m0 for a, b in zip(ls, ls[1:]))
                        assert all(l.slot == (0 if l.m0 == 0 else p.nblk_body) for l in ls)
                        assert all(l.m0 % 128 == 0 for l in ls)
                        seen |= {(l.TM, l.TN, l.WM, l.BF) for l in ls}
    for waves_bf in (0, 3):
        seen |= {(l.TM, l.TN, l.WM, l.BF) for l in R.run_igemm(1000, 128, waves_bf == 3, False, "0", waves=4)}
    assert len(seen) == 18 and {s[:3] for s in seen} == set(R.SHAPES)        # six shapes x three arithmetics


def test_the_table_names_its_edges():
    p = R.plan_igemm(65 * 65, 1024, 0)
    assert p == R.Plan(4096, 1, 1, 32, 3)                                      # 32 body blocks and a 129-row tail on <1, 1, 2>
    for arith, on, tail in R.BODY_TAIL_STATES:
        ls = R.run_launches(R.BODY_TAIL_RUN, arith, tail)
        assert [(l.TM, l.TN, l.WM, l.m0, l.m1, l.slot) for l in ls] == [(1, 2, 4, 0, 4096, 0), (1, 1, 2, 4096, 4225, 32)] and R.stat_blocks(ls) == 35
    assert len(R.run_launches(R.BODY_TAIL_RUN, "six")) == 1                    # the split form's default: no tail
    ids = [R.run_id(r) for r in R.runs()]
    assert len(set(ids)) == len(ids)
    reached = set()
    for r in R.runs():
        g = R.geo(r.case, r.ncol)
        _, BM, BN, couts = R.SHAPES[r.shape]
        for arith in R.ARITHS:
            ls = R.run_launches(r, arith)
            assert len(ls) == 1 and (ls[0].TM, ls[0].TN, ls[0].WM) == r.shape and (ls[0].BM, ls[0].BN) == (BM, BN), (R.run_id(r), arith)
            reached.add(R.shape_of(ls[0]))
        assert g.Cin % 32 == 0
    assert len(reached) == 18
    for shape, (_, BM, BN, couts) in R.SHAPES.items():
        Ms = {R.rows_out(R.geo(r.case, r.ncol)) for r in R.runs() if r.shape == shape and r.case.name.startswith("rows")}
        assert Ms == {1, BM - 1, BM, BM + 1, 2 * BM + 5}
        assert any(c % BN == 4 for c in couts if c > 64) or shape == (2, 1, 2)  # a last column tile 4 wide
    assert {c.name: R.k_schedule(c.C * c.k ** 2 // 32, False) for c in R.KLOOP}["nk5"] == [0, 1, 2, 3, 4]
    d = R.geo(R.CASES["dil6_5x7"], 20)
    assert (d.Hout, d.Wout) == (5, 7) and d.step == 6                           # every off-centre tap outside the map
    assert R.geo(R.CASES["d_s2_1x1"], 20).log2div == 1 and R.geo(R.CASES["d_s4"], 20).log2div == 2


def test_schedules_multiply_every_chunk_once_in_order():
    for nk in range(1, 12):
        for single in (False, True):
            assert R.k_schedule(nk, single) == list(range(nk))
            if nk % 2:
                assert R.k_schedule(nk, single, "skip_last_odd_chunk") == list(range(nk - 1))
            if nk >= 4:
                assert R.k_schedule(nk, single, "stale_prefetch") != list(range(nk))


# ---- refusals: U2PL_EINVAL (or 0 for an empty problem) before any launch -----------------------------------------------------------
def test_refusals(L, split):
    geom = (2, 5, 7, 32, 5, 7, 20, 3, 3, 1, 1, 1)                   # N Hin Win Cin Hout Wout Cout R S stride pad dil
    bad_cin = (2, 5, 7, 48, 5, 7, 20, 3, 3, 1, 1, 1)
    one = 1                                                        # a non-null pointer that no call below dereferences
    for on in (1, 0):
        split(on)
        assert L.u2pl_conv2d_fwd_f32(None, 48, None, None, None, 20, *bad_cin, None) == EINVAL
        assert L.u2pl_conv2d_fwd_bf16op_f32(None, 48, None, None, None, 20, *bad_cin, None) == EINVAL
        assert L.u2pl_conv2d_fwd_bnstats_f32(None, 48, None, None, None, 20, *bad_cin, None, None, None) == EINVAL
        assert L.u2pl_conv2d_fwd_bnstats_bf16op_f32(None, 48, None, None, None, 20, *bad_cin, None, None, None) == EINVAL
        assert L.u2pl_conv2d_fwd_bnact_f32(None, 48, None, None, None, 20, *bad_cin, one, one, one, one, None, 0, 1, None) == EINVAL
        assert L.u2pl_gemm_batched_f32(None, 48, 0, None, 0, None, 20, 0, 70, 48, 20, 16, None) == EINVAL
        for fn in (L.u2pl_conv2d_dgrad_f32, L.u2pl_conv2d_dgrad_bf16op_f32):
            for stride in (3, 5, 6):                               # not a power of two
                assert fn(None, 32, None, None, 20, 2, 9, 7, 20, 3, 3, 32, 3, 3, stride, 1, 1, None) == EINVAL, stride
            assert fn(None, 48, None, None, 20, 2, 9, 7, 20, 5, 4, 48, 3, 3, 2, 1, 1, None) == EINVAL        # the reduction (Cout) % 32
        bn = (one, one, one, one)
        assert L.u2pl_conv2d_fwd_bnact_f32(None, 32, None, None, None, 18, *geom[:6], 18, *geom[7:], *bn, None, 0, 1, None) == EINVAL   # Cout % 4
        assert L.u2pl_conv2d_fwd_bnact_f32(None, 32, None, None, None, 20, *geom, *bn, one, 22, 1, None) == EINVAL                    # ldr % 4
        for miss in range(4):
            args = [one] * 4
            args[miss] = None
            assert L.u2pl_conv2d_fwd_bnact_f32(None, 32, None, None, None, 20, *geom, *args, None, 0, 1, None) == EINVAL, miss
        for M, batch in ((0, 16), (-5, 16), (70, 0), (70, -1)):
            assert L.u2pl_gemm_batched_f32(None, 32, 0, None, 0, None, 20, 0, M, 32, 20, batch, None) == 0
        # operand extents of 2^31 bytes or more: refused in front of the launch line
        big = 2 ** 31 // (4 * 69) + 2
        assert (70 - 1) * big * 4 >= 2 ** 31
        assert L.u2pl_conv2d_fwd_f32(None, big, None, None, None, 20, *geom, None) == EINVAL
        assert L.u2pl_gemm_batched_f32(None, big, 0, None, 0, None, 20, 0, 70, 32, 20, 16, None) == EINVAL


# ---- the emulation ----------------------------------------------------------------------------------------------------------------
RUNS = {R.run_id(r): r for r in R.runs()}


@functools.lru_cache(maxsize=None)
def _data(rid):
    r = RUNS[rid] if rid != "body_tail" else R.BODY_TAIL_RUN
    d = R.run_data(r)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r, d


@functools.lru_cache(maxsize=None)
def _ref(rid, arith):
    r, d = _data(rid)
    return R.product_ref(r.case, r.ncol, d["A"], d["W"], arith)


def emu_excess(rid, arith, entry="fwd", fault=None, tail="table", pivot=True, res=True, ldr_extra=0, relu=1):
    """largest excess of the (faulty) emulation of one run over its bounds: the output (inf where something outside it changed), and for
    entry = stats every partial block"""
    r, d = _data(rid)
    g, K = d["g"], d["g"].R * d["g"].S * d["g"].Cin
    ls = R.run_launches(r, arith, tail)
    ref, cond = _ref(rid, arith)
    v, bv = R.y_ref_bound(ref, cond, K, arith, d["bias"])
    piv = (np.random.default_rng(3).standard_normal(r.ncol) * 0.3).astype(R.F32) if (entry == "stats" and pivot) else None
    epi = R.bn_params(r.ncol, d["M"], ldr_extra, 17, res, relu) if entry == "bnact" else None
    y, st, info = R.emulate(d["x"], d["ldx"], d["W"].reshape(-1), g, ls, d["y"], d["ldy"], r.yshift, d["bias"], entry == "stats", piv, epi=epi,
                            fault=fault)
    if epi is not None:
        rs = None if epi.res is None else R.unpitch(epi.res, d["M"], r.ncol, epi.ldr)
        v, bv = R.bnact_ref_bound(v, bv, epi.mean, epi.invstd, epi.gamma, epi.beta, rs, relu)
    e = R.held(d, r, y, v, bv)
    if fault is None and (bv == 0).any():                       # every tap outside: the bias, or exactly zero
        got = R.unpitch(y, d["M"], r.ncol, d["ldy"], r.yshift)
        assert np.array_equal(got[bv == 0], v[bv == 0].astype(R.F32))
    if entry == "stats":
        sref, sb = R.stats_ref_bound(v, R.product_bound(cond, K, arith), d["bias"], piv, ls)
        e = max(e, R.excess(st, sref, sb))
    return e, info


def test_faithful_emulation_meets_its_bound_on_every_run():
    worst = {}
    for rid, r in RUNS.items():
        for arith in R.ARITHS:
            e, info = emu_excess(rid, arith, "stats")
            assert e <= 1.0, (rid, arith, e)
            key = "%s %s" % (arith, info["shapes"][0])
            worst[key] = max(worst.get(key, 0.0), e)
            if r.ldy_extra % 4 or r.yshift % 4 or r.ncol % 4:
                assert info["scalar"], rid
    assert len(worst) == 18
    for key in sorted(worst):
        print("largest excess  %-28s %.3f" % (key, worst[key]))


def test_epilogues_and_both_launches_hold_in_emulation():
    for shape, (_, BM, BN, couts) in R.SHAPES.items():
        rid = "rows%d-%d-%d%d%d%s" % ((BM + 1, couts[0]) + shape + ("-bias",))
        for arith in ("six", "fp32"):
            for kw in (dict(res=True, relu=1), dict(res=True, relu=0, ldr_extra=4), dict(res=False, relu=1)):
                e, _ = emu_excess(rid, arith, "bnact", **kw)
                assert e <= 1.0, (rid, arith, kw, e)
            assert emu_excess(rid, arith, "stats", pivot=False)[0] <= 1.0
    for arith, on, tail in R.BODY_TAIL_STATES:
        e, info = emu_excess("body_tail", arith, "stats", tail=tail)
        assert e <= 1.0 and len(info["shapes"]) == 2, (arith, e)


def _batched(batch, M, K, Nn, arith, fault=None):
    rng = np.random.default_rng(batch + K + Nn)
    X = rng.standard_normal((batch, M, K)).astype(R.F32)
    W = (rng.standard_normal((batch, Nn, K)) / np.sqrt(K)).astype(R.F32)
    ldx, ldy = K + 4, Nn + 4
    zx, zw, zy = M * ldx + 40, Nn * K + 24, M * ldy + 12
    xb, wb = np.full(batch * zx, np.nan, dtype=R.F32), np.full(batch * zw, np.nan, dtype=R.F32)
    for z in range(batch):
        xb[z * zx:z * zx + M * ldx].reshape(M, ldx)[:, :K] = X[z]
        wb[z * zw:z * zw + Nn * K] = W[z].reshape(-1)
    yb = np.full(batch * zy, R.SENT, dtype=R.F32)
    split, bf = R.state_of(arith)
    ls = R.run_igemm(M, Nn, split, bf, None, batch=batch)
    y, _, _ = R.emulate(xb, ldx, wb, R.gemm_geo(M, K, Nn), ls, yb, ldy, batch=batch, zx=zx, zw=zw, zy=zy, fault=fault)
    ref, cond = R.gemm_ref(X, W, arith)
    got = np.stack([y[z * zy:z * zy + M * ldy].reshape(M, ldy)[:, :Nn] for z in range(batch)])
    mask = np.ones(y.shape, dtype=bool)
    for z in range(batch):
        mask[z * zy:z * zy + M * ldy].reshape(M, ldy)[:, :Nn] = False
    if not (y[mask] == R.SENT).all():
        return float("inf")
    return R.excess(got, ref, R.product_bound(cond, K, arith))


def test_batched_products_hold_in_emulation():
    for batch, M, K, Nn in R.BATCHED:
        for arith in ("six", "fp32"):
            assert _batched(batch, M, K, Nn, arith) <= 1.0, (batch, K, Nn, arith)


# fault -> the named runs that reject it: (run id, arithmetic, entry, keywords)
PITCH8 = "pad1-68-124-ldx8-ldy8-bias"
NAMED = [
    ("unmasked_rows", ("rows129-68-124-bias", "six", "fwd", {})), ("unmasked_rows", ("rows65-68-112-bias", "fp32", "fwd", {})),
    ("no_parity", ("d_s2_3x3-20-212", "six", "fwd", {})), ("no_parity", ("d_s2_1x1-68-122", "fp32", "fwd", {})),
    ("no_upper_limit", ("pad1-20-212", "six", "fwd", {})), ("no_upper_limit", ("d_s2_3x3_even-68-122", "bf16op", "fwd", {})),
    ("swap_rs", ("pad1-20-212", "fp32", "fwd", {})), ("swap_rs", ("s2_odd-68-122-bias", "six", "fwd", {})),
    ("stride_as_dil", ("dil2-20-212-bias", "six", "fwd", {})), ("stride_as_dil", ("s2_even-68-122", "fp32", "fwd", {})),
    ("skip_last_odd_chunk", ("nk3-20-212", "six", "fwd", {})), ("skip_last_odd_chunk", ("nk1-68-124", "fp32", "fwd", {})),
    ("skip_last_odd_chunk", ("nk5-132-112", "bf16op", "fwd", {})),
    ("stale_prefetch", ("nk4-20-212", "six", "fwd", {})), ("stale_prefetch", ("nk5-68-124", "six", "fwd", {})),
    ("stale_prefetch", ("nk3-68-124", "fp32", "fwd", {})), ("stale_prefetch", ("k3x3_c32-132-112", "bf16op", "fwd", {})),
    ("bias_past_cout", ("cols129-132-124-bias", "six", "fwd", {})), ("bias_past_cout", ("cols129-19-212-bias", "fp32", "fwd", {})),
    ("store_past_cout", (PITCH8, "six", "fwd", {})), ("store_past_cout", ("pad1-68-124-ldx4-ldy3-bias", "fp32", "fwd", {})),
    ("ldy_ignored", (PITCH8, "six", "fwd", {})), ("ldx_ignored", (PITCH8, "fp32", "fwd", {})),
    ("ldx_ignored", ("d_s2_3x3-128-112-ldx40-ldy24", "six", "fwd", {})),
    ("stats_rows_unmasked", ("rows129-68-124-bias", "six", "stats", {})), ("stats_rows_unmasked", ("rows65-68-112-bias", "fp32", "stats", dict(pivot=False))),
    ("stats_tail_at_zero", ("body_tail", "fp32", "stats", {})), ("stats_tail_at_zero", ("body_tail", "six", "stats", dict(tail="-1"))),
    ("stats_without_bias", ("rows129-68-124-bias", "six", "stats", {})), ("stats_without_bias", ("rows127-20-212-bias", "fp32", "stats", {})),
    ("relu_before_residual", ("rows129-68-124-bias", "six", "bnact", {})), ("relu_before_residual", ("rows129-20-212-bias", "fp32", "bnact", {})),
    ("drop_piece", ("nk2-20-212", "six", "fwd", {})), ("drop_piece", ("pad1-68-122", "six", "fwd", {})),
    ("bf16_once", ("nk2-20-212", "six", "fwd", {})), ("bf16_once", ("rows129-68-124-bias", "six", "fwd", {})),
]


def test_every_fault_has_a_named_case():
    assert {f for f, _ in NAMED} | {"batch_stride_ignored"} == set(R.FAULTS)


@pytest.mark.parametrize("fault,case", NAMED, ids=["%s-%s-%s-%d" % (f, c[0], c[1], i) for i, (f, c) in enumerate(NAMED)])
def test_faulty_emulation_is_rejected(fault, case):
    rid, arith, entry, kw = case
    assert emu_excess(rid, arith, entry, **kw)[0] <= 1.0                   # the named run passes without the fault ...
    assert emu_excess(rid, arith, entry, fault=fault, **kw)[0] > 1.0       # ... and the bound sees the fault


def test_ignored_batch_strides_are_rejected():
    assert _batched(16, 70, 32, 20, "six") <= 1.0 and _batched(16, 70, 32, 20, "six", "batch_stride_ignored") > 1.0
    assert _batched(36, 70, 96, 68, "fp32") <= 1.0 and _batched(36, 70, 96, 68, "fp32", "batch_stride_ignored") > 1.0
