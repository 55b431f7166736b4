"""-m gpu: the exact selection (u2pl_amd/csrc/select.hip) against the sorted reference of tests/select_ref.py, bit for bit,
at every edge of the three-pass radix select, and the fused split (u2pl_amd/csrc/relfused.hip) at its route switch.

There is no tolerance anywhere in this file.  Every case is shared with tests/test_select_cpu.py, which proves on the
reference alone that the case reaches the edge it is named for (the table of edges and kernel lines is in that file's
header).  Per case the threshold words, the two selected values of every spec (SEL_VAL), the lerp weights (SEL_GAMMA), hist0
and the hist1 / hist2 rows of every leader are compared: a wrong histogram names the pass that went wrong (k_sel_hist0,
k_sel_pass<1>, k_sel_pass<2>), a wrong value with right histograms names resolve_level / k_sel_finish.  Rows of slots that
are not leaders are unspecified and not read.

Beyond the shared cases:
  layouts      a value pointer that is not 16-byte aligned (`n4 = 0` in k_sel_hist0 and k_sel_pass: every element on the scalar
               path), n % 4 = 0..3 (the scalar tail after the float4 loop), 262144 + 5 values (one full grid-stride trip of the
               256 x 256 x 4 launch plus a ragged tail)
  NaN contract a NaN of any sign and payload is not valid and moves no rank (sel_key in select.hip; f32_key would sort a NaN
               with the sign bit below -inf, into rank 0); n_valid = 0 gives a NaN threshold for pct and +inf for kth
  kth rule     k at 1, at the end of a tie run, at n_valid, n_valid + 1, 0, -3, above n_total; floors below / equal / above
  hand-over    hist0 accumulated by u2pl_entropy_f32 / u2pl_ohem_prob_f32 (hist0_done = 1) against k_sel_hist0 on the same tensor
  rejections   0 and 5 specs: U2PL_EINVAL, no launch, workspace untouched (`nspec < 1 || 2 * nspec > MAXS`)
  drop rule    u2pl_apply_drop_i64 with the threshold ON a tie value (`ent >= thr`), NaN pixels keep their label
  fused split  `ncand > RF_CAP` (relfused.hip, phase C) at RF_CAP - 1, RF_CAP, RF_CAP + 1 equal candidates, and a total above
               RF_CAP whose two lists each fit (`n <= RF_CAP` in the degenerate route's selection)

A threshold that is NaN by arithmetic (inf - inf between infinite neighbours) is compared as NaN, not by its bits: sign and
payload of an invalid operation's result belong to the arithmetic unit (0xffc00000 on x86, where the reference runs)."""
import numpy as np
import pytest
import torch

import select_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, u32 = np.float32, np.uint32


def hip():
    from u2pl_amd import hipops as H
    return H


def D(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def words(ws):
    return ws.cpu().numpy().view(u32)


def run_plain(vd, n_valid, specs):
    """u2pl_select_f32 on a plain value array (hist0_done = 0) -> the workspace words"""
    H = hip()
    ws = H.new_select_ws(DEV, vd.numel())
    ws[0] = int(n_valid)
    H.run_select(vd, ws, specs)
    return words(ws)


def result_words(w, nspec):
    return dict(thr=w[S.SEL_THR:S.SEL_THR + nspec], val=w[S.SEL_VAL:S.SEL_VAL + 2 * nspec], gamma=w[S.SEL_GAMMA:S.SEL_GAMMA + nspec])


def check_against_reference(tag, v, specs, w, n_valid=None):
    exp = S.expected(v, specs, n_valid)
    got = result_words(w, len(specs))
    lv = exp["levels"]
    tok, fig = S.describe(v, specs)
    print(tag, sorted(tok), fig, "specs", specs, "thr", [hex(x) for x in got["thr"]], "want", [hex(x) for x in exp["thr"]],
          "val", [hex(x) for x in got["val"]], "want", [hex(x) for x in exp["val"]])
    # histograms first: they localise a failure to a pass
    assert np.array_equal(w[S.SEL_H0:S.SEL_H0 + 2048], lv[0]["hist"][0]), (tag, "hist0")
    for l, h in lv[1]["hist"].items():
        assert np.array_equal(w[S.SEL_H1 + 2048 * l:S.SEL_H1 + 2048 * (l + 1)], h), (tag, "hist1", l)
    for l, h in lv[2]["hist"].items():
        assert np.array_equal(w[S.SEL_H2 + 1024 * l:S.SEL_H2 + 1024 * (l + 1)], h), (tag, "hist2", l)
    assert np.array_equal(got["val"], exp["val"]), (tag, "SEL_VAL")
    assert np.array_equal(got["gamma"], exp["gamma"]), (tag, "SEL_GAMMA")
    for j in range(len(specs)):
        if np.isnan(exp["thr"][j:j + 1].view(f32)[0]) and exp["thr"][j] != S.QNAN:      # NaN by arithmetic (file header)
            assert np.isnan(got["thr"][j:j + 1].view(f32)[0]), (tag, j)
        else:
            assert got["thr"][j] == exp["thr"][j], (tag, j, hex(got["thr"][j]), hex(exp["thr"][j]))
    return got


# ------------------------------------------------------------------ threshold, values, histograms
@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_select_equals_the_sorted_reference(case):
    v, specs = S.case_inputs(case)
    w = run_plain(D(v), int((~np.isnan(v)).sum()), specs)
    check_against_reference(case.id, v, specs, w)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("case", S.LAYOUT_CASES, ids=[c.id for c in S.LAYOUT_CASES])
def test_select_layouts_aligned_and_unaligned_pointer(case):
    v, specs = S.case_inputs(case)
    nv = int((~np.isnan(v)).sum())
    vd = D(v)
    assert vd.data_ptr() % 16 == 0
    w0 = run_plain(vd, nv, specs)
    got0 = check_against_reference(case.id, v, specs, w0)
    buf = torch.zeros(v.size + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(vd)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    w1 = run_plain(view, nv, specs)
    got1 = check_against_reference(case.id + "-unaligned", v, specs, w1)
    for k in got0:
        assert np.array_equal(got0[k], got1[k]), k


# ------------------------------------------------------------------ NaN contract
@pytest.mark.parametrize("pattern", S.NAN_PATTERNS, ids=[hex(p) for p in S.NAN_PATTERNS])
def test_nan_of_any_sign_and_payload_is_invalid_and_moves_no_rank(pattern):
    n = 4099
    fin = S.family("octaves", n, 11)
    rng = np.random.default_rng(pattern % 1000)
    nan = rng.random(n) < 0.1
    v = np.where(nan, u32(pattern), S.bits(fin)).astype(u32).view(f32)
    assert int(np.isnan(v).sum()) == int(nan.sum()) > 100
    specs = [("pct", 0.0), ("pct", 20.0), ("pct", 80.0), ("kth", 7, -1e30)]
    w = run_plain(D(v), int((~nan).sum()), specs)
    got = check_against_reference("nan-%08x" % pattern, v, specs, w)
    # the same values with the producers' NaN: identical results, whatever the NaN looked like
    canon = np.where(nan, u32(S.QNAN), S.bits(fin)).astype(u32).view(f32)
    got_c = result_words(run_plain(D(canon), int((~nan).sum()), specs), len(specs))
    for k in got:
        assert np.array_equal(got[k], got_c[k]), (hex(pattern), k)
    # and exactly the statistics of the valid values alone
    valid = fin[~nan]
    ref = [S.bits1(S.percentile_ref(valid, q).thr) for q in (0.0, 20.0, 80.0)] + [S.bits1(np.sort(valid)[6])]
    assert [int(x) for x in got["thr"]] == ref


def test_nothing_valid_gives_nan_for_pct_and_inf_for_kth():
    v = np.array(S.NAN_PATTERNS * 20, u32).view(f32)
    specs = [("pct", 50.0), ("kth", 5, 0.5), ("pct", 0.0)]
    w = run_plain(D(v), 0, specs)
    got = check_against_reference("all-nan", v, specs, w)
    assert [int(x) for x in got["thr"]] == [S.QNAN, 0x7F800000, S.QNAN]


# ------------------------------------------------------------------ kth rule
@pytest.mark.parametrize("case", S.KTH_CASES, ids=[c.id for c in S.KTH_CASES])
def test_kth_rule(case):
    v, specs = S.case_inputs(case)
    w = run_plain(D(v), int((~np.isnan(v)).sum()), specs)
    got = check_against_reference(case.id, v, specs, w)
    if case.specs[0][1] in ("n_valid+1", "zero", "neg", "above_total"):
        assert int(got["thr"][0]) == 0x7F800000


# ------------------------------------------------------------------ hist0 handed over by the producers
@pytest.mark.parametrize("fam", ["trained", "uniform"])
def test_producer_histogram_equals_the_plain_array_pass(fam):
    import loss_bounds as LB
    from u2pl_amd._lib import call
    H = hip()
    C, shape = 19, (2, 23, 31)
    z, t = LB.make_case(fam, C, shape)
    lab = LB.apply_ignore(t, "some")
    zd, ld = D(z), D(lab)
    n = lab.size
    # entropy producer, three percentiles
    ws = H.new_select_ws(DEV, n)
    ent = H.entropy_map(zd, ld, ws)
    assert ws._hist0
    specs = [("pct", 20.0), ("pct", 80.0), ("pct", 50.0)]
    H.run_select(ent, ws, specs)
    wp = words(ws)
    e = ent.cpu().numpy().ravel()
    assert int(wp[0]) == int((lab != 255).sum()) == int((~np.isnan(e)).sum())
    assert np.array_equal(S.bits(e[np.isnan(e)]), np.full(int(np.isnan(e).sum()), S.QNAN, u32))      # the producers' NaN
    wf = run_plain(ent.reshape(-1), int(wp[0]), specs)
    got = check_against_reference("entropy-" + fam, e, specs, wf)
    gp = result_words(wp, 3)
    print("handed over", [hex(x) for x in gp["thr"]], [hex(x) for x in gp["val"]])
    assert np.array_equal(wp[S.SEL_H0:S.SEL_H0 + 2048], wf[S.SEL_H0:S.SEL_H0 + 2048])
    assert np.array_equal(gp["thr"], got["thr"]) and np.array_equal(gp["val"], got["val"])
    # OHEM producer, one k-th spec
    ws = H.new_select_ws(DEV, n)
    mp = torch.empty(shape, dtype=torch.float32, device=DEV)
    call("u2pl_ohem_prob_f32", zd, ld, 255, shape[0], C, shape[1], shape[2], mp, ws)
    ws._hist0 = True
    nv = int(words(ws)[0])
    assert nv == int((lab != 255).sum())
    for k, floor in ((nv // 3, 0.0), (nv, 0.7), (nv + 1, 0.7)):
        wsk = ws.clone()
        wsk._hist0 = True
        H.run_select(mp, wsk, [("kth", k, floor)])
        wp = words(wsk)
        m = mp.cpu().numpy().ravel()
        wf = run_plain(mp.reshape(-1), nv, [("kth", k, floor)])
        got = check_against_reference("ohem-%s-k%d" % (fam, k), m, [("kth", k, floor)], wf, n_valid=nv)
        gp = result_words(wp, 1)
        assert np.array_equal(wp[S.SEL_H0:S.SEL_H0 + 2048], wf[S.SEL_H0:S.SEL_H0 + 2048])
        assert np.array_equal(gp["thr"], got["thr"]) and np.array_equal(gp["val"], got["val"])


# ------------------------------------------------------------------ rejections
@pytest.mark.parametrize("nspec", [0, 5])
def test_select_rejects_zero_and_five_specs_without_launching(nspec):
    from u2pl_amd import _lib
    H = hip()
    vd = D(S.family("uniform", 1000, 1))
    ws = H.new_select_ws(DEV, 1000)
    ws.fill_(0x5A5A5A5A)
    before = words(ws).copy()
    par = torch.zeros(64, dtype=torch.int64, device=DEV)       # kparam | kind | q32 | fparam, naturally aligned, all zero: pct 0
    base = par.data_ptr()
    torch.cuda.synchronize()
    cd = _lib.lib().cdll
    k0 = cd.u2pl_kernel_launches()
    rc = cd.u2pl_select_f32(vd.data_ptr(), 1000, nspec, base + 64, base + 128, base, base + 192, ws.data_ptr(), 0, _lib.stream_ptr())
    k1 = cd.u2pl_kernel_launches()
    torch.cuda.synchronize()
    print("rc", rc, "launches", k1 - k0)
    assert rc == S.EINVAL
    assert k1 - k0 == 0
    assert np.array_equal(words(ws), before)
    if nspec:
        with pytest.raises(_lib.HipError, match=str(S.EINVAL)):
            H.run_select(vd, ws, [("pct", 50.0)] * nspec)
        assert np.array_equal(words(ws), before)


# ------------------------------------------------------------------ drop rule
def test_drop_rule_with_the_threshold_on_a_tie_value():
    H = hip()
    n = 20000
    ent = S.family("runs", n, 9, nan_frac=0.1)
    valid = ent[~np.isnan(ent)]
    q = S.q_between(valid.size, S.edge_rank(valid, "in_run"))
    ws = H.new_select_ws(DEV, n)
    ws[0] = int(valid.size)
    ed = D(ent)
    thr = H.run_select(ed, ws, [("pct", q)])
    t = thr.cpu().numpy()[0]
    ties = int((valid == t).sum())
    assert ties >= 2 and S.bits1(t) == S.bits1(S.percentile_ref(valid, q).thr)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 19, n).astype(np.int64)
    lab[rng.random(n) < 0.05] = 255
    tgt = D(lab)
    nk = H.drop_high_entropy_(tgt, ed, thr[0:1])
    with np.errstate(invalid="ignore"):
        want = np.where(ent >= t, 255, lab)
    out = tgt.cpu().numpy()
    print("thr", t, "ties", ties, "dropped", int((want != lab).sum()), "nan", int(np.isnan(ent).sum()), "nkept", int(nk))
    assert np.array_equal(out, want)
    assert np.array_equal(out[np.isnan(ent)], lab[np.isnan(ent)])          # NaN pixels keep their label
    assert (out[ent == t] == 255).all() and (want != lab).sum() > ties
    assert int(nk) == int((want != 255).sum())


# ------------------------------------------------------------------ the fused split at its route switch
B_, C_, S_LOW, S_FULL = 2, 19, 25, 97          # 18818 pixels: the smallest fixture size above RF_CAP (relsplit_97_a13)


def _labels(seed):
    g = torch.Generator().manual_seed(seed)
    lab_l = torch.randint(0, C_, (B_, S_FULL, S_FULL), generator=g)
    lab_l[:, :8] = 255
    lab = torch.randint(0, C_, (B_, S_FULL, S_FULL), generator=g)
    return lab_l.to(DEV), lab


def _keep_only(lab, region, count, seed):
    """label 255 on all pixels of the boolean region but `count` of them, chosen by a seeded permutation"""
    idx = np.flatnonzero(region.ravel())
    assert idx.size >= count
    drop = np.random.default_rng(seed).permutation(idx)[count:]
    flat = lab.reshape(-1)
    flat[torch.from_numpy(drop)] = 255


def _fused(low, lab_l, lab_u, pcts):
    H = hip()
    h0 = H.split_route_stats()
    f = H.reliability_split(low, (S_FULL, S_FULL), lab_l, lab_u, (S_LOW, S_LOW), pcts, fused=True)
    assert "nkept" in f, "the fused kernel was not used"
    keep = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in f.items()}
    h1 = H.split_route_stats()
    return keep, (h1[0] - h0[0], h1[1] - h0[1])


@pytest.mark.parametrize("K,second", [(S.RF_CAP - 1, 0), (S.RF_CAP, 0), (S.RF_CAP + 1, 1)], ids=["cap-1", "cap", "cap+1"])
def test_fused_split_route_switch_on_equal_candidates(K, second):
    from test_gpu_loss_path import _self_consistent
    assert B_ * S_FULL * S_FULL > S.RF_CAP + 1
    lab_l, lab = _labels(K)
    _keep_only(lab, np.ones(lab.numel(), bool), K, K)
    lab_u = lab.to(DEV)
    low = (torch.zeros(B_, C_, S_LOW, S_LOW, device=DEV) + torch.arange(C_, device=DEV).view(1, C_, 1, 1) * 0.1)
    low = low.contiguous(memory_format=torch.channels_last)
    pcts = [80.0, 20.0, 80.0]
    f, (launches, big) = _fused(low, lab_l, lab_u, pcts)
    ent = f["entropy"].cpu().numpy()
    vals = np.unique(S.bits(ent[~np.isnan(ent)]))
    print("K", K, "valid", int((~np.isnan(ent)).sum()), "distinct entropies", [hex(x) for x in vals], "launches", launches, "second barrier", big,
          "thr", f["thr"].cpu().numpy(), "err", int(f["err"]))
    assert int((~np.isnan(ent)).sum()) == K and vals.size == 1       # K equal candidates in one bin: ncand == K
    assert int(f["err"]) == 0
    assert (launches, big) == (1, second)
    _self_consistent(f, lab_u, pcts, (S_LOW, S_LOW))


def test_fused_split_two_lists_that_fit_with_a_total_above_the_cap():
    from test_gpu_loss_path import _self_consistent, _split_equal
    H = hip()
    nA, nB, r0 = S.RF_CAP - 10, 2000, 17
    lab_l, lab = _labels(1)
    rows = np.zeros((B_, S_FULL, S_FULL), bool)
    top, mix, bot = rows.copy(), rows.copy(), rows.copy()
    top[:, :4 * (r0 - 1)] = True                  # taps inside block A (low-resolution rows < r0)
    mix[:, 4 * (r0 - 1):4 * r0] = True            # the cells whose corners see both blocks
    bot[:, 4 * r0:] = True                        # taps inside block B
    _keep_only(lab, top, nA, 1)
    _keep_only(lab, mix, 0, 2)
    _keep_only(lab, bot, nB, 3)
    lab_u = lab.to(DEV)
    low = torch.zeros(B_, C_, S_LOW, S_LOW, device=DEV)
    low[:, :, :r0] = (torch.arange(C_, device=DEV) * 0.1).view(1, C_, 1, 1)
    low[:, 0, r0:] = 5.0
    low = low.contiguous(memory_format=torch.channels_last)
    # the two entropy values, from the kernel's own output (any percentiles: the entropy map does not depend on them)
    f0, _ = _fused(low, lab_l, lab_u, [50.0, 20.0, 80.0])
    e0 = f0["entropy"].cpu().numpy()
    v0 = np.sort(e0[~np.isnan(e0)])
    vals, counts = np.unique(S.bits(v0), return_counts=True)
    sc = S.rf_bin_scale(C_)
    bins = [S.rf_bin(x, sc) for x in vals.view(f32)]
    print("values", vals.view(f32), "counts", counts, "bins", bins)
    assert vals.size == 2 and sorted(counts.tolist()) == sorted([nA, nB]) and bins[0] != bins[1]
    assert max(counts) <= S.RF_CAP < nA + nB
    n, n_low = nA + nB, int((v0 == v0[0]).sum())
    pcts = [S.q_between(n, n_low - 1), S.q_between(n, n_low // 2), S.q_between(n, n_low + (n - n_low) // 2)]
    for q, (a, b) in zip(pcts, ((v0[0], v0[-1]), (v0[0], v0[0]), (v0[-1], v0[-1]))):
        p = S.percentile_ref(v0, q)
        assert (p.a, p.b) == (a, b) and 0 < p.gamma < 1
    f, (launches, big) = _fused(low, lab_l, lab_u, pcts)
    print("pcts", pcts, "launches", launches, "second barrier", big, "thr", f["thr"].cpu().numpy(), "err", int(f["err"]))
    assert int(f["err"]) == 0 and launches == 1
    assert torch.equal(f["entropy"].view(torch.int32), f0["entropy"].view(torch.int32))
    _self_consistent(f, lab_u, pcts, (S_LOW, S_LOW))
    assert big == 1          # both bins are selected: ncand = nA + nB > RF_CAP, and each list is staged in LDS (n <= RF_CAP)
    u = H.reliability_split(low, (S_FULL, S_FULL), lab_l, lab_u, (S_LOW, S_LOW), pcts, fused=False)
    _self_consistent(u, lab_u, pcts, (S_LOW, S_LOW))
    _split_equal(f, u, 3)
