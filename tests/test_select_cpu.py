"""Conditions on the selection reference alone (tests/select_ref.py); no GPU.

tests/test_gpu_select_exact.py holds u2pl_amd/csrc/select.hip to select_ref bit for bit.  That is worth as much as the
reference and as the cases are: here the reference is held to np.percentile (scalar python-float q: numpy's float32 path),
and every shared case is shown to stand on the edge of the kernel it is named for, by a descriptor computed with the
reference arithmetic only.  The edges, and the lines of select.hip they exercise:

  leaders1>4 / leaders2>4  more than GROUP = 4 distinct prefixes among the rank slots after level 0 / level 1: the
                           `for (base = 0; base < nlead; base += GROUP)` loop of k_sel_pass<1> / <2> takes a second sweep
  one_bin0 / one_bin01     every value shares its upper 11 / 22 key bits: hist0 (and hist1) have ONE occupied bin, resolve_level
                           finds every rank in the same thread's registers and the last pass resolves everything
  split0 / split1 / split2 lo and hi of one percentile in different bins of hist0 / the same bin of hist0 but different bins of
                           hist1 / different only in the last 10 bits: `k >= excl && k < incl` of resolve_level at a bin's last
                           and first member, set_leaders giving the two slots one leader or two
  run_edge / in_run        lo the last of a tie run and hi the first of the next / both inside one run: nk (the rank left inside
                           the prefix) at count - 1 and 0 / anywhere inside
  gamma0 / gamma_half      the lerp weight of k_sel_finish at 0 and at the `t >= 0.5f` switch of its two forms
  q0 / q100, n=1..7        the clamps of resolve_chain (`vi >= n - 1`, lo = hi)
  duplicates / mixed       slots that share a leader from the start; pct and kth specs in one call (ranks from n_valid and n_total)
"""
import numpy as np
import pytest

import select_ref as S

f32, u32 = np.float32, np.uint32
ALL = S.CASES + S.LAYOUT_CASES + S.KTH_CASES
IDS = [c.id for c in ALL]


def _same_bits_or_both_nan(a, b):
    a, b = f32(a), f32(b)
    return (np.isnan(a) and np.isnan(b)) or S.bits1(a) == S.bits1(b)


# ------------------------------------------------------------------ keys
def test_key_orders_like_the_floats_and_unkey_inverts_it():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(u32)
    w = np.concatenate([w, np.array([0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x007FFFFF, 0x807FFFFF], u32)])
    v = w.view(f32)
    assert np.array_equal(S.bits(S.unkey(S.key(v))), w)
    fin = v[~np.isnan(v)]
    order = np.argsort(S.key(fin), kind="stable")
    srt = fin[order]
    assert (srt[:-1] <= srt[1:]).all()
    assert S.key(f32(-0.0)) < S.key(f32(0.0))
    assert S.key(f32(-np.inf)) == S.key(fin).min() or S.key(f32(-np.inf)) < S.key(fin).min()


def test_selection_key_puts_every_nan_above_inf_and_keeps_the_producers_nan():
    pats = np.array(S.NAN_PATTERNS, u32).view(f32)
    assert np.isnan(pats).all()
    assert (S.sel_key(pats) > S.key(f32(np.inf))).all()
    assert S.sel_key(pats[:1])[0] == S.key(pats[:1])[0] == 0xFFC00000 and (S.sel_key(pats) == 0xFFC00000).all()
    # f32_key itself sorts a NaN with the sign bit BELOW -inf: what the plain-array passes must not do
    assert S.key(pats[1:2])[0] == 0x003FFFFF < S.key(f32(-np.inf))
    fin = S.family("octaves", 1000, 0)
    assert np.array_equal(S.sel_key(fin), S.key(fin))
    assert (S.bits(S.unkey(S.sel_key(pats))) == S.QNAN).all()


def test_rf_bin_restatement_is_monotone():
    sc = S.rf_bin_scale(19)
    e = np.sort(np.concatenate([S.family("entropy_like", 5000, 0), np.linspace(0, 3.0, 5000).astype(f32), [f32(-1e-7), f32(0)]]))
    b = [S.rf_bin(x, sc) for x in e]
    assert all(x <= y for x, y in zip(b[:-1], b[1:])) and b[0] == 0 and max(b) <= 2047 and len(set(b)) > 500


# ------------------------------------------------------------------ the reference against numpy
def _agree(name, v, q):
    valid = v[~np.isnan(v)]
    p = S.percentile_ref(valid, q)
    with np.errstate(invalid="ignore"):
        want = np.percentile(valid, q)
    assert isinstance(q, float) and want.dtype == f32
    if name == "signed_zeros":      # numpy's sort does not order -0 against +0, the key does: equal as floats
        assert p.thr == want, (name, q, p, want)
    else:
        assert _same_bits_or_both_nan(p.thr, want), (name, q, p, want)
    return p


@pytest.mark.parametrize("name", S.FAMILIES)
def test_reference_equals_numpy_on_every_family(name):
    kw = dict(two_values=dict(nA=300, a=0.5, b=0.75)).get(name, {})
    nan_seen = False
    for n in (1, 2, 3, 4, 5, 7, 100, 1001, 4098):
        if name == "two_values" and n <= 300:
            kw = dict(nA=n // 2, a=0.5, b=0.75)
        v = S.family(name, n, 7, **kw)
        if not (~np.isnan(v)).any():
            continue
        for q in (0.0, 16.5, 20.0, 50.0, 83.7, 99.99, 100.0):
            p = _agree(name, v, q)
            nan_seen |= bool(np.isnan(p.thr))
    if name == "infinities":
        assert nan_seen      # infinite neighbours: inf - inf in the lerp, NaN on both sides


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_reference_equals_numpy_and_chain_ends_at_the_selected_values(case):
    v, specs = S.case_inputs(case)
    valid = v[~np.isnan(v)]
    lv = S.chain(v, specs)
    exp = S.expected(v, specs)
    keys = S.sel_key(v)
    assert int(lv[0]["hist"][0].sum()) == v.size and lv[0]["n_leaders"] == 1
    for L in (1, 2):
        for l, h in lv[L]["hist"].items():
            sh = S.SHIFTS[L - 1]
            assert int(h.sum()) == int(((keys >> u32(sh)) == u32(lv[L - 1]["prefix"][l] >> sh)).sum()) > 0
    for j, s in enumerate(specs):
        if s[0] == "pct" and valid.size:
            p = _agree(case.family, v, s[1])
            assert lv[2]["prefix"][2 * j] == int(S.key(p.a).reshape(-1)[0]) and lv[2]["prefix"][2 * j + 1] == int(S.key(p.b).reshape(-1)[0])
            assert 0 <= p.lo <= p.hi <= valid.size - 1 and p.hi - p.lo <= 1
            srt = np.sort(valid)
            assert p.a == srt[p.lo] and p.b == srt[p.hi]
        # the full key that the chain selects is the value word that the kernel must write
        assert int(S.sel_key(exp["val"][2 * j: 2 * j + 2].view(f32))[0]) == lv[2]["prefix"][2 * j]
        assert int(S.sel_key(exp["val"][2 * j: 2 * j + 2].view(f32))[1]) == lv[2]["prefix"][2 * j + 1]


# ------------------------------------------------------------------ every shared case reaches its edge
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_reaches_the_edge_it_is_named_for(case):
    v, specs = S.case_inputs(case)
    tok, fig = S.describe(v, specs)
    print(case.id, sorted(tok), fig)
    assert 1 <= len(specs) <= 4 and all(s[0] in ("pct", "kth") for s in specs)
    assert v.size <= 262144 + 5 and (v.size <= 70001 or case.id == "layout-trip")
    for e in case.expect:
        assert e in tok, (case.id, e, sorted(tok), fig)


def test_the_cases_together_reach_every_edge():
    reached = set()
    nspec = set()
    for c in S.CASES + S.LAYOUT_CASES:
        v, specs = S.case_inputs(c)
        assert set(c.expect) <= S.describe(v, specs)[0]
        reached |= set(c.expect)
        nspec.add(len(specs))
    want = {"leaders1>4", "leaders2>4", "one_bin0", "one_bin01", "split0", "split1", "split2", "run_edge", "in_run", "gamma0",
            "gamma_half", "q0", "q100", "duplicates"} | {"n=%d" % n for n in (0, 1, 2, 3, 4, 5, 7)}
    assert want <= reached, want - reached
    assert nspec == {1, 2, 3, 4}
    assert {c.family for c in S.CASES} == set(S.FAMILIES)
    assert [P for P in (S.P(50, 50, 20, 20), S.P(0, 100, 0, 100)) if P in [c.specs for c in S.CASES]] == [S.P(50, 50, 20, 20), S.P(0, 100, 0, 100)]
    mixed = [S.case_inputs(c)[1] for c in S.CASES if c.id == "octaves-mixed"][0]
    assert [s[0] for s in mixed] == ["pct", "kth", "pct", "kth"]
    assert sorted({S.case_inputs(c)[0].size % 4 for c in S.LAYOUT_CASES}) == [0, 1, 2, 3]
    assert max(S.case_inputs(c)[0].size for c in S.LAYOUT_CASES) == 256 * 256 * 4 + 5


# ------------------------------------------------------------------ builders and the k-th rule
def test_spec_builders_hold_their_own_property():
    for n in (2, 3, 5, 899, 4097, 70001, 262149):
        for r in sorted({0, 1 % (n - 1), (n - 2) // 2, n - 2}):
            lo, hi, g = S.vindex(n, S.q_between(n, r))
            assert (lo, hi) == (r, r + 1) and 0 < g < 1
    for n, r in ((4097, 1024), (4097, 3072), (5, 2), (1001, 250), (3, 1), (2, 0)):
        lo, hi, g = S.vindex(n, S.q_exact(n, r))
        assert (lo, hi) == (r, r + 1) and g == 0
    for n in (2, 4, 4098):
        assert S.vindex(n, 50.0)[2] == f32(0.5)
    for n in (1, 2, 3):
        assert S.vindex(n, 0.0)[:2] == (0, min(1, n - 1)) and S.vindex(n, 100.0)[:2] == (n - 1, n - 1)
    assert S.vindex(0, 50.0)[:2] == (0, 0)


@pytest.mark.parametrize("case", S.KTH_CASES, ids=[c.id for c in S.KTH_CASES])
def test_kth_reference_is_the_ohem_rule(case):
    v, specs = S.case_inputs(case)
    (_, k, floor), = specs
    valid = np.sort(v[~np.isnan(v)])
    r = S.kth_ref(v, valid.size, k, floor)
    where, rel = case.specs[0][1], case.specs[0][2]
    if where in ("n_valid+1", "zero", "neg", "above_total"):
        assert r.thr == np.inf and (k > valid.size or k <= 0)
    else:
        kth = valid[k - 1]
        assert r.a == kth and r.thr == max(kth, f32(floor))
        assert (f32(floor) < kth, f32(floor) == kth, f32(floor) > kth) == (rel < 0, rel == 0, rel > 0)
        if where == "run_edge" and case.family == "runs":
            assert valid[k - 2] == kth != valid[k]
    if case.family == "runs":
        assert valid.size < v.size      # NaNs present: n_valid + 1 is still inside the array
