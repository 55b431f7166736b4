"""-m gpu: the contrastive kernels of u2pl_amd/csrc/contrast.hip held to float64 at every dispatch edge (tests/contrast_bounds.py;
INTEGRATION.md section 4).  All shapes are tiny.

  a. k_infonce, every instantiation, per anchor against float64 (u2pl_infonce_f32 called directly on a hand-built job table)
  b. u2pl_infonce_fused_f32 against u2pl_infonce_f32 + u2pl_infonce_reduce_f32 at 1, 31, 32, 33 and 1088 blocks; Q % 4 != 0
  c. the stale-row clearing of the fused launch when the previous step had more jobs (hipops._InfoNCE, two steps);
     u2pl_scatter_rows_ordered_f32 called directly on multi-leader chains
  d. phase 1 (classify, compaction, prototypes) against oracle.restate.contra_phase1, exact, C in {2, 5, 19, 20, 21, 32}
  e. compute_contra_memobank_loss against oracle.restate.contra_memobank_loss away from the stock shape

Which case reaches which instantiation (test_infonce_every_instantiation ids are D-K-temp-family; VPL = D / 64, PRE = K <= 64,
ONLINE = 2 / temp > 80):

  k_infonce<1, true,  false>  64-50-0.025-random      k_infonce<1, true,  true>  64-50-0.024-random
  k_infonce<1, false, false>  64-100-0.025-random     k_infonce<1, false, true>  64-100-0.024-random
  k_infonce<2, true,  false>  128-50-0.025-random     k_infonce<2, true,  true>  128-50-0.024-random
  k_infonce<2, false, false>  128-100-0.025-random    k_infonce<2, false, true>  128-100-0.024-random
  k_infonce<4, true,  false>  256-50-0.025-random     k_infonce<4, true,  true>  256-50-0.024-random
  k_infonce<4, false, false>  256-100-0.025-random    k_infonce<4, false, true>  256-100-0.024-random
  k_infonce<8, true,  false>  512-50-0.025-random     k_infonce<8, true,  true>  512-50-0.024-random
  k_infonce<8, false, false>  512-100-0.025-random    k_infonce<8, false, true>  512-100-0.024-random
  (each also with the anti and zero families; the full K list {1, 3, 4, 7, 8, 50, 64, 65, 100} at D = 256 and 64, temp 0.5 / 0.01)
  k_contra_classify_rows      test_phase1_against_restate[*-nhwc-*] with C odd (5, 19, 21)
  k_contra_classify           every nchw case, and nhwc with C even (2, 20, 32)
  u2pl_contra_phase1 C = 19 / 21 / 32 (k_proto_stream<19 / 21 / 32>, k_phase1_tail)   test_phase1_against_restate[19- / 21- / 32-*]
  five-launch sequence        the same three with PHASE1_FUSED off, and C = 2, 5 (k_proto_stream<19>), 20 (k_proto_stream<21>)

Set U2PL_CONTRAST_RECORD to a path to have the worst excess per family written there as JSON (the figures of DESIGN.md)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_bounds as CB  # noqa: E402
from oracle import restate as R  # noqa: E402
from oracle.gen_golden import CONTRA_CFG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U2PL_EINVAL = 1001
K_LIST = (1, 3, 4, 7, 8, 50, 64, 65, 100)
WORST = {}


def hip():
    from u2pl_amd import hipops as H
    return H


def lib():
    from u2pl_amd import _lib
    return _lib


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def _note(kind, fam, e):
    WORST[f"{kind}/{fam}"] = max(WORST.get(f"{kind}/{fam}", 0.0), float(e))


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    print("\nworst excess (error / bound):", json.dumps(WORST, sort_keys=True))
    path = os.environ.get("U2PL_CONTRAST_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


_REFS = {}


def _case_ref(fam, D, K, Q, temp, jobs=CB.JOBS3, P=48, seed=1):
    """the case and its float64 reference: computed once, shared, never modified"""
    ck = (fam, D, K, Q, jobs, P, seed)
    if ck not in _REFS:
        _REFS[ck] = CB.make_case(fam, seed, D, K, Q, jobs, P)
    rk = ck + (temp,)
    if rk not in _REFS:
        _REFS[rk] = CB.case_ref(_REFS[ck], temp)
    return _REFS[ck], _REFS[rk]


def _launch_plain(case, dc, temp, Q=None):
    lib().call("u2pl_infonce_f32", dc["jobs"], len(case["jobs"]), dc["rep"], dc["ld"], case["D"], Q or case["Q"], case["K"], float(temp),
               dc["loss_q"], dc["ganchor"], dc["apix"], dc["head"], dc["nxt"], dc["groups"][2])
    torch.cuda.synchronize()


def _check_outputs(case, ref, dc, temp, tag):
    """loss_q and ganchor per anchor within the bounds, anchor_pix exact, the per-pixel chains hold exactly the group leaders"""
    l64, g64, pix, anchors = ref
    D, K, Q, nj = case["D"], case["K"], case["Q"], len(case["jobs"])
    n = nj * Q
    el = CB.loss_excess(dc["loss_q"][:n].cpu().numpy().reshape(nj, Q), l64, D, K, temp)
    eg = CB.grad_excess(dc["ganchor"][:n].cpu().numpy().reshape(nj, Q, D), g64, anchors, D, K, temp)
    _note("loss", case["family"], el), _note("grad", case["family"], eg)
    print(f"{tag}: loss excess {el:.4f} grad excess {eg:.4f}")
    assert el <= 1.0 and eg <= 1.0, (tag, el, eg)
    apix = dc["apix"][:n].cpu().numpy()
    assert np.array_equal(apix, pix.reshape(-1))
    head, nxt, seg_len = dc["head"].cpu().numpy(), dc["nxt"][:n].cpu().numpy(), dc["groups"][2].cpu().numpy()
    leaders = {}
    for e in np.flatnonzero(seg_len[:n] > 0):
        leaders.setdefault(int(apix[e]), []).append(int(e))
    for p in range(case["P"]):
        chain, cur = [], int(head[p])
        while cur != -1:
            assert 0 <= cur < n and len(chain) < n, (tag, p, chain)
            chain.append(cur)
            cur = int(nxt[cur])
        assert sorted(chain) == leaders.get(p, []) and len(set(chain)) == len(chain), (tag, p, chain)


def _nce_cases():
    out = []
    for D in (64, 128, 256, 512):          # every (VPL, PRE, ONLINE): K on both sides of 64, the last fixed-shift and the first online temp
        for K in (50, 100):
            for temp in (0.025, 0.024):
                out += [(D, K, temp, fam) for fam in ("random", "anti", "zero")]
    for D in (256, 64):                    # the full K list: 1 + K inside the first batch, on a batch edge, one past it
        for K in K_LIST:
            out += [(D, K, 0.5, "random"), (D, K, 0.01, "zero")]
    out += [(256, 7, 0.07, fam) for fam in CB.FAMILIES] + [(128, 65, 0.07, "aligned"), (64, 8, 0.5, "scales"), (512, 3, 0.01, "anti")]
    return out


@pytest.mark.parametrize("D,K,temp,fam", _nce_cases(), ids=lambda v: str(v))
def test_infonce_every_instantiation(D, K, temp, fam):
    """Q = 8, three jobs: candidate lists of 1, 5 and 11 pixels with one pixel on two lists, rings of capacity 7 (head 0, partly
    filled), 64 (head = cap - 2, full: most rows wrap) and 300"""
    case, ref = _case_ref(fam, D, K, 8, temp)
    dc = CB.device_case(case, DEV)
    _launch_plain(case, dc, temp)
    _check_outputs(case, ref, dc, temp, f"{D}-{K}-{temp}-{fam}")


@pytest.mark.parametrize("D,K,temp", [(128, 8, 0.5), (256, 65, 0.024)])
def test_infonce_rows_as_a_column_slice(D, K, temp):
    """the feature rows are a column slice of a wider buffer (ld = D + 64) whose other columns hold NaN"""
    case, ref = _case_ref("random", D, K, 8, temp)
    dc = CB.device_case(case, DEV, ld=D + 64)
    assert dc["ld"] == D + 64 and dc["rep"].stride(0) == D + 64
    _launch_plain(case, dc, temp)
    _check_outputs(case, ref, dc, temp, f"ld-{D}-{K}-{temp}")


# ---- b. fused entry against the two-launch form --------------------------------------------------------------------------------
def _jobs(nj):
    return tuple(CB.JOBS3[j % 3] for j in range(nj))


@pytest.mark.parametrize("nj,Q,D,K,temp", [(1, 4, 64, 3, 0.5), (31, 4, 128, 7, 0.5), (32, 4, 256, 8, 0.024), (11, 12, 64, 65, 0.07),
                                           (17, 256, 64, 3, 0.5)], ids=["nb1", "nb31", "nb32", "nb33", "nb1088"])
def test_infonce_fused_equals_two_launch_form(nj, Q, D, K, temp):
    """njobs * Q / 4 blocks of 1, 31, 32, 33 (the ticket shards on both sides of 32) and 1088 (more than one sweep of 1024
    partials); each twice on ONE workspace zeroed once (the tickets must be left at zero); loss bits equal, both within the bound
    of the float64 mean"""
    assert nj * Q // 4 in (1, 31, 32, 33, 1088)
    case, ref = _case_ref("random", D, K, Q, temp, jobs=_jobs(nj), P=256, seed=2)
    l64 = ref[0]
    inv_vs = 1.0 / (nj + 1)
    dc = CB.device_case(case, DEV)
    _launch_plain(case, dc, temp)
    loss2 = torch.zeros((), device=DEV)
    lib().call("u2pl_infonce_reduce_f32", dc["loss_q"], nj, Q, inv_vs, loss2)
    want64 = l64.sum() / Q * float(np.float32(inv_vs))
    # the mean of per-anchor errors each <= E_loss max(1, |l_q|), plus the reduction's own rounding to fp32
    bound = CB.E_loss(D, K, temp) * np.maximum(1.0, np.abs(l64)).sum() / Q * inv_vs + CB.EPS * abs(want64)
    ws = torch.zeros(lib().query("u2pl_infonce_fused_workspace_bytes", nj, Q), dtype=torch.uint8, device=DEV)
    for rep in range(2):
        df = CB.device_case(case, DEV)
        lossf = torch.full((), -1.0, device=DEV)
        lib().call("u2pl_infonce_fused_f32", df["jobs"], nj, df["rep"], df["ld"], D, Q, K, float(temp), df["loss_q"], df["ganchor"],
                   df["apix"], df["head"], df["nxt"], df["groups"][2], None, 0, None, 0, ws, inv_vs, lossf)
        torch.cuda.synchronize()
        assert torch.equal(df["loss_q"], dc["loss_q"]) and torch.equal(df["ganchor"], dc["ganchor"]) and torch.equal(df["apix"], dc["apix"])
        print(f"nb {nj * Q // 4} run {rep}: fused {float(lossf)!r} two-launch {float(loss2)!r} float64 {want64!r} bound {bound:.3e}")
        assert abs(float(lossf) - want64) <= bound and abs(float(loss2) - want64) <= bound
        assert float(lossf) == float(loss2), (rep, float(lossf), float(loss2))
        assert not ws[:33 * 4].any(), "the ticket counters must be left at zero"
    _check_outputs(case, ref, df, temp, f"fused-nb{nj * Q // 4}")


def test_infonce_q_not_a_multiple_of_four():
    """Q = 6, two jobs (entry e = job * Q + q with job > 0: the second job's rows start inside a four-wave block's worth of
    entries): the fused entry refuses (U2PL_EINVAL), u2pl_infonce_f32 computes all twelve anchors (each job's second block's
    last two waves leave early) and writes nothing past row njobs * Q of slightly oversized, sentinel-filled outputs"""
    D, K, temp, Q = 64, 7, 0.5, 6
    case, ref = _case_ref("random", D, K, Q, temp, jobs=CB.JOBS3[1:], P=48, seed=3)
    nj = len(case["jobs"])
    assert nj == 2
    dc = CB.device_case(case, DEV, rows_past_Q=4)
    ws = torch.zeros(lib().query("u2pl_infonce_fused_workspace_bytes", nj, 8), dtype=torch.uint8, device=DEV)
    loss = torch.zeros((), device=DEV)
    with pytest.raises(lib().HipError, match=str(U2PL_EINVAL)):
        lib().call("u2pl_infonce_fused_f32", dc["jobs"], nj, dc["rep"], D, D, Q, K, temp, dc["loss_q"], dc["ganchor"], dc["apix"], dc["head"],
                   dc["nxt"], dc["groups"][2], None, 0, None, 0, ws, 1.0, loss)
    torch.cuda.synchronize()
    assert bool((dc["loss_q"] == -7.0).all()) and bool((dc["head"] == -1).all())
    _launch_plain(case, dc, temp)
    _check_outputs(case, ref, dc, temp, "Q6")
    assert bool((dc["loss_q"][nj * Q:] == -7.0).all()) and bool((dc["ganchor"][nj * Q:] == -7.0).all())
    assert bool((dc["apix"][nj * Q:] == -7).all()) and bool((dc["nxt"][nj * Q:] == -7).all())


# ---- c. stale-row clearing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 256])
def test_stale_rows_of_a_step_with_more_jobs_are_cleared(D):
    """step 1: five jobs, step 2: one job on the same (P, D) through hipops._InfoNCE -- step 2's forward has 8 waves for the 40
    rows step 1 wrote (the tail loop r = zw + nw).  After step 2's backward the persistent gradient buffer is the float64
    scatter of step 2 within the bound and EXACTLY zero everywhere else; every chain head is -1."""
    H = hip()
    Q, K, temp, P = 8, 7, 0.5, 96 + D // 64      # (P, D) of its own: the persistent state is keyed by it
    gout = 0.75
    steps = [(_jobs(5), 4), (CB.JOBS3[2:], 5)]
    st, pix_of_step = None, []
    for (jobs, seed), vs in zip(steps, (6, 2)):
        case, ref = _case_ref("random", D, K, Q, temp, jobs=jobs, P=P, seed=seed)
        dc = CB.device_case(case, DEV)
        rep = dc["rep"].clone().requires_grad_(True)
        with CB.recorded_calls(H) as seen:
            loss = H._InfoNCE.apply(rep, dc["jobs"], len(jobs), Q, K, temp, vs, dc["groups"], dc["keep"])
            (loss * gout).backward()
        torch.cuda.synchronize()
        assert "u2pl_infonce_fused_f32" in seen and "u2pl_zero_rows_f32" not in seen
        st = H._nce_state(rep.device, P, D)
        pix_of_step.append(np.unique(ref[2]))
        assert bool(st["grad"][T(pix_of_step[-1]).long()].any(dim=1).all()), "every drawn pixel's row was written"
        if len(jobs) == 1:
            a = seen["u2pl_infonce_fused_f32"][0]
            assert a[17] == 40 and a[14] is not None, "step 2 must be handed the 40 rows step 1 wrote"
    l64, g64, pix, anchors = ref
    scale = 1.0 / (Q * 2)
    want = CB.scatter_ref(case, g64, scale, gout)
    got = st["grad"].cpu().numpy().astype(np.float64)
    touched = np.zeros(P, dtype=bool)
    touched[pix.reshape(-1)] = True
    only1 = np.setdiff1d(pix_of_step[0], pix_of_step[1])
    assert only1.size >= 8, "step 1 must have written rows that step 2 does not (else the zero check below is vacuous)"
    assert not got[~touched].any(), "a row step 2 did not write is not zero (a stale row of step 1 survived)"
    cnt = np.bincount(pix.reshape(-1), minlength=P)
    na = np.maximum(np.linalg.norm(case["rep"].astype(np.float64), axis=1), 1e-8)
    # per component: cnt entries each within E_grad_comp, summed in fp32 (cnt - 1 adds) and scaled (scale * gout, then * sum: 2
    # roundings), |g| <= 2
    bound = cnt * (CB.E_grad_comp(D, K, temp) + 2 * (cnt + 2) * CB.EPS) / (temp * na) * scale * gout
    err = np.abs(got - want).max(axis=1)
    e = float((err[touched] / bound[touched]).max())
    _note("scatter", "random", e)
    print(f"stale D={D}: scatter excess {e:.4f}")
    assert e <= 1.0
    assert abs(float(loss) - l64.mean() / 2) <= CB.E_loss(D, K, temp) * np.maximum(1, np.abs(l64)).mean() / 2 + CB.EPS * l64.mean() / 2
    assert bool((st["head"] == -1).all())
    assert rep.grad.data_ptr() == st["grad"].data_ptr() or torch.equal(rep.grad, st["grad"])


@pytest.mark.parametrize("D,ld,with_gout", [(64, 64, False), (100, 132, True), (256, 320, True)])
def test_scatter_rows_ordered_direct(D, ld, with_gout):
    """u2pl_scatter_rows_ordered_f32 called directly on the chains that u2pl_infonce_f32 built: five jobs whose candidate lists
    share six pixels (up to five leaders per pixel, groups of several entries) and own one pixel each.  dst is a column slice of
    a wider, sentinel-filled buffer: a drawn pixel's row is scale * gout * (the float64 sum of its entries' src rows) within the
    (cnt + 1) roundings of any fp32 order, everything else keeps the sentinel, every chain head is left at -1."""
    Q, K, temp, P, nj = 8, 3, 0.5, 48, 5
    Dn = 64 if D == 100 else D               # k_infonce takes 64 / 128 / 256 / 512; the scatter any D % 4 == 0 up to 256
    case = CB.make_case("random", 11, Dn, K, Q, jobs=_jobs(nj), P=P)
    rng = np.random.default_rng([11, D])
    common = np.array([3, 7, 8, 20, 33, 47])
    for j, J in enumerate(case["jobs"]):
        J["cand"] = np.sort(np.r_[common, 10 + j]).astype(np.int32)
        J["ia"] = rng.integers(0, J["cand"].size, Q).astype(np.int64)
        J["ia"][0] = int(np.flatnonzero(J["cand"] == 10 + j)[0])
    dc = CB.device_case(case, DEV)
    _launch_plain(case, dc, temp)
    n = nj * Q
    apix = dc["apix"].cpu().numpy()
    assert np.array_equal(apix, np.concatenate([J["cand"][J["ia"]] for J in case["jobs"]]))
    seg_len, nxt = dc["groups"][2].cpu().numpy(), dc["nxt"].cpu().numpy()
    leaders_of = {p: int(((apix == p) & (seg_len > 0)).sum()) for p in np.unique(apix)}
    assert max(leaders_of.values()) >= 3 and min(leaders_of.values()) == 1 and int(seg_len.max()) >= 2
    src_np = rng.standard_normal((n, D)).astype(np.float32) * (10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    src = T(src_np)
    buf = torch.full((P, ld), -7.0, dtype=torch.float32, device=DEV)
    dst = buf[:, :D]
    scale, gout = 1.0 / (Q * 6), 0.75
    lib().call("u2pl_scatter_rows_ordered_f32", dst, ld, D, dc["apix"], dc["nxt"], dc["head"], dc["groups"][0], dc["groups"][1],
               dc["groups"][2], src, n, T(np.float32([gout])) if with_gout else None, float(scale))
    torch.cuda.synchronize()
    sc = float(np.float32(scale) * np.float32(gout if with_gout else 1.0))
    want, mag = np.zeros((P, D)), np.zeros((P, D))
    np.add.at(want, apix, src_np.astype(np.float64))
    np.add.at(mag, apix, np.abs(src_np.astype(np.float64)))
    cnt = np.bincount(apix, minlength=P)
    got = buf.cpu().numpy().astype(np.float64)
    assert (got[:, D:] == -7.0).all() and (got[cnt == 0] == -7.0).all()
    # cnt - 1 adds of a sum bounded by mag, the product sc * sum, and sc's own rounding (scale * gout)
    bound = (cnt[:, None] + 1) * CB.EPS * sc * mag
    e = float((np.abs(got[:, :D] - sc * want)[cnt > 0] / bound[cnt > 0]).max())
    _note("scatter_direct", "random", e)
    print(f"scatter direct D={D} ld={ld}: excess {e:.4f}; leaders per pixel {sorted(leaders_of.values())}")
    assert e <= 1.0
    assert bool((dc["head"] == -1).all())


# ---- d. phase 1 against restate.contra_phase1 --------------------------------------------------------------------------------------
def _bits_to_onehot(bits, C):
    """uint32 [N, h, w] -> int64 [N, C, h, w]"""
    return ((bits[:, None] >> np.arange(C, dtype=np.uint32)[None, :, None, None]) & 1).astype(np.int64)


def _label_bits(rng, N2, C, h, w, mode="random"):
    """class bits on ALL images: ~70 % of the pixels carry one class, ~15 % two (multi-hot), the rest none; class C - 1 (the
    sign bit of the int32 mask when C = 32) is forced onto a stripe of every image"""
    if mode == "none":
        return np.zeros((N2, h, w), dtype=np.uint32)
    if mode == "one_class":
        return np.full((N2, h, w), np.uint32(1) << np.uint32(C - 1), dtype=np.uint32)
    a = rng.integers(0, C, (N2, h, w)).astype(np.uint32)
    b = rng.integers(0, C, (N2, h, w)).astype(np.uint32)
    u = rng.random((N2, h, w))
    bits = np.where(u < 0.85, np.uint32(1) << a, np.uint32(0)) | np.where(u < 0.15, np.uint32(1) << b, np.uint32(0))
    bits[:, 1, ::2] |= np.uint32(1) << np.uint32(C - 1)
    return bits.astype(np.uint32)


def _probs(rng, kind, N2, C, h, w, cfg):
    if kind == "softmax":
        z = rng.standard_normal((N2, C, h, w)).astype(np.float32) * np.float32(2.5)
        return R.softmax_nchw(z)
    p = (rng.integers(0, 17, (N2, C, h, w)) / 16.0).astype(np.float32)       # ties are frequent and straddle both ranks
    if kind == "thresholds":
        u = rng.random((N2, C, h, w))
        p[u < 0.25] = np.float32(cfg["current_class_threshold"])
        p[u > 0.75] = np.float32(cfg["current_class_negative_threshold"])
    return p


def _run_phase1(H, fused, rows, ld, D, prob_np, layout, lbits, low, high, B, C, h, w, cfg):
    """hipops.contra_phase1 -> (outputs, the three bit planes it handed the kernels, the entry points it called)"""
    prob = T(prob_np)
    if layout == "nhwc":
        prob = prob.contiguous(memory_format=torch.channels_last)
        pstr = (prob.stride(0), prob.stride(1), prob.stride(3))
    else:
        pstr = (C * h * w, h * w, 1)
    H.PHASE1_FUSED = fused
    try:
        with CB.recorded_calls(H) as seen:
            ph = H.contra_phase1(rows, ld, D, prob, pstr, lbits, low, high, B, C, h, w, cfg)
    finally:
        H.PHASE1_FUSED = True
    torch.cuda.synchronize()
    if "u2pl_contra_phase1" in seen:
        planes = seen["u2pl_contra_phase1"][0][19:22]
    else:
        planes = seen["u2pl_contra_classify"][0][16:19]
    return ph, [p.cpu().numpy().view(np.uint32) for p in planes], set(seen)


def _check_phase1(ph, planes, ref, bits_np, low_np, rows64, C, D, tag):
    N2, h, w = bits_np.shape
    P = N2 * h * w
    counts = ph.counts.cpu().numpy().view(np.uint32)
    idx = ph.idx.cpu().numpy()
    proto = ph.proto.cpu().numpy().astype(np.float64)
    want_planes = [np.zeros(P, dtype=np.uint32) for _ in range(3)]
    for c in range(C):
        r = ref[c]
        for k, key in enumerate(("anchor_idx", "low_idx", "neg_idx")):
            want_planes[k][r[key]] |= np.uint32(1) << np.uint32(c)
            assert int(counts[k, c]) == len(r[key]), (tag, c, key, int(counts[k, c]), len(r[key]))
        for k, key in ((0, "anchor_idx"), (2, "neg_idx")):
            assert np.array_equal(idx[k, c, :len(r[key])], r[key]), (tag, c, key)
        if r["n_low"] == 0:      # documented: the prototype row of a class without low-valid pixels is NaN (k_proto_finish)
            assert np.isnan(proto[c]).all(), (tag, c)
            assert len(r["anchor_idx"]) == 0      # ... and its anchor list is empty: infonce_loss builds no job on it
        else:
            e = float((np.abs(proto[c] - r["proto"]) / (CB.proto_bound(rows64, r["low_idx"]) + 1e-300)).max())
            _note("proto", "phase1", e)
            assert e <= 1.0, (tag, c, e)
    for k, name in enumerate(("abits", "lowbits", "nbits")):
        assert np.array_equal(planes[k].reshape(-1), want_planes[k]), (tag, name)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(9, 13), (16, 16), (23, 31)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("C", [2, 5, 19, 20, 21, 32])
def test_phase1_against_restate(C, layout, hw, B):
    """exact: bit planes, the three count rows, the anchor / negative lists element by element; prototypes within the prototype
    bound.  Three probability sets (softmax; multiples of 1/16 with frequent ties; entries equal to both thresholds, whose
    comparisons are strict) x two rank configurations (the stock 3 / 20: high_rank > C at 5 and 19, low_rank >= C at 2 where every
    negative list is empty; 1 / 4), fused and five-launch form where the fused one applies."""
    H = hip()
    h, w = hw
    N2, P = 2 * B, 2 * B * h * w
    rng = np.random.default_rng([C, h, w, B, layout == "nhwc"])
    D = (4, 64, 100, 256)[(C + h + B) % 4]
    ld = D + 12
    rows_np = (rng.standard_normal((P, ld)) * 10.0 ** rng.uniform(-1, 1, (P, 1)) + 0.5).astype(np.float32)
    rows = T(rows_np)[:, 4:4 + D]
    rows64 = rows_np[:, 4:4 + D].astype(np.float64)
    rep_t = rows64.reshape(N2, h, w, D).transpose(0, 3, 1, 2)
    bits_np = _label_bits(rng, N2, C, h, w)
    onehot = _bits_to_onehot(bits_np, C)
    lbits = T(bits_np.view(np.int32))
    assert np.array_equal(H.pack_class_bits(T(onehot)).cpu().numpy().view(np.uint32), bits_np)      # class 31: the sign bit
    low_np = (rng.random((N2, 1, h, w)) < 0.5).astype(np.float32)
    high_np = (rng.random((N2, 1, h, w)) < 0.6).astype(np.float32)
    low, high = T(low_np), T(high_np)
    routes, tot_a, tot_n = set(), 0, 0
    for ranks in ((3, 20), (1, 4)):
        for kind in ("softmax", "sixteenths", "thresholds"):
            cfg = dict(CONTRA_CFG, low_rank=ranks[0], high_rank=ranks[1], current_class_threshold=0.3125 if kind != "softmax" else 0.3,
                       current_class_negative_threshold=0.6875 if kind != "softmax" else 1)
            prob_np = _probs(rng, kind, N2, C, h, w, cfg)
            ref = R.contra_phase1(rep_t, onehot[:B], onehot[B:], prob_np[:B], prob_np[B:], low_np, high_np, cfg)
            tot_a, tot_n = tot_a + sum(len(r["anchor_idx"]) for r in ref), tot_n + sum(len(r["neg_idx"]) for r in ref)
            if C <= ranks[0]:
                assert all(len(r["neg_idx"]) == 0 for r in ref)
            for fused in ((True, False) if C in (19, 21, 32) else (False,)):
                ph, planes, seen = _run_phase1(H, fused, rows, ld, D, prob_np, layout, lbits, low, high, B, C, h, w, cfg)
                routes |= seen
                assert ("u2pl_contra_phase1" in seen) == fused and ("u2pl_class_prototypes" in seen) == (not fused)
                _check_phase1(ph, planes, ref, bits_np, low_np, rows64, C, D, (C, layout, hw, B, ranks, kind, fused))
    assert tot_a > 0 and tot_n > 0      # the lists under test are not empty (C = 2: negatives only with low_rank = 1)


@pytest.mark.parametrize("mode", ["none", "one_class"])
@pytest.mark.parametrize("C", [5, 19, 32])
def test_phase1_without_label_bits_and_with_a_single_owner(C, mode):
    """no label bits at all: every count is zero and every prototype row is NaN; one class (the last: bit 31 at C = 32) owning
    every pixel: its low-valid list is the low mask, every other class is empty"""
    H = hip()
    B, h, w, D = 2, 9, 13, 64
    N2, P = 2 * B, 2 * B * h * w
    rng = np.random.default_rng([C, mode == "none"])
    rows_np = rng.standard_normal((P, D)).astype(np.float32)
    rows, rows64 = T(rows_np), rows_np.astype(np.float64)
    bits_np = _label_bits(rng, N2, C, h, w, mode)
    onehot = _bits_to_onehot(bits_np, C)
    low_np = (rng.random((N2, 1, h, w)) < 0.5).astype(np.float32)
    high_np = (rng.random((N2, 1, h, w)) < 0.6).astype(np.float32)
    cfg = dict(CONTRA_CFG, low_rank=1, high_rank=4)
    prob_np = _probs(rng, "softmax", N2, C, h, w, cfg)
    ref = R.contra_phase1(rows64.reshape(N2, h, w, D).transpose(0, 3, 1, 2), onehot[:B], onehot[B:], prob_np[:B], prob_np[B:],
                          low_np, high_np, cfg)
    for fused in ((True, False) if C in (19, 32) else (False,)):
        for layout in ("nchw", "nhwc"):
            ph, planes, _ = _run_phase1(H, fused, rows, D, D, prob_np, layout, T(bits_np.view(np.int32)), T(low_np), T(high_np), B, C, h, w, cfg)
            _check_phase1(ph, planes, ref, bits_np, low_np, rows64, C, D, (C, mode, fused, layout))
            counts = ph.counts.cpu().numpy()
            if mode == "none":
                assert not counts[:, :C].any() and bool(torch.isnan(ph.proto).all())
            else:
                assert int(counts[1, C - 1]) == int(low_np.sum()) and not counts[:, :C - 1].any()


# ---- e. the whole loss away from the stock shape -----------------------------------------------------------------------------------
def _loss_inputs(rng, C, D, B, h, w):
    N2 = 2 * B
    bits = _label_bits(rng, N2, C, h, w)
    onehot = _bits_to_onehot(bits, C)
    return dict(rep=rng.standard_normal((N2, D, h, w)).astype(np.float32), rep_t=rng.standard_normal((N2, D, h, w)).astype(np.float32),
                label_l=onehot[:B], label_u=onehot[B:], prob=_probs(rng, "softmax", N2, C, h, w, None),
                low=(rng.random((N2, 1, h, w)) < 0.6).astype(np.float32), high=(rng.random((N2, 1, h, w)) < 0.6).astype(np.float32))


@pytest.mark.parametrize("K", [3, 70])
@pytest.mark.parametrize("C,D", [(5, 64), (21, 128), (32, 256)])
def test_whole_loss_away_from_the_stock_shape(C, D, K):
    """two consecutive steps on a DeviceMemoryBank with ring capacities {1, 5, 40} cycling over the classes (a ring of length 1,
    a wrap in step 1, sampling from wrapped rings in step 2), num_queries 8, 9 x 13 maps: loss within E_loss, the gradient of rep
    within E_grad_comp / (Q valid_seg) per component and drawing entry (and within the contract 1e-5 max(1, |g|_max)), zero where nothing was drawn;
    bank contents, ptr and new_keys exact"""
    from u2pl_amd.utils import loss_helper as LH
    H = hip()
    B, h, w, Q = 2, 9, 13, 8
    temp = CB.temp32(0.07)
    # high_rank = C: every class but the top one of an unlabelled pixel is a negative, so that even at C = 32 the 468 pixels hand
    # each class more keys per step than a ring of 5 holds (a window of 3 ranks gives one or two, and no ring ever wraps)
    cfg = dict(CONTRA_CFG, num_queries=Q, num_negatives=K, temperature=temp, low_rank=1, high_rank=C, current_class_threshold=0.05,
               current_class_negative_threshold=0.5)
    caps = [(1, 5, 40)[c % 3] for c in range(C)]
    bank = H.DeviceMemoryBank(C, caps, D, DEV)
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    rbank, rptr = [[np.zeros((0, D), np.float32)] for _ in range(C)], [[0] for _ in range(C)]
    rng = np.random.default_rng([C, D, K])
    for step in range(2):
        x = _loss_inputs(rng, C, D, B, h, w)
        gen = torch.Generator().manual_seed(100 + step)
        rkeys, rloss, rgrad, info = R.contra_memobank_loss(
            x["rep"], x["label_l"], x["label_u"], x["prob"][:B], x["prob"][B:], x["low"], x["high"], cfg, rbank, rptr, caps, x["rep_t"],
            lambda high, n: torch.randint(high, (n,), generator=gen).numpy())
        rep = T(x["rep"]).requires_grad_(True)
        torch.manual_seed(100 + step)      # the product draws from the global CPU generator, in the reference's order
        keys, loss = LH.compute_contra_memobank_loss(rep, T(x["label_l"]), T(x["label_u"]), T(x["prob"][:B]), T(x["prob"][B:]), T(x["low"]),
                                                     T(x["high"]), cfg, bank, ptrs, caps, T(x["rep_t"]))
        loss.backward()
        torch.cuda.synchronize()
        assert [int(k) for k in keys] == [int(k) for k in rkeys]
        for c in range(C):
            assert np.array_equal(bank.logical(c).cpu().numpy(), rbank[c][0]), (step, c)
            assert int(ptrs[c][0]) == int(rptr[c][0]) == bank.ptr[c]
        # the enqueue precedes the sampling: in both steps at least one job draws its negatives from a ring whose head has moved
        assert any(bank.head[c] != 0 for _, c, _, _ in info["processed"]), ("no job sampled a wrapped ring", step, bank.head)
        vs = len(info["valid_classes"])
        assert vs > 1 and len(info["processed"]) == LH.LAST_STATS["njobs"] > 0 and LH.LAST_STATS["valid_seg"] == vs
        # l_q >= 0: the mean of max(1, l_q) over the anchors is <= 1 + the mean; skipped jobs only shrink it; the reduction rounds once
        lb = CB.E_loss(D, K, temp) * (1.0 + rloss) + CB.EPS * rloss
        el = abs(float(loss) - rloss) / lb
        assert abs(float(loss) - rloss) <= CB.CONTRACT_LOSS * max(1.0, abs(rloss))
        rows = x["rep"].transpose(0, 2, 3, 1).reshape(-1, D).astype(np.float64)
        cnt = np.zeros(rows.shape[0])
        for i, _, ia, _ in info["processed"]:
            np.add.at(cnt, info["ph1"][i]["anchor_idx"][ia], 1)
        na = np.maximum(np.linalg.norm(rows, axis=1), 1e-8)
        gb = cnt * (CB.E_grad_comp(D, K, temp) + 2 * (cnt + 2) * CB.EPS) / (temp * na * Q * vs)      # per component
        got = rep.grad.cpu().numpy().astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, D)
        want = rgrad.transpose(0, 2, 3, 1).reshape(-1, D)
        assert not got[cnt == 0].any()
        eg = float((np.abs(got - want).max(axis=1)[cnt > 0] / gb[cnt > 0]).max())
        _note("whole_loss", "random", el), _note("whole_grad", "random", eg)
        print(f"C={C} D={D} K={K} step {step}: loss {float(loss):.6f} ref {rloss:.6f} excess {el:.4f}; grad excess {eg:.4f}; jobs {len(info['processed'])}")
        assert el <= 1.0 and eg <= 1.0
        assert np.abs(got - want).max() <= CB.CONTRACT_GRAD * max(1.0, np.abs(want).max())
    st = H._nce_state(rep.device, 2 * B * h * w, D)
    assert bool((st["head"] == -1).all()) and st["pending"] is None


def test_whole_loss_rejects_d_512():
    """the prototypes take D <= 256: the whole-loss path raises before anything is enqueued or chained"""
    from u2pl_amd.utils import loss_helper as LH
    H = hip()
    C, D, B, h, w = 5, 512, 2, 9, 13
    x = _loss_inputs(np.random.default_rng(5), C, D, B, h, w)
    caps = [5] * C
    bank = H.DeviceMemoryBank(C, caps, D, DEV)
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    cfg = dict(CONTRA_CFG, num_queries=8, num_negatives=3, low_rank=1, high_rank=4)
    rep = T(x["rep"]).requires_grad_(True)
    with pytest.raises(lib().HipError):
        LH.compute_contra_memobank_loss(rep, T(x["label_l"]), T(x["label_u"]), T(x["prob"][:B]), T(x["prob"][B:]), T(x["low"]), T(x["high"]),
                                        cfg, bank, ptrs, caps, T(x["rep_t"]))
    torch.cuda.synchronize()
    assert bank.length == [0] * C and bank.head == [0] * C and bank.ptr == [0] * C and not bool(bank.storage.any())
    assert all(int(p[0]) == 0 for p in ptrs)
    st = H._NCE_STATE.get((str(rep.device), 2 * B * h * w, D))      # not even created: the failure comes before phase 2
    assert st is None or (bool((st["head"] == -1).all()) and st["pending"] is None)
