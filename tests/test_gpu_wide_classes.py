"""-m gpu: training with more than 32 classes (csrc/contrast_wide.hip, the *_wide producers of csrc/reliability.hip) against
the reference-generated fixtures of tools/gen_wide_golden.py, the numpy restatement (tests/wide_ref.py) and the narrow
route."""
import copy

import numpy as np
import pytest
import torch

import contrast_bounds as CB
import wide_ref as WR
from conftest import golden
from oracle import restate as R
from oracle.gen_golden import CONTRA_CFG, formula_bank

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def hip():
    from u2pl_amd import hipops as H
    return H


def _run_fixture(tag, api, check=True):
    """the steps of a contra_65_<tag> fixture through compute_contra_memobank_loss, in the form of
    test_contra_memobank_golden -> per step (loss bits, gradient), and the final banks"""
    from u2pl_amd.utils.loss_helper import compute_contra_memobank_loss
    H = hip()
    meta, steps = WR.load_contra(tag)
    C, D, B = int(meta["num_classes"]), int(meta["D"]), int(meta["B"])
    qs = [int(x) for x in meta["queue_size"]]
    pre, fill = int(meta["prefill"]), [int(x) for x in meta["fill"]]
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    if api == "device_bank":
        bank = H.DeviceMemoryBank(C, qs, D, DEV)
        for c in range(C):
            if pre:
                bank.load_logical(c, formula_bank(c, fill[c], D).to(DEV))
    else:
        bank = [[formula_bank(c, fill[c], D) if pre else torch.zeros(0, D)] for c in range(C)]
    out = []
    for st, g in enumerate(steps):
        prob = T(WR.full_prob(g["prob_slot0"], B))
        fmt = torch.channels_last if st else torch.contiguous_format
        rep = T(g["rep"]).contiguous(memory_format=fmt).requires_grad_(True)
        rep_t = T(g["rep_teacher"]).contiguous(memory_format=fmt)
        torch.set_rng_state(torch.from_numpy(g["rng_state"]))
        new_keys, loss = compute_contra_memobank_loss(
            rep, T(g["label_l_small"], torch.int64), T(g["label_u_small"], torch.int64), prob[:B], prob[B:],
            T(g["low_mask_all"], torch.float32), T(g["high_mask_all"], torch.float32), CONTRA_CFG, bank, ptrs, qs, rep_t)
        loss.backward()
        grad = rep.grad.cpu().numpy()
        out.append((np.float32(loss.item()), grad))
        if not check:
            continue
        gref = g["grad_rep"]
        print(tag, api, "step", st, "loss", loss.item(), "ref", float(g["loss"]), "grad err", float(np.abs(grad - gref).max()),
              "njobs", H.infonce_loss.last_njobs)
        assert list(new_keys) == list(g["new_keys"])
        assert H.infonce_loss.last_njobs == int(g["njobs"])
        assert abs(float(loss) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"]))), (float(loss), float(g["loss"]))
        assert np.abs(grad - gref).max() < 1e-5 * max(1.0, float(np.abs(gref).max()))
        assert [bank[c][0].shape[0] for c in range(C)] == list(g["bank_len"])
        assert [int(q[0]) for q in ptrs] == list(g["queue_ptr"])
    banks = [bank[c][0].cpu().numpy() for c in range(C)]
    if check:
        for c, b in enumerate(banks):
            head, tail = WR.bank_ends(b, D)
            assert np.array_equal(head, meta["bank_head"][c]) and np.array_equal(tail, meta["bank_tail"][c]), c
            assert np.allclose(b.astype(np.float64).sum(0), meta["bank_sum"][c], atol=1e-9), c
    return out, banks


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("tag", WR.CONTRA_TAGS)
@pytest.mark.parametrize("api", ["device_bank", "reference_lists"])
def test_wide_contra_memobank_golden(tag, api):
    """the reference's compute_contra_memobank_loss at 33 / 40 / 65 / 150 / 255 classes (what each fixture covers:
    tools/gen_wide_golden.py): new_keys, bank lengths, queue pointers and bank head / tail rows exact, the loss within
    1e-4 max(1, |loss|), grad_rep within 1e-5 max(1, max|g|) -- test_contra_memobank_golden's bounds at C = 19."""
    _run_fixture(tag, api)


@pytest.mark.parametrize("tag,B", [("c150", 2), ("c150_b3", 3)])
def test_wide_reliability_split_golden(tag, B):
    """test_reliability_split_golden at 150 classes: the reference's thresholds exact, masks exact, the unpacked planes equal
    to its label_onehot outputs (three labels on one pixel at B = 3), through reliability_masks and the fused
    reliability_apply; Tier B: entropy recomputed on the device from the logits."""
    H = hip()
    g = golden("relsplit_65_" + tag)
    C, s, S = int(g["num_classes"]), g["label_l_small"].shape[-1], int(g["size"])
    assert g["label_l"].shape[0] == B and C == 150
    lab_u, lab_l = g["label_u_aug"].astype(np.int64), g["label_l"].astype(np.int64)
    ent = g["entropy"].copy()
    ent[lab_u == 255] = np.nan            # Tier A: reference entropy is the fixed input
    ws = H.new_select_ws(DEV, ent.size)
    ws[0] = int((lab_u != 255).sum())
    a = float(g["alpha_t"])
    thr = H.run_select(T(ent), ws, [("pct", a), ("pct", 100 - a)])
    tn = thr.cpu().numpy()
    assert tn[0] == g["low_thresh"] and tn[1] == g["high_thresh"]
    low, high, lbits = H.reliability_masks(T(ent), thr[0:1], thr[1:2], T(lab_l), T(lab_u), (s, s), num_classes=C)
    assert lbits.shape == (5, 2 * B, s, s)
    assert np.array_equal(low.cpu().numpy().astype(np.uint8), g["low_mask_all"])
    assert np.array_equal(high.cpu().numpy().astype(np.uint8), g["high_mask_all"])
    oh = H.unpack_class_bits(lbits, C).cpu().numpy()
    assert np.array_equal(oh[:B].astype(np.uint8), g["label_l_small"])
    assert np.array_equal(oh[B:].astype(np.uint8), g["label_u_small"])
    assert int(oh.sum(1).max()) == (3 if B == 3 else 2)          # B labels on one pixel under the slot-0 quirk, on the device
    assert np.array_equal(H.pack_class_bits(T(oh)).cpu().numpy(), lbits.cpu().numpy())
    thr3 = torch.cat((thr[0:1], thr)).contiguous()              # (drop, low, high)
    _, _, low3, high3, lbits3 = H.reliability_apply(T(ent), thr3, T(lab_l), T(lab_u), (s, s), num_classes=C)
    assert torch.equal(low3, low) and torch.equal(high3, high) and torch.equal(lbits3, lbits)
    # Tier B: entropy recomputed on the device from the logits (the fixture holds the unlabelled half)
    large = H.bilinear_up(T(g["low_t_train"]), (S, S))
    ws2 = H.new_select_ws(DEV, ent.size)
    ent_d = H.entropy_map(large, T(lab_u), ws2)
    thr2 = H.run_select(ent_d, ws2, [("pct", a), ("pct", 100 - a)])
    low2, high2, lbits2 = H.reliability_masks(ent_d, thr2[0:1], thr2[1:2], T(lab_l), T(lab_u), (s, s), num_classes=C)
    assert (low2.cpu().numpy().astype(np.uint8) != g["low_mask_all"]).sum() <= 1
    assert (high2.cpu().numpy().astype(np.uint8) != g["high_mask_all"]).sum() <= 1
    assert torch.equal(lbits2, lbits)


def test_wide_bank_init_and_enqueue_through_the_device_resident_state():
    """u2pl_bank_init_wide + u2pl_bank_enqueue_wide_f32 in the form of the narrow test
    (test_bank_sequence_golden_through_the_device_resident_state): 40 classes, flat index lists with offsets and the
    idx == NULL / row_start form, classes over capacity (only the last `cap` rows are kept, utils.py:38-41); contents in FIFO
    order and the device state equal to the host mirror (mirror_counts) after every step."""
    from u2pl_amd._lib import call
    H = hip()
    C, D = 40, 8
    caps = [3 + (c * 5) % 7 for c in range(C)]
    bank = H.DeviceMemoryBank(C, caps, feat_dim=D, device=DEV)
    bank.state = torch.full((C, 5), -1, dtype=torch.int64, device=DEV)
    call("u2pl_bank_init_wide", bank.state, C, np.array(caps, dtype=np.int64).ctypes.data)
    bank._state_stale = False
    offs = np.concatenate([[0], np.cumsum(caps)[:-1]])
    assert bank.state.cpu().numpy().tolist() == [[int(offs[c]), caps[c], 0, 0, 0] for c in range(C)]
    with pytest.raises(_lib_error()):
        call("u2pl_bank_init_wide", bank.state, 256, np.array(caps, dtype=np.int64).ctypes.data)
    gen = torch.Generator().manual_seed(1)
    rows = torch.randn(600, D, generator=gen)
    rows_d = rows.to(DEV)
    ref = [torch.zeros(0, D) for _ in caps]
    for step in range(4):
        cnts = torch.randint(0, 6, (C,), generator=gen).tolist()
        cnts[39], cnts[step] = 12, 11                      # over capacity (caps <= 9)
        cnt_d = torch.tensor(cnts, dtype=torch.int32, device=DEV)
        start = np.concatenate([[0], np.cumsum(cnts)[:-1]]).astype(np.int64)
        if step % 2 == 0:       # flat index lists
            flat = torch.randperm(600, generator=gen)[: sum(cnts)].int()
            src = [flat[int(start[c]): int(start[c]) + cnts[c]].long() for c in range(C)]
            bank.enqueue_device(rows_d, D, flat.to(DEV), 0, cnt_d, list_off=torch.from_numpy(start).to(DEV))
        else:                   # idx == NULL: class c's rows are rows[row_start[c] + j]
            start = start + 17
            src = [torch.arange(int(start[c]), int(start[c]) + cnts[c]) for c in range(C)]
            bank._sync_state()
            call("u2pl_bank_enqueue_wide_f32", bank.state, bank.storage, D, rows_d, D, None, None, torch.from_numpy(start).to(DEV),
                 cnt_d, C)
        bank.mirror_counts(cnts)
        for c in range(C):
            ref[c] = torch.cat((ref[c], rows[src[c]]))[-caps[c]:]
            assert torch.equal(bank.logical(c).cpu(), ref[c]), (step, c)
        st = bank.state.cpu().numpy()
        assert st[:, 2].tolist() == bank.head and st[:, 3].tolist() == bank.length and st[:, 4].tolist() == bank.ptr


def _lib_error():
    from u2pl_amd import _lib
    return _lib.HipError


# ------------------------------------------------------------------ 2. stage parity
def _stage_case(C, B, s, seed):
    rng = np.random.default_rng(seed)
    S = 4 * (s - 1) + 1
    D = 64
    lab_l = rng.integers(0, C, size=(B, S // 8 + 1, S // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :S, :S].astype(np.int64)
    lab_u = rng.integers(0, C, size=(B, S // 8 + 1, S // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :S, :S].astype(np.int64)
    lab_l[:, :3] = 255
    lab_l[1, 10:14, 5:9] = 255            # ignored on ANOTHER sample only: counts as class 0 in slot 0 (Q0)
    lab_u[0, S // 2:S // 2 + 3] = 255
    lab_l[0, -8:, -8:], lab_u[0, -8:, -8:] = C - 1, C - 1      # the last class is present
    ent = rng.random((B, S, S)).astype(np.float32)
    ent[lab_u == 255] = np.nan
    tlo, thi = np.float32(0.45), np.float32(0.6)
    small_l = R.nearest_down(lab_l, s, s)
    small_u = R.nearest_down(lab_u, s, s)
    logits = (rng.standard_normal((2 * B, C, s, s)) * 2.5).astype(np.float32)
    boost = (rng.random((2 * B, s, s)) < 0.5) * 7.0
    cls = np.where(np.concatenate([small_l, small_u]) == 255, 0, np.concatenate([small_l, small_u]))
    np.put_along_axis(logits, cls[:, None], np.take_along_axis(logits, cls[:, None], 1) + boost[:, None].astype(np.float32), 1)
    prob = R.softmax_nchw(logits)
    rep_t = (np.round(rng.standard_normal((2 * B, D, s, s)) * 64) / 64).astype(np.float32)
    return dict(S=S, D=D, lab_l=lab_l, lab_u=lab_u, ent=ent, tlo=tlo, thi=thi, prob=prob, rep_t=rep_t)


@pytest.mark.parametrize("C", [33, 64, 65, 96, 97, 255])
@pytest.mark.parametrize("B,s", [(2, 5), (3, 5), (2, 17), (3, 17)])
def test_wide_stages_equal_the_numpy_restatement(C, B, s):
    """label bits (Q0, legacy nearest), abits / lowbits / nbits, list lengths and contents bit for bit against
    tests/wide_ref.py (oracle/restate.py's contra_phase1 / class_rank / label_onehot_quirk); prototypes against float64 to
    contrast_bounds.proto_bound (the C = 19 prototype bound).  Row-contiguous and planar probabilities; P = 2 B s^2 is
    100 / 150 / 1156 / 1734 pixels: never a multiple of the block's 64 / 128 / 256 pixels."""
    H = hip()
    k = _stage_case(C, B, s, 1000 * C + 10 * B + s)
    S, D = k["S"], k["D"]
    thr = T(np.array([k["tlo"], k["thi"]], np.float32))
    low, high, lbits = H.reliability_masks(T(k["ent"]), thr[0:1], thr[1:2], T(k["lab_l"]), T(k["lab_u"]), (s, s), num_classes=C)
    assert lbits.shape == (WR.words(C), 2 * B, s, s)
    oh_l = R.nearest_down(R.label_onehot_quirk(k["lab_l"], C), s, s)
    oh_u = R.nearest_down(R.label_onehot_quirk(k["lab_u"], C), s, s)
    want_planes = WR.label_planes(k["lab_l"], k["lab_u"], C, s)
    assert np.array_equal(lbits.cpu().numpy().view(np.uint32), want_planes)
    assert int(np.concatenate([oh_l, oh_u]).sum(1).max()) >= 2            # a union of labels on one pixel
    # the fused tail writes the same bits; pack / unpack round-trip
    ws3 = T(np.array([np.float32(0.9), k["tlo"], k["thi"]], np.float32))
    _, _, low2, high2, lbits2 = H.reliability_apply(T(k["ent"]), ws3, T(k["lab_l"]), T(k["lab_u"]), (s, s), num_classes=C)
    assert torch.equal(lbits2, lbits) and torch.equal(low2, low) and torch.equal(high2, high)
    oh = H.unpack_class_bits(lbits, C)
    assert np.array_equal(oh.cpu().numpy(), np.concatenate([oh_l, oh_u]).astype(np.int64))
    assert torch.equal(H.pack_class_bits(oh), lbits)
    e_small = R.nearest_down(k["ent"], s, s)
    valid_l = R.nearest_down((k["lab_l"] != 255).astype(np.float32), s, s)
    with np.errstate(invalid="ignore"):
        want_low = np.concatenate([valid_l, (e_small <= k["tlo"]).astype(np.float32)])[:, None]
        want_high = np.concatenate([valid_l, (e_small >= k["thi"]).astype(np.float32)])[:, None]
    assert np.array_equal(low.cpu().numpy(), want_low) and np.array_equal(high.cpu().numpy(), want_high)
    cfg = dict(CONTRA_CFG, current_class_threshold=0.2)
    ref = WR.phase1_ref(k["rep_t"], oh_l.astype(np.int64), oh_u.astype(np.int64), k["prob"][:B], k["prob"][B:], want_low,
                        want_high, cfg)
    assert ref["counts"][0].sum() > 0 and ref["counts"][2].sum() > 0 and ref["counts"][:, 32:].sum() > 0
    rows64 = k["rep_t"].transpose(0, 2, 3, 1).reshape(-1, D).astype(np.float64)
    rep_rows = T(k["rep_t"]).permute(0, 2, 3, 1).contiguous().reshape(-1, D)
    for layout in ("rows", "planar"):
        prob = T(k["prob"])
        if layout == "rows":
            prob = prob.contiguous(memory_format=torch.channels_last)
            pstr = (prob.stride(0), prob.stride(1), prob.stride(3))
        else:
            pstr = (C * s * s, s * s, 1)
        ph = H.contra_phase1(rep_rows, D, D, prob, pstr, lbits, low.contiguous(), high.contiguous(), B, C, s, s, cfg)
        counts = ph.counts.cpu().numpy()
        assert np.array_equal(counts, ref["counts"]), layout
        ph.finish(counts)
        assert np.array_equal(ph.offsets.cpu().numpy(), ref["offsets"]) and np.array_equal(ph.offsets_host, ref["offsets"])
        for kind in range(3):
            assert np.array_equal(ph.bits[kind].cpu().numpy().view(np.uint32), ref["bits"][kind]), (layout, kind)
        assert np.array_equal(ph.idx.cpu().numpy()[:ref["flat"].size], ref["flat"]), layout
        proto = ph.proto.cpu().numpy()
        for c, o in enumerate(ref["per"]):
            if o["n_low"] == 0:
                assert np.isnan(proto[c]).all()
            else:
                assert (np.abs(proto[c] - o["proto"]) <= CB.proto_bound(rows64, o["low_idx"]) + 1e-300).all(), (layout, c)


# ------------------------------------------------------------------ 3. narrow and wide agree
def _prefill_inputs(C):
    """step 0 of contra_65_prefill (C = 19), padded with zero-probability, never-labelled classes up to C"""
    g = golden("contra_65_prefill")
    D, B = int(g["D"]), g["s0_label_l"].shape[0]
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], C - 19) + a.shape[2:], a.dtype)], 1)
    qs = [int(x) for x in g["queue_size"]] + [3000] * (C - 19)
    fill = [int(g["prefill"]) + 3 * c for c in range(C)]
    return g, dict(D=D, B=B, qs=qs, fill=fill, prob=pad(g["s0_prob_all"]), ll=pad(g["s0_label_l_small"]), lu=pad(g["s0_label_u_small"]))


def _prefill_step(C, wide, monkeypatch):
    from u2pl_amd.utils.loss_helper import compute_contra_memobank_loss
    H = hip()
    g, k = _prefill_inputs(C)
    D, B = k["D"], k["B"]
    bank = H.DeviceMemoryBank(C, k["qs"], D, DEV)
    for c in range(C):
        bank.load_logical(c, formula_bank(c, k["fill"][c], D).to(DEV))
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    seen = {}
    orig = H.contra_phase1

    def phase1(*a, **kw):
        ph = orig(*a, wide=wide, **kw)
        seen["ph"] = ph
        return ph
    monkeypatch.setattr(H, "contra_phase1", phase1)
    prob = T(k["prob"])
    rep = T(g["s0_rep"]).requires_grad_(True)
    torch.set_rng_state(torch.from_numpy(g["s0_rng_state"]))
    new_keys, loss = compute_contra_memobank_loss(
        rep, T(k["ll"], torch.int64), T(k["lu"], torch.int64), prob[:B], prob[B:], T(g["s0_low_mask_all"], torch.float32),
        T(g["s0_high_mask_all"], torch.float32), CONTRA_CFG, bank, ptrs, k["qs"], T(g["s0_rep_teacher"]))
    loss.backward()
    monkeypatch.setattr(H, "contra_phase1", orig)
    ph = seen["ph"]
    assert bool(ph.wide) == wide
    cnt = np.asarray(ph.counts_host)[:, :C].astype(np.int64)
    lists = [[ph.list(kind, c).cpu().numpy() for c in range(C)] for kind in (0, 2)]
    bits = [b.cpu().numpy().reshape(-1) for b in ph.bits]
    return dict(new_keys=list(new_keys), loss=float(loss), grad=rep.grad.cpu().numpy(), counts=cnt, lists=lists, bits=bits,
                proto=ph.proto.cpu().numpy(), lens=list(bank.length), heads=list(bank.head), ptrs=[int(p[0]) for p in ptrs],
                banks=[bank.logical(c).cpu().numpy() for c in range(C)], gref=g)


@pytest.fixture(autouse=True)
def _clear_dropout_hook():
    yield
    from u2pl_amd import nn as Kn
    Kn.DROPOUT_HOOK = None


@pytest.mark.parametrize("C", [19, 32])
def test_forced_wide_route_equals_the_narrow_route(C, monkeypatch):
    """contra_65_prefill through both routes (wide=True is contra_phase1's test-only argument).  Every integer output --
    class bits, list lengths, list contents, new_keys, bank lengths / heads / pointers -- and the bank rows are IDENTICAL.
    Loss and gradient are held to 1e-4 max(1, |loss|) / 1e-5 max(1, max|g|), NOT bit equality: the prototypes are summed in
    a different order (narrow: fp32 per-wave partial sums, then doubles; wide: one ordered double-precision sum per
    class), so they differ in the last bit and the InfoNCE logits with them; InfoNCE itself is the same launch."""
    a, b = _prefill_step(C, False, monkeypatch), _prefill_step(C, True, monkeypatch)
    assert np.array_equal(a["counts"], b["counts"]) and a["counts"][0].sum() > 0 and a["counts"][2].sum() > 0
    for x, y in zip(a["bits"], b["bits"]):
        assert np.array_equal(x, y)
    for kind in range(2):
        for c in range(C):
            assert np.array_equal(a["lists"][kind][c], b["lists"][kind][c]), (kind, c)
    for key in ("new_keys", "lens", "heads", "ptrs"):
        assert a[key] == b[key], key
    for x, y in zip(a["banks"], b["banks"]):
        assert np.array_equal(x, y)
    assert np.array_equal(np.isnan(a["proto"]), np.isnan(b["proto"]))
    print("C", C, "loss narrow / wide", a["loss"], b["loss"], "grad diff", float(np.abs(a["grad"] - b["grad"]).max()))
    assert abs(a["loss"] - b["loss"]) < 1e-4 * max(1.0, abs(a["loss"]))
    assert np.abs(a["grad"] - b["grad"]).max() < 1e-5 * max(1.0, float(np.abs(a["grad"]).max()))
    if C == 19:      # ... and both are the reference's
        g = a["gref"]
        assert a["new_keys"] == list(g["s0_new_keys"]) == b["new_keys"]
        assert abs(b["loss"] - float(g["s0_loss"])) < 1e-4 * max(1.0, abs(float(g["s0_loss"])))
        assert np.abs(b["grad"] - g["s0_grad_rep"]).max() < 1e-5 * max(1.0, float(np.abs(g["s0_grad_rep"]).max()))


# ------------------------------------------------------------------ 3b. one body, two instantiations
# The reliability stages, pack / unpack and the device-resident bank are ONE implementation each, instantiated for one word
# of class bits per pixel (C <= 32) and for word planes / the flat list buffer.  Where both are defined they must agree
# bit for bit, and with a third party (tests/wide_ref.py, the host mirror, a FIFO of torch rows): a bug shared by both
# instantiations still shows.
SHARED_C = [1, 19, 31, 32]
_BODY_CASES = {}


def _body_case(C, B, S, s):
    """inputs shared by the tests below (built once per shape, never modified): labels from [0, C) with ignore pixels in
    batch slot 0 (own ignore: no bits) and in slot 1 only (counts as class 0 in slot 0, Q0), the last class present"""
    key = (C, B, S, s)
    if key not in _BODY_CASES:
        rng = np.random.default_rng(7000 + 100 * C + 10 * B + s)
        lab_l, lab_u = (rng.integers(0, C, size=(B, S, S)).astype(np.int64) for _ in range(2))
        lab_l[:, :3] = 255
        lab_l[1, 10:14, 5:9] = 255
        lab_u[0, S // 2:S // 2 + 3] = 255
        lab_u[B - 1, :, -4:] = 255
        lab_l[0, -8:, -8:], lab_u[1, -8:, -8:] = C - 1, C - 1
        ent = rng.random((B, S, S)).astype(np.float32)
        ent[lab_u == 255] = np.nan
        for lab in (lab_l, lab_u):        # the ignore pixels survive the down-sampling, in slot 0 and in another slot alone
            small = R.nearest_down(lab, s, s)
            assert (small[0] == 255).any() and ((small[1:] == 255).any(0) & (small[0] != 255)).any()
        thr3 = np.array([0.9, 0.45, 0.6], np.float32)          # drop, low, high
        _BODY_CASES[key] = dict(lab_l=lab_l, lab_u=lab_u, ent=ent, thr3=thr3, planes=WR.label_planes(lab_l, lab_u, C, s))
    return _BODY_CASES[key]


@pytest.mark.parametrize("C", SHARED_C)
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("S,s", [(17, 5), (65, 17)])
def test_reliability_stages_one_word_and_plane_forms_agree(C, B, S, s):
    """u2pl_reliability_apply / _masks against their _wide entries on the same inputs: target_u, nkept, low_mask and
    high_mask bit-equal, plane 0 of the wide lbits == the one-word lbits == tests/wide_ref.py's restatement (bit 31 set
    at C = 32); the target also against numpy.  apply runs with negative_high_entropy = 1, masks with 0."""
    H = hip()
    k = _body_case(C, B, S, s)
    ent, thr3, lab_l, lab_u = T(k["ent"]), T(k["thr3"]), T(k["lab_l"]), T(k["lab_u"])
    n = 2 * B * s * s

    def outputs(planes):
        f = lambda: torch.full((2 * B, 1, s, s), -7.0, device=DEV)
        return (torch.full((B, S, S), -7, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), f(), f(),
                torch.full((planes, n) if planes else (n,), -7, dtype=torch.int32, device=DEV))
    tn, kn, lown, highn, bitsn = outputs(0)
    tw, kw, loww, highw, bitsw = outputs(1)
    H.call("u2pl_reliability_apply", ent, thr3, lab_l, lab_u, 255, B, S, S, s, s, 1, tn, kn, lown, highn, bitsn)
    H.call("u2pl_reliability_apply_wide", ent, thr3, lab_l, lab_u, 255, B, S, S, s, s, 1, C, tw, kw, loww, highw, bitsw)
    want = k["planes"].reshape(1, n)
    assert torch.equal(tn, tw) and torch.equal(kn, kw) and torch.equal(lown, loww) and torch.equal(highn, highw)
    assert torch.equal(bitsw[0], bitsn)
    assert np.array_equal(bitsn.cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(bitsw.cpu().numpy().view(np.uint32), want)
    if C == 32:
        assert (bitsn.cpu().numpy().view(np.uint32) >> np.uint32(31)).any()
    with np.errstate(invalid="ignore"):
        t_want = np.where(k["ent"] >= k["thr3"][0], 255, k["lab_u"])
    assert np.array_equal(tn.cpu().numpy(), t_want) and int(kn) == int((t_want != 255).sum()) and 0 < int(kn) < t_want.size
    assert 0 < float(lown.sum()) < n and 0 < float(highn.sum()) < n
    _, _, low2n, high2n, bits2n = outputs(0)
    _, _, low2w, high2w, bits2w = outputs(1)
    H.call("u2pl_reliability_masks", ent, thr3[1:2], thr3[2:3], lab_l, lab_u, 255, B, S, S, s, s, 0, low2n, high2n, bits2n)
    H.call("u2pl_reliability_masks_wide", ent, thr3[1:2], thr3[2:3], lab_l, lab_u, 255, B, S, S, s, s, 0, C, low2w, high2w,
           bits2w)
    assert torch.equal(low2n, low2w) and torch.equal(high2n, high2w) and torch.equal(bits2w[0], bits2n)
    assert torch.equal(bits2n, bitsn) and torch.equal(low2n, lown)
    assert torch.equal(high2n[:B], highn[:B]) and bool((high2n[B:] == 1).all())       # negative_high_entropy = 0: all ones


@pytest.mark.parametrize("C", SHARED_C)
def test_pack_and_unpack_one_word_and_plane_forms_agree(C):
    """pack_class_bits(wide=False) against wide=True (three blocks of pixels): the one plane == the word == the numpy
    planes, and unpack of either returns the input"""
    H = hip()
    gen = torch.Generator(device=DEV).manual_seed(C)
    oh = (torch.rand(3, C, 17, 17, device=DEV, generator=gen) < 0.3).long()
    oh[0, C - 1, 0, 0] = 1
    narrow, wide = H.pack_class_bits(oh, wide=False), H.pack_class_bits(oh, wide=True)
    assert narrow.shape == (3, 17, 17) and wide.shape == (1, 3, 17, 17)
    assert torch.equal(wide[0], narrow)
    assert np.array_equal(wide.cpu().numpy().view(np.uint32), WR.planes_from_onehot(oh.cpu().numpy()))
    assert torch.equal(H.unpack_class_bits(narrow, C), oh) and torch.equal(H.unpack_class_bits(wide, C), oh)


@pytest.mark.parametrize("C", [1, 19, 32])
def test_bank_entries_for_32_and_255_classes_agree(C):
    """u2pl_bank_init / u2pl_bank_enqueue_f32 on a [C][stride] list array against the _wide entries on the same array
    flattened with list_off[c] = c * stride: state and storage bit-equal after init and after each of three enqueues
    whose counts cover 0, exactly cap, more than cap (only the last cap rows survive) and a wrap of the ring, then one
    enqueue with idx = NULL and row_start; both equal the host mirror (head, length, pointer) and a FIFO of torch rows."""
    H = hip()
    D, stride, nrows = 8, 70, 200
    caps = [(3, 5, 64)[c % 3] for c in range(C)]
    seq = lambda c, cap: ([0, cap + 2, cap], [cap - 1, 2, cap + 3], [cap, 0, cap - 1])[(c // 3) % 3]
    steps = [[seq(c, caps[c])[i] for c in range(C)] for i in range(3)]
    assert 0 in sum(steps, []) and max(max(st) for st in steps) <= stride
    gen = torch.Generator().manual_seed(C)
    rows = torch.randn(nrows, D, generator=gen)
    rows_d = rows.to(DEV)
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    caps_np = np.array(caps, dtype=np.int64)
    state = [torch.full((C, 5), -1, dtype=torch.int64, device=DEV) for _ in range(2)]
    store = [torch.zeros((int(offs[-1]), D), device=DEV) for _ in range(2)]
    H.call("u2pl_bank_init", state[0], C, caps_np.ctypes.data)
    H.call("u2pl_bank_init_wide", state[1], C, caps_np.ctypes.data)
    assert torch.equal(state[0], state[1])
    assert state[0].cpu().numpy().tolist() == [[int(offs[c]), caps[c], 0, 0, 0] for c in range(C)]
    mirror = H.DeviceMemoryBank(C, caps, feat_dim=D, device="cpu")           # host bookkeeping only
    fifo = [torch.zeros(0, D) for _ in caps]
    list_off = torch.arange(C, dtype=torch.int64, device=DEV) * stride
    row_start = torch.arange(C, dtype=torch.int64) * 3 + 5
    seen = set()
    for step, cnts in enumerate(steps + [[(c + 2) % 4 for c in range(C)]]):
        for c in range(C):      # what this count exercises, from the mirror's ring position before it
            tail = (mirror.head[c] + mirror.length[c]) % caps[c]
            seen |= {"zero"} if cnts[c] == 0 else {"cap"} if cnts[c] == caps[c] else {"over"} if cnts[c] > caps[c] else set()
            seen |= {"wrap"} if 0 < cnts[c] < caps[c] and tail + cnts[c] > caps[c] else set()
        cnt_d = torch.tensor(cnts, dtype=torch.int32, device=DEV)
        if step < 3:
            idx = torch.randint(0, nrows, (C, stride), generator=gen, dtype=torch.int32)
            src = [idx[c, :cnts[c]].long() for c in range(C)]
            idx_d = idx.to(DEV)
            H.call("u2pl_bank_enqueue_f32", state[0], store[0], D, rows_d, D, idx_d, stride, None, cnt_d, C)
            H.call("u2pl_bank_enqueue_wide_f32", state[1], store[1], D, rows_d, D, idx_d.reshape(-1), list_off, None, cnt_d, C)
        else:
            src = [int(row_start[c]) + torch.arange(cnts[c]) for c in range(C)]
            H.call("u2pl_bank_enqueue_f32", state[0], store[0], D, rows_d, D, None, 0, row_start.to(DEV), cnt_d, C)
            H.call("u2pl_bank_enqueue_wide_f32", state[1], store[1], D, rows_d, D, None, None, row_start.to(DEV), cnt_d, C)
        mirror.mirror_counts(cnts)
        assert torch.equal(state[0], state[1]), step
        assert torch.equal(store[0].view(torch.int32), store[1].view(torch.int32)), step
        st = state[0].cpu().numpy()
        assert st[:, 2].tolist() == mirror.head and st[:, 3].tolist() == mirror.length and st[:, 4].tolist() == mirror.ptr
        got = store[0].cpu()
        for c in range(C):
            fifo[c] = torch.cat((fifo[c], rows[src[c]]))[-caps[c]:]
            ring = (mirror.head[c] + np.arange(mirror.length[c])) % caps[c] + int(offs[c])
            assert torch.equal(got[ring], fifo[c]), (step, c)
    assert seen >= ({"zero", "cap", "over"} | ({"wrap"} if C > 3 else set())), seen


# ------------------------------------------------------------------ 4. unchanged calls at C <= 32
@pytest.mark.parametrize("C", [19, 32])
def test_up_to_32_classes_make_the_narrow_calls_only(C, monkeypatch):
    H = hip()
    names = []
    orig_call = H.call

    def rec(name, *a):
        names.append(name)
        return orig_call(name, *a)
    monkeypatch.setattr(H, "call", rec)
    from u2pl_amd.utils.loss_helper import compute_contra_memobank_loss
    g, k = _prefill_inputs(C)
    D, B = k["D"], k["B"]
    bank = H.DeviceMemoryBank(C, k["qs"], D, DEV)
    for c in range(C):
        bank.load_logical(c, formula_bank(c, k["fill"][c], D).to(DEV))
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    prob = T(k["prob"])
    rep = T(g["s0_rep"]).requires_grad_(True)
    torch.set_rng_state(torch.from_numpy(g["s0_rng_state"]))
    _, loss = compute_contra_memobank_loss(
        rep, T(k["ll"], torch.int64), T(k["lu"], torch.int64), prob[:B], prob[B:], T(g["s0_low_mask_all"], torch.float32),
        T(g["s0_high_mask_all"], torch.float32), CONTRA_CFG, bank, ptrs, k["qs"], T(g["s0_rep_teacher"]))
    loss.backward()
    contra = list(names)
    assert contra[:2] == ["u2pl_pack_class_bits", "u2pl_contra_phase1"], contra
    assert contra[2:] == ["u2pl_bank_append_multi_f32", "u2pl_infonce_fused_f32", "u2pl_scatter_rows_ordered_f32"] or \
        contra[2:] == ["u2pl_bank_append_multi_f32", "u2pl_infonce_fused_f32", "u2pl_zero_rows_f32", "u2pl_scatter_rows_ordered_f32"], contra
    del names[:]
    gen = torch.Generator(device=DEV).manual_seed(C)
    s, S = 17, 65
    logits = torch.randn(2, C, s, s, device=DEV, generator=gen) * 3
    lab = torch.randint(0, C, (2, 2, S, S), device=DEV, generator=gen)
    rs = H.reliability_split(logits, (S, S), lab[0], lab[1], (s, s), [80.0, 20.0, 80.0])
    torch.cuda.synchronize()
    assert rs["lbits"].shape == (4, s, s)
    unfused = ["u2pl_entropy_up_f32", "u2pl_select_f32", "u2pl_reliability_apply"]
    assert names == unfused or (C == 19 and names == ["u2pl_reliability_fused"]), names     # (the persistent split: C in {19, 21})
    assert not any("_wide" in n for n in contra + names)


# ------------------------------------------------------------------ 5. determinism
def test_wide_route_is_bit_reproducible():
    a, banks_a = _run_fixture("c150s", "device_bank", check=False)
    b, banks_b = _run_fixture("c150s", "device_bank", check=False)
    for (la, ga), (lb, gb) in zip(a, b):
        assert la.tobytes() == lb.tobytes() and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    for x, y in zip(banks_a, banks_b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_wide_device_enqueue_equals_the_host_sized_append(monkeypatch):
    """u2pl_bank_enqueue_wide_f32 (list lengths and offsets on the device) leaves the banks of the default append"""
    from u2pl_amd.utils import loss_helper as LH
    _, want = _run_fixture("c40s", "device_bank", check=False)
    monkeypatch.setattr(LH, "DEVICE_ENQUEUE", True)
    _, got = _run_fixture("c40s", "device_bank", check=True)
    for x, y in zip(want, got):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 6 / 7. the whole step at 40 classes
def _inputs(B, S, C, seed):
    g = torch.Generator().manual_seed(seed)
    il, iu = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 3, S, S, generator=g)
    gsz = (S + 7) // 8
    coarse = torch.randint(0, C, (B, gsz, gsz), generator=g)
    iy = (torch.arange(S) // 8).clamp(max=gsz - 1)
    ll = coarse[:, iy][:, :, iy].contiguous()
    ll[:, :6] = 255
    return il, ll, iu


def _cfg40(S):
    from u2pl_amd import configs
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=2, sync_bn=False, epochs=20, num_classes=40)
    cfg["criterion"]["kwargs"]["min_kept"] = 2000
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.026     # near-uniform softmax at init (1 / 40): exercise InfoNCE
    return cfg


def test_train_step_with_40_classes_matches_cpu_port():
    """R50, S = 65, 40 classes, aux + OHEM + CutMix: two steps against oracle.step_ref.CpuStepRef(num_classes=40), with the
    assertions of test_train_step_matches_cpu_port for its Winograd-default mode: losses (step 0 against the fp32 port at 1e-4;
    step 1 against the float64 arbiter, k = 8, and the fixed caps), labels / target / low / high masks, the unsupervised loss on
    the port's pixel set, the parameters after the updates; plus the wide label bits unpacked against label_onehot.  Then
    engine.validate on four images against validate_ref.  (ent_err is printed, as there: that test asserts nothing on it.)"""
    from oracle.step_ref import CpuStepRef, validate_ref
    from u2pl_amd import engine
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    H = hip()
    B, C, S = 2, 40, 65
    cfg = _cfg40(S)
    torch.manual_seed(0)
    model, teacher = ModelBuilder(cfg["net"]), ModelBuilder(cfg["net"])
    sd = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items()}
    model.load_state_dict(sd), teacher.load_state_dict(sd)
    from oracle.parity_dropout import KeyedMasks, tag_model
    from u2pl_amd import nn as Kn
    tag_model(model, "student"), tag_model(teacher, "teacher")      # dropout ON, both sides draw their keep-masks from KeyedMasks
    Kn.DROPOUT_HOOK = KeyedMasks(11).hook
    model, teacher = model.to(DEV), teacher.to(DEV)
    tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=5)
    contra = copy.deepcopy(cfg["trainer"]["contrastive"])
    mk = lambda dt: CpuStepRef(arch="resnet50", num_classes=C, aux=True, epochs=20, steps_per_epoch=5, ohem=(0.7, 2000), p_drop=0.1,
                               contra=copy.deepcopy(contra), state_dict={k: v.clone() for k, v in sd.items()},
                               dropout_masks=KeyedMasks(11), dtype=dt)
    ref, arb = mk(torch.float32), mk(torch.float64)
    rnd = lambda seed: (lambda g: (lambda hi, n: torch.randint(hi, size=(n,), generator=g)))(torch.Generator().manual_seed(seed))
    report = []
    for step in range(2):
        il, ll, iu = _inputs(B, S, C, 100 + step)
        outs = []
        for side in (ref, arb):
            np.random.seed(7 + step)
            f = rnd(50 + step)
            outs.append(side.step(il, ll, iu, 0, randint=lambda hi, n, f=f: f(hi, n).numpy()))
        o, o64 = outs
        np.random.seed(7 + step)
        dbg = {}
        m = [float(x) for x in tr.train_step(il.to(DEV), ll.to(DEV), iu.to(DEV), 0, randint=rnd(50 + step), debug=dbg).cpu()]
        assert dbg["lbits"].dim() == 4 and dbg["lbits"].shape[:2] == (2, 2 * B)          # two word planes
        npy = lambda k: dbg[k].cpu().numpy()
        lab_eq = float((npy("label_u") == o["label_u"]).mean())
        tgt_eq = float((npy("target_u") == o["new_target"]).mean())
        low_eq = float((npy("low_mask") == o["low_mask"]).mean())
        high_eq = float((npy("high_mask") == o["high_mask"]).mean())
        n_diff = int((npy("label_u") != o["label_u"]).sum() + (npy("target_u") != o["new_target"]).sum()
                     + (npy("low_mask") != o["low_mask"]).sum() + (npy("high_mask") != o["high_mask"]).sum())
        ent_err = float(np.nanmax(np.abs(np.where(np.isnan(npy("entropy")), o["entropy"], npy("entropy")) - o["entropy"])))
        # the wide label bits, unpacked: exactly label_onehot (slot-0 quirk, legacy nearest) of the labels this step used,
        # and, pixel for pixel, of the port's labels (they differ only where the pseudo-labels do)
        hm, wm = dbg["lbits"].shape[2:]
        oh = H.unpack_class_bits(dbg["lbits"], C).cpu().numpy()
        own = np.concatenate([R.nearest_down(R.label_onehot_quirk(ll.numpy(), C), hm, wm),
                              R.nearest_down(R.label_onehot_quirk(npy("label_u"), C), hm, wm)]).astype(np.int64)
        port = np.concatenate([own[:B], R.nearest_down(R.label_onehot_quirk(o["label_u"], C), hm, wm).astype(np.int64)])
        assert np.array_equal(oh, own)
        lbits_px = int((oh != port).any(1).sum())
        tgt_port = torch.from_numpy(np.asarray(o["new_target"])).long()
        unsup_same_px = float(torch.nn.functional.cross_entropy(dbg["pred_u_large"].float().cpu(), tgt_port, ignore_index=255)
                              * (tgt_port.numel() / max(int((tgt_port != 255).sum()), 1)))
        r = dict(step=step, hip=m, ref=[o["sup"], o["unsup"], o["contra"]], f64=[o64["sup"], o64["unsup"], o64["contra"]],
                 njobs=o["contra_info"]["njobs"], keys_hip=sum(map(int, tr.memobank.length)),
                 keys_ref=sum(b[0].shape[0] for b in ref.bank), lab_eq=lab_eq, tgt_eq=tgt_eq, low_eq=low_eq, high_eq=high_eq,
                 mask_px_differing=n_diff, ent_err=ent_err, lbits_px_differing=lbits_px, unsup_same_px=unsup_same_px,
                 coin=o["coin"])
        print(r)
        report.append(r)
    for r in report:
        for k_, (a, b, c64) in enumerate(zip(r["hip"], r["ref"], r["f64"])):
            if r["step"] == 0:
                assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), r
            e_hip, e_port = abs(a - c64), abs(b - c64)
            assert e_hip <= 8.0 * e_port + 1e-6 + (2e-4 * max(1.0, abs(c64)) if r["step"] else 0.0), (k_, e_hip, e_port, r)
            assert abs(a - b) <= (2e-3, 6e-3, 2e-3)[k_] * max(1.0, abs(b)), (k_, r)
        b = r["ref"][1]
        if r["step"] == 0:
            assert abs(r["unsup_same_px"] - b) <= 1e-4 * max(1.0, abs(b)), r
            # identical weights, Winograd F(4x4) default: test_train_step_matches_cpu_port's bound on labels / target / masks
            assert r["mask_px_differing"] <= 8 and r["lbits_px_differing"] <= 8, r
        else:
            assert abs(r["unsup_same_px"] - b) <= 6e-3 * max(1.0, abs(b)), r
            assert r["lab_eq"] > 0.999 and r["tgt_eq"] > 0.995 and r["low_eq"] > 0.995 and r["high_eq"] > 0.995, r
    assert report[0]["njobs"] > 0 and abs(report[0]["keys_hip"] - report[0]["keys_ref"]) <= 2
    # parameters after the two optimizer steps + EMA stay close, relative to the size of the update (the backward pass)
    sref, worst = ref.student.state_dict(), {}
    for k in ["encoder.conv1.0.weight", "decoder.classifier.8.weight", "encoder.layer3.2.bn2.weight", "auxor.aux.4.bias",
              "encoder.layer4.2.conv3.weight", "decoder.aspp.conv4.0.weight"]:
        a = dict(model.named_parameters())[k].detach().cpu()
        worst[k] = ((a - sref[k]).abs().max().item(), (sref[k] - sd[k]).abs().max().item())
    a = dict(teacher.named_parameters())["decoder.classifier.8.weight"].detach().cpu()
    terr = (a - ref.teacher.state_dict()["decoder.classifier.8.weight"]).abs().max().item()
    print("param (err, update)", worst, "teacher err", terr)
    for k, (err, upd) in worst.items():
        assert err <= 0.15 * upd + 1e-6, (k, err, upd)
    assert terr <= 0.05 * worst["decoder.classifier.8.weight"][1] + 1e-6
    g = torch.Generator().manual_seed(9)
    batches = [(torch.randn(2, 3, S, S, generator=g), torch.randint(0, C, (2, S, S), generator=g)) for _ in range(2)]
    Kn.DROPOUT_HOOK = None
    model.load_state_dict(ref.student.state_dict())      # the same weights on both sides: validate() itself is under test
    miou, iou = engine.validate(model, batches, cfg, DEV)
    miou_ref, iou_ref = validate_ref(ref.student, batches, C)
    print("mIoU", miou, miou_ref)
    assert abs(miou - miou_ref) <= 2e-3 and np.abs(iou - iou_ref).max() <= 2e-2


def _graph_run(monkeypatch, graphs_on, steps=4, S=65, C=40):
    from u2pl_amd import graphs as G
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    monkeypatch.setenv("U2PL_GRAPHS", "1" if graphs_on else "0")
    cfg = _cfg40(S)
    torch.manual_seed(0)
    model, teacher = ModelBuilder(copy.deepcopy(cfg["net"])), ModelBuilder(copy.deepcopy(cfg["net"]))
    teacher.load_state_dict(model.state_dict())
    model, teacher = model.to(DEV), teacher.to(DEV)
    tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=4)
    g = torch.Generator().manual_seed(5)
    stats0 = dict(G.STATS)
    meters = []
    for step in range(steps):
        il, iu = torch.randn(2, 3, S, S, generator=g), torch.randn(2, 3, S, S, generator=g)
        ll = torch.randint(0, C, (2, S, S), generator=g)
        ll[:, :6] = 255
        np.random.seed(30 + step)
        torch.manual_seed(40 + step)
        torch.cuda.manual_seed(50 + step)
        meters.append(tr.train_step(il.to(DEV), ll.to(DEV), iu.to(DEV), epoch=0).cpu().numpy())
    torch.cuda.synchronize()
    return dict(meters=np.stack(meters), w=tr.arena.flat.clone(), bank_len=[int(x) for x in tr.memobank.length],
                stats={k: G.STATS[k] - stats0[k] for k in stats0})


def test_graph_replay_equals_eager_with_40_classes(monkeypatch):
    """the C = 19 graph test's claim (test_graph_replay_steps_are_bit_identical_to_eager_steps) at 40 classes: replayed and
    eager steps give the same loss bits, weights and bank lengths"""
    a, b = _graph_run(monkeypatch, True), _graph_run(monkeypatch, False)
    assert a["stats"]["replays"] > 0 and b["stats"]["replays"] == 0 and a["stats"]["aborted"] == 0
    assert np.array_equal(a["meters"], b["meters"]), (a["meters"], b["meters"])
    assert torch.equal(a["w"], b["w"]) and a["bank_len"] == b["bank_len"] and sum(a["bank_len"]) > 0


# ------------------------------------------------------------------ 9. limits
def test_class_count_limits():
    """255 classes run (also test_wide_stages_equal_the_numpy_restatement[255] and the c255 fixture); 256 is a ValueError
    at construction; the narrow entry points still answer U2PL_EINVAL at C = 33"""
    from u2pl_amd import _lib, configs
    from u2pl_amd.trainer import SemiTrainer
    H = hip()
    C, s = 255, 5
    gen = torch.Generator(device=DEV).manual_seed(1)
    oh = (torch.rand(4, C, s, s, device=DEV, generator=gen) < 0.02).long()
    lbits = H.pack_class_bits(oh)
    assert lbits.shape == (8, 4, s, s) and torch.equal(H.unpack_class_bits(lbits, C), oh)
    bank = H.DeviceMemoryBank(C, [8] * C, 64, DEV)
    assert len(bank) == 255
    with pytest.raises(ValueError, match="too many classes"):
        SemiTrainer(configs.cityscapes_semi(arch="resnet50", crop=65, batch_size=2, sync_bn=False, num_classes=256), None, None,
                    None, steps_per_epoch=2)
    with pytest.raises(ValueError, match="too many classes"):
        H.pack_class_bits(torch.zeros(1, 256, s, s, dtype=torch.long, device=DEV))
    z = torch.zeros(4096, device=DEV)
    zi = torch.zeros(4096, dtype=torch.int32, device=DEV)
    for name, args in (("u2pl_pack_class_bits", (zi.long(), 1, 33, 2, 2, zi)),
                       ("u2pl_contra_classify", (z, 132, 1, 33, zi, z, z, 1, 1, 33, 2, 2, 0.3, 1.0, 3, 20, zi, zi, zi, zi)),
                       ("u2pl_compact_lists", (zi, zi, zi, 4, 33, zi, zi, 4, zi, 0)),
                       ("u2pl_bank_enqueue_f32", (zi.long(), z, 4, z, 4, zi, 4, None, zi, 33))):
        with pytest.raises(_lib.HipError, match="1001"):
            _lib.call(name, *args)
