"""-m gpu: the contrastive sampling planned on the device (u2pl_infonce_plan, u2pl_infonce_fused_dev_f32,
u2pl_scatter_rows_ordered_dev_f32) against the host path it replaces.  Same generator state -> the same job table, the
same draws, the same grouping, the same loss and gradient BITS, the same bank, the same generator afterwards."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden
from oracle.gen_golden import CONTRA_CFG, formula_bank

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = ["65_empty", "65_prefill", "65_t007", "65_t001", "65_wrap"]
C19 = 19


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def mods():
    from u2pl_amd import hipops as H, rng_words as RW
    from u2pl_amd.utils import loss_helper as LH
    return H, LH, RW


def _host_tables(H, rep_rows, ph1, bank, counts, cfg, randint=None):
    """what infonce_loss / group_entries build on the host for this ph1 / bank / generator state: (loss or None, tables)"""
    valid = [i for i in range(ph1.C) if counts[1][i] > 0]
    saved, H.REPLAY = H.REPLAY, {}
    try:
        loss = H.infonce_loss(rep_rows, ph1, bank, valid, counts, cfg, randint) if len(valid) > 1 else None
        rec = H.REPLAY.get("infonce")
    finally:
        H.REPLAY = saved
    if loss is None:
        return None, dict(njobs=0, valid_seg=len(valid))
    _, jobs_dev, njobs, Q, K, _, valid_seg, groups, keep = rec
    idx_all = keep[0]
    jb = jobs_dev.cpu().numpy().copy()
    jb[:, 1] -= idx_all.data_ptr()           # the two index pointers as byte offsets into the index buffer
    jb[:, 2] -= idx_all.data_ptr()
    return loss, dict(njobs=njobs, valid_seg=valid_seg, jobs=jb, idx=idx_all.cpu().numpy(), groups=groups.cpu().numpy())


def _device_tables(plan, njobs, Q):
    per = plan["per"]
    jb = plan["jobs"].cpu().numpy()[:njobs].copy()
    jb[:, 1] -= plan["idx"].data_ptr()
    jb[:, 2] -= plan["idx"].data_ptr()
    return dict(jobs=jb, idx=plan["idx"].cpu().numpy().reshape(-1)[:njobs * per],
                groups=plan["groups"].cpu().numpy().reshape(3, -1)[:, :njobs * Q])


def _compare_tables(host, plan, H, Q):
    counts, njobs, valid_seg = H.plan_mirror(plan)
    assert (njobs, valid_seg) == (host["njobs"], host["valid_seg"]), (njobs, valid_seg, host["njobs"], host["valid_seg"])
    hdr = plan["hdr"].cpu().numpy()
    assert hdr[0] == njobs and hdr[1] == valid_seg and hdr[4] == njobs * Q
    if njobs:
        dev = _device_tables(plan, njobs, Q)
        assert hdr[2:4].view(np.float32).tolist() == [np.float32(1.0 / valid_seg), np.float32(1.0 / (Q * valid_seg))]
        for k in ("jobs", "idx", "groups"):
            assert dev[k].dtype == host[k].dtype and dev[k].tobytes() == host[k].tobytes(), k
    apix = plan["apix"].cpu().numpy()
    assert (apix[njobs:] == -1).all()
    return counts, njobs, valid_seg


def _bank(H, C, D, caps, lens, heads=None):
    bank = H.DeviceMemoryBank(C, caps, D, DEV)
    for c in range(C):
        if lens[c]:
            bank.load_logical(c, formula_bank(c, lens[c], D).to(DEV))
            if heads is not None and heads[c]:       # the same logical rows, rotated: logical row j at slot (head + j) % cap
                assert lens[c] == caps[c]
                bank.buf[c].copy_(torch.roll(bank.buf[c].clone(), heads[c], 0))
                bank.head[c] = heads[c]
    bank._state_stale = True
    bank._sync_state()
    return bank


# ------------------------------------------------------------------ 1. the fixtures: plan tables, loss and gradient bits, bank, generator
@pytest.mark.parametrize("tag", TAGS)
def test_device_sampling_equals_host_sampling_on_the_fixtures(tag):
    """every step of a contra_65 fixture through contra_memobank_core on the device path (defer=True) and on the host
    path (two banks): the plan's job table (index pointers as offsets), draws and grouping arrays equal the host's bytes;
    loss and rep gradient bit for bit; bank rows, length / head / ptr, LAST_STATS and the generator state equal after
    every step.  65_t001 takes the running-maximum kernel, 65_wrap samples from rings with head != 0."""
    H, LH, RW = mods()
    g = golden("contra_" + tag)
    D = int(g["D"])
    qs = [int(x) for x in g["queue_size"]]
    pre = int(g["prefill"])
    fill = [int(x) for x in g["fill"]] if "fill" in g else [pre + 3 * c for c in range(C19)]
    cfg = dict(CONTRA_CFG, temperature=float(g["temperature"])) if "temperature" in g else dict(CONTRA_CFG)
    Q = int(cfg["num_queries"])
    banks = [_bank(H, C19, D, qs, fill if pre else [0] * C19) for _ in range(2)]
    with_jobs = 0
    for st in range(int(g["num_steps"])):
        p = f"s{st}_"
        B = g[p + "label_l"].shape[0]
        prob = T(g[p + "prob_all"])
        fmt = torch.channels_last if st else torch.contiguous_format
        lbits = H.pack_class_bits(torch.cat((T(g[p + "label_l_small"], torch.int64), T(g[p + "label_u_small"], torch.int64))))
        rep_t = T(g[p + "rep_teacher"]).contiguous(memory_format=fmt)
        lo, hi = T(g[p + "low_mask_all"], torch.float32), T(g[p + "high_mask_all"], torch.float32)
        res = []
        for defer in (True, False):
            rep = T(g[p + "rep"]).contiguous(memory_format=fmt).requires_grad_(True)
            torch.set_rng_state(torch.from_numpy(g[p + "rng_state"]))
            new_keys, loss = LH.contra_memobank_core(rep, lbits, B, prob[:B], prob[B:], lo, hi, cfg, banks[0 if defer else 1],
                                                     rep_t, defer=defer)
            assert H.host_read_pending() == defer and (new_keys is None) == defer
            loss.backward()
            if defer:
                plan = H.infonce_loss_device.last_plan
            LH.settle_sampling()
            assert not H.host_read_pending()
            res.append(dict(loss=loss.detach().cpu().numpy().copy(), grad=rep.grad.cpu().numpy().copy(),
                            stats=dict(LH.LAST_STATS), rng=torch.get_rng_state().clone(), rep=rep))
        d, h = res
        print(tag, "step", st, "loss", float(d["loss"]), float(h["loss"]), "stats", d["stats"])
        assert d["loss"].tobytes() == h["loss"].tobytes()
        assert d["grad"].tobytes() == h["grad"].tobytes()
        assert d["stats"] == h["stats"]
        assert torch.equal(d["rng"], h["rng"])
        for a in ("length", "head", "ptr"):
            assert getattr(banks[0], a) == getattr(banks[1], a), a
        assert torch.equal(banks[0].storage, banks[1].storage)
        # the plan's tables against the host builder on the SAME phase-1 object and bank, from the step's generator state
        counts = H.plan_mirror(plan)[0]
        torch.set_rng_state(torch.from_numpy(g[p + "rng_state"]))
        rep2 = T(g[p + "rep"]).contiguous(memory_format=fmt).requires_grad_(True)
        loss2, host = _host_tables(H, LH._rows_view(rep2), plan["ph1"], banks[0], counts, cfg)
        _, njobs, _ = _compare_tables(host, plan, H, Q)
        assert njobs == int(g[p + "njobs"]) if (p + "njobs") in g else True
        if loss2 is not None:
            loss2.backward()
            assert loss2.detach().cpu().numpy().tobytes() == d["loss"].tobytes()
            assert rep2.grad.cpu().numpy().tobytes() == d["grad"].tobytes()
            with_jobs += 1
        else:
            assert float(d["loss"]) == 0.0 and not d["grad"].any()
        torch.set_rng_state(d["rng"])
    assert with_jobs > 0 or tag == "65_empty"


# ------------------------------------------------------------------ 2. hand-made list lengths and rings
P_HAND, D_HAND = 300, 64


def _hand_case(name):
    """-> counts [3][32], bank caps, lengths, heads, words (or None: the generator's)"""
    C = C19
    c0, c1 = np.zeros(32, np.int64), np.zeros(32, np.int64)
    caps, lens, heads, words = [40] * C, [17 + c for c in range(C)], None, None
    per = 256 + 256 * 50
    if name == "no_valid_class":
        c0[:C] = 5
    elif name == "one_valid_class":
        c0[:C] = 7
        c1[4] = 3
    elif name == "all_valid":
        c0[:C] = [1 + 13 * i for i in range(C)]
        c1[:C] = 2
    elif name == "valid_class_with_empty_bank":
        c0[:C] = 50
        c1[[1, 5, 6, 11]] = 9
        lens[5] = 0                      # position 1 (class 5): no job, no words; positions 2 and 3 keep their offsets
    elif name == "position_is_not_class":
        c0[:3] = [11, 0, 23]             # candidates by POSITION: position 1 has none although class 9 is valid
        c1[[7, 9, 16]] = 1
    elif name == "ring_at_capacity_head_nonzero":
        c0[:C] = 31
        c1[:C] = 1
        lens = list(caps)
        heads = [(3 + 5 * c) % 40 for c in range(C)]
    elif name == "all_anchors_equal":
        c0[:C] = 200
        c1[[2, 3]] = 1
        words = np.arange(C * per, dtype=np.uint32) * np.uint32(2654435761)
        for j in range(2):
            words[j * per:j * per + 256] = 200 * 7 + 123          # every anchor draw: candidate 123
    elif name == "all_anchors_distinct":
        c0[:C] = 256
        c1[[0, 18]] = 1
        words = np.arange(C * per, dtype=np.uint32) * np.uint32(40503)
        for j in range(2):
            words[j * per:j * per + 256] = (np.arange(256, dtype=np.uint32)[::-1] * 3 + 1) % 256 + 256 * np.arange(256, dtype=np.uint32)
    else:
        raise KeyError(name)
    return np.stack([c0, c1, np.zeros(32, np.int64)]), caps, lens, heads, words


HAND = ["no_valid_class", "one_valid_class", "all_valid", "valid_class_with_empty_bank", "position_is_not_class",
        "ring_at_capacity_head_nonzero", "all_anchors_equal", "all_anchors_distinct"]


@pytest.mark.parametrize("name", HAND)
def test_plan_on_hand_made_lengths(name):
    """u2pl_infonce_plan + the device-header InfoNCE forward / ordered scatter on list lengths and rings made by hand
    (every list entry a valid pixel, every length <= the list's capacity): tables equal the host builder's bytes, loss
    and gradient equal the host launch's bits; with at most one valid class or no job the loss is exactly 0.0 and the
    gradient all zeros, and no word is consumed."""
    H, LH, RW = mods()
    cfg = dict(CONTRA_CFG)
    Q, K = int(cfg["num_queries"]), int(cfg["num_negatives"])
    counts, caps, lens, heads, words = _hand_case(name)
    gen = torch.Generator().manual_seed(11)
    ph1 = H.ContraPhase1()
    ph1.wide, ph1.C, ph1.cap, ph1.offsets, ph1.offsets_host, ph1.bits, ph1._fin = False, C19, P_HAND, None, None, None, None
    ph1.idx = torch.randint(0, P_HAND, (3, H.MAXC, P_HAND), generator=gen, dtype=torch.int32).to(DEV)
    ph1.counts = T(counts.astype(np.int32))
    ph1.proto = (torch.rand((C19, D_HAND), generator=gen) - 0.5).to(DEV)
    ph1.counts_host = counts
    assert counts.max() <= P_HAND
    bank = _bank(H, C19, D_HAND, caps, lens, heads)
    rep_src = torch.randn((P_HAND, D_HAND), generator=gen)
    torch.manual_seed(123)
    torch.randint(5, (77,))
    s0 = torch.get_rng_state().clone()
    rep_d = rep_src.to(DEV).requires_grad_(True)
    loss_d, plan = H.infonce_loss_device(rep_d, ph1, bank, cfg, words=words)
    loss_d.backward()
    grad_d = rep_d.grad.cpu().numpy().copy()               # (the gradient may BE the persistent row-sparse buffer: copy it now)
    loss_d_bits = loss_d.detach().cpu().numpy().tobytes()
    assert torch.equal(s0, torch.get_rng_state())          # the plan only peeks
    feed = None
    if words is not None:
        state = {"o": 0}

        def feed(high, n):
            r = torch.from_numpy(RW.randint_from_words(words[state["o"]:], high, n))
            state["o"] += n
            return r
    rep_h = rep_src.to(DEV).requires_grad_(True)
    loss_h, host = _host_tables(H, rep_h, ph1, bank, counts, cfg, feed)
    _, njobs, valid_seg = _compare_tables(host, plan, H, Q)
    print(name, "njobs", njobs, "valid_seg", valid_seg, "loss", float(loss_d.detach()))
    expect = {"no_valid_class": (0, 0), "one_valid_class": (0, 1), "all_valid": (19, 19), "valid_class_with_empty_bank": (3, 4),
              "position_is_not_class": (2, 3), "ring_at_capacity_head_nonzero": (19, 19), "all_anchors_equal": (2, 2),
              "all_anchors_distinct": (2, 2)}[name]
    assert (njobs, valid_seg) == expect
    if loss_h is None:
        assert loss_d_bits == np.float32(0.0).tobytes()
        assert rep_d.grad is not None and grad_d.shape == (P_HAND, D_HAND) and not grad_d.any()
        assert torch.equal(s0, torch.get_rng_state())
        return
    loss_h.backward()
    assert loss_d_bits == loss_h.detach().cpu().numpy().tobytes()
    assert grad_d.tobytes() == rep_h.grad.cpu().numpy().tobytes()
    assert grad_d.any()
    if words is None:       # the host drew njobs * (Q + Q K) words from the generator; advancing by as many lands there too
        s_host = torch.get_rng_state().clone()
        torch.set_rng_state(s0)
        RW.advance(njobs * (Q + Q * K))
        assert torch.equal(s_host, torch.get_rng_state())
    grp = plan["groups"].cpu().numpy().reshape(3, -1)
    if name == "all_anchors_equal":
        assert grp[2, 0] == Q and not grp[2, 1:Q].any() and grp[2, Q] == Q
    if name == "all_anchors_distinct":
        assert (grp[2, :2 * Q] == 1).all()
    if name == "ring_at_capacity_head_nonzero":
        assert all(h != 0 for h in bank.head) and bank.length == caps


# ------------------------------------------------------------------ 3. whole steps
def _train(monkeypatch, device_sampling, steps=3, S=65):
    from u2pl_amd import configs, engine
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    H, LH, RW = mods()

    monkeypatch.setattr(LH, "DEVICE_SAMPLING", device_sampling)
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=2, sync_bn=False, epochs=20)
    cfg["criterion"]["kwargs"]["min_kept"] = 1500
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    torch.manual_seed(0)
    model, teacher = ModelBuilder(copy.deepcopy(cfg["net"])), ModelBuilder(copy.deepcopy(cfg["net"]))
    teacher.load_state_dict(model.state_dict())
    model, teacher = model.to(DEV), teacher.to(DEV)
    tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=2)     # (sup_only_epoch = 0: every step is semi-supervised)
    g = torch.Generator().manual_seed(5)
    np.random.seed(30)
    torch.manual_seed(40)
    torch.cuda.manual_seed(50)
    out = dict(meters=[], mirrors=[], stats=[], deferred=[])
    for step in range(steps):
        il, iu = torch.randn(2, 3, S, S, generator=g), torch.randn(2, 3, S, S, generator=g)
        ll = torch.randint(0, 19, (2, S, S), generator=g)
        ll[:, :6] = 255
        seen = []
        orig = H.defer_host_read
        monkeypatch.setattr(H, "defer_host_read", lambda fn: (seen.append(1), orig(fn))[1])
        out["meters"].append(tr.train_step(il.to(DEV), ll.to(DEV), iu.to(DEV), epoch=step // 2).cpu().numpy())
        monkeypatch.setattr(H, "defer_host_read", orig)
        assert not H.host_read_pending()                 # train_step settles before it returns
        out["deferred"].append(len(seen))
        bank = tr.memobank
        out["mirrors"].append((list(bank.length), list(bank.head), list(bank.ptr)))
        out["stats"].append(dict(LH.LAST_STATS))
        if step == 1:                                    # readers of host state between steps
            sd = tr.optimizer_state_dict()
            ck = engine.checkpoint_state(1, 0.0, model, teacher, tr)
            assert torch.equal(ck["rng_state"]["torch"], torch.get_rng_state()) and sd is not None
            assert [r.shape[0] for r in ck["memobank"]["rows"]] == list(bank.length)
    torch.cuda.synchronize()
    out.update(w=tr.arena.flat.clone(), t=tr.t_arena.flat.clone(), bank=tr.memobank.storage.clone(),
               state=tr.memobank.state.cpu().numpy().copy() if not tr.memobank._state_stale else None,
               rng=torch.get_rng_state().clone(), np_rng=np.random.get_state()[1].copy())
    return out


def test_three_train_steps_with_the_switch_on_and_off(monkeypatch):
    """a small R50 at 65^2, three semi-supervised steps, generator state flowing from step to step: meters, student and
    teacher weights, bank rows, the host mirrors and LAST_STATS after EVERY step and the final generator state are those
    of the host path; the device path really deferred its read (and the host path did not)."""
    a = _train(monkeypatch, True)
    b = _train(monkeypatch, False)
    print("meters", np.stack(a["meters"]).tolist(), "stats", a["stats"], "deferred", a["deferred"], b["deferred"])
    assert all(n >= 1 for n in a["deferred"]) and not any(b["deferred"])
    assert np.isfinite(np.stack(a["meters"])).all()
    assert np.stack(a["meters"]).tobytes() == np.stack(b["meters"]).tobytes()
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["t"], b["t"])
    assert torch.equal(a["bank"], b["bank"])
    assert a["mirrors"] == b["mirrors"] and a["stats"] == b["stats"]
    assert torch.equal(a["rng"], b["rng"]) and np.array_equal(a["np_rng"], b["np_rng"])
    assert any(s["njobs"] > 0 for s in a["stats"])       # the steps really sampled
    st = a["state"]
    assert st[:, 3].tolist() == a["mirrors"][-1][0] and st[:, 2].tolist() == a["mirrors"][-1][1]
