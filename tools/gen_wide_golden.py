"""Fixtures for more than 32 classes, generated from the REFERENCE's own compute_contra_memobank_loss / label_onehot
(through oracle/ref_shim.py, on the CPU) into tests/golden/:

    python tools/gen_wide_golden.py [contra_c33 contra_c40s contra_c65 contra_c150s contra_c255 relsplit]

Each fixture ASSERTS what it is for (see main()).  Layout, chosen so that no file exceeds 1 MiB:
  contra_65_<tag>.npz        meta (queue sizes, pre-fill, D, ...) and the final banks: bank_sum [C][D] float64,
                             bank_head / bank_tail [C][2][D] (first / last two rows)
  contra_65_<tag>_s<k>.npz   step k: rep, rep_teacher, prob_slot0, masks, small labels, loss, grad_rep, new_keys, ...
  relsplit_65_<tag>.npz      the unlabelled half of the teacher logits (Tier B of the GPU test), labels, entropy, thresholds,
                             masks and small multi-hot labels
prob_slot0 holds the probabilities of images 0 and B only.  Under the label_onehot slot-0 quirk no other image carries a
label bit, so no other image's probabilities are ever selected; the reference is FED the constant 1 / C there and the
tests rebuild the same tensor (wide_ref.full_prob).  oracle.gen_golden.make_step_inputs draws randn * 3 logits, which at
C = 150 leave almost no pixel with prob > 0.3: `boost` adds that much to the logit of a blocky class map.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20


def save(name, **arrs):
    conv = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **conv)
    size = os.path.getsize(path)
    print("wrote", path, size // 1024, "KiB")
    return path, size


def make_inputs(seed, B, S, s, C, D, boost):
    """gen_golden.make_step_inputs with (boost > 0) a blocky class map added to the train-mode teacher logits: the
    labelled images' own labels (nearest down-sampled), a fresh block map for the unlabelled ones"""
    gen = torch.Generator().manual_seed(seed)
    low_t_train = torch.randn(2 * B, C, s, s, generator=gen) * 3
    label_l = GG.block_labels(B, S, C, gen)
    if boost:
        iy = torch.from_numpy(np.minimum(np.floor(np.arange(s, dtype=np.float32) * np.float32(S / s)).astype(np.int64), S - 1))
        cls_l = label_l[:, iy][:, :, iy].clone()
        cls_l[cls_l == 255] = 0
        cls_u = GG.block_labels(B, s, C, gen, ignore_rows=0, cell=3)
        cls = torch.cat((cls_l, cls_u))
        low_t_train = low_t_train + boost * F.one_hot(cls, C).permute(0, 3, 1, 2).float()
    low_t_eval = low_t_train[B:] + 1.5 * torch.randn(B, C, s, s, generator=gen)
    conf, label_u = torch.max(torch.softmax(F.interpolate(low_t_eval, (S, S), mode="bilinear", align_corners=True), 1), 1)
    rep = torch.round(torch.randn(2 * B, D, s, s, generator=gen) * 64) / 64
    rep_t = torch.round(torch.randn(2 * B, D, s, s, generator=gen) * 64) / 64
    prob_all = torch.softmax(low_t_train, 1)
    GG.assert_no_ties(prob_all[[0, B]], k=min(4, C - 1))
    prob_all[1:B] = float(np.float32(1.0) / np.float32(C))
    prob_all[B + 1:] = float(np.float32(1.0) / np.float32(C))
    pred_u_large_teacher = F.interpolate(low_t_train[B:], (S, S), mode="bilinear", align_corners=True)
    return dict(label_l=label_l, label_u_aug=label_u, rep=rep, rep_teacher=rep_t, prob_all=prob_all,
                pred_u_large_teacher=pred_u_large_teacher, low_t_train=low_t_train)


def gen_contra(ns, seed, C, tag, steps=2, boost=0.0, prefill=0, queue_size=400, B=2, S=65, s=17, D=64, alpha_t=20.0):
    """-> per-step facts for the caller's assertions"""
    torch.manual_seed(seed + 1000)
    cfg = dict(GG.CONTRA_CFG)
    fill = [prefill] * C
    memobank = [[GG.formula_bank(i, fill[i], D) if prefill else torch.zeros(0, D)] for i in range(C)]
    ptrs = [torch.zeros(1, dtype=torch.long) for _ in range(C)]
    qs = [queue_size] * C
    qs[0] = queue_size + 100
    facts = []
    for st in range(steps):
        inp = make_inputs(seed + 31 * st, B, S, s, C, D, boost)
        rs = GG.relsplit_reference(ns, inp["pred_u_large_teacher"], inp["label_u_aug"], inp["label_l"], alpha_t, (s, s), C)
        rep = inp["rep"].clone().requires_grad_(True)
        rng_state = torch.get_rng_state()
        len0 = [memobank[c][0].shape[0] for c in range(C)]
        new_keys, loss = ns.loss_helper.compute_contra_memobank_loss(
            rep, rs["label_l_small"], rs["label_u_small"], inp["prob_all"][:B], inp["prob_all"][B:], rs["low_mask_all"],
            rs["high_mask_all"], cfg, memobank, ptrs, qs, inp["rep_teacher"])
        loss.backward()
        assert torch.isfinite(loss)
        # what the reference's loop saw, restated from the saved arrays (loss_helper.py:103-196)
        label = torch.cat((rs["label_l_small"], rs["label_u_small"])).bool()
        low_valid = label & rs["low_mask_all"].bool()
        valid = [c for c in range(C) if low_valid[:, c].any()]
        anchors = [int(((inp["prob_all"][:, c] > cfg["current_class_threshold"]) & low_valid[:, c]).sum()) for c in range(C)]
        len1 = [memobank[c][0].shape[0] for c in range(C)]
        jobs = [(i, vc) for i, vc in enumerate(valid) if anchors[i] > 0 and len1[vc] > 0]      # Q1: list of class i, bank of vc
        facts.append(dict(valid=valid, anchors=anchors, new_keys=list(new_keys), jobs=jobs,
                          wrapped=[c for c in range(C) if len0[c] + new_keys[c] > qs[c]]))
        print(tag, "step", st, "loss", float(loss), "valid", len(valid), "jobs", len(jobs), "keys", int(sum(new_keys)))
        _, size = save(f"contra_65_{tag}_s{st}", rep=inp["rep"], rep_teacher=inp["rep_teacher"],
                       prob_slot0=inp["prob_all"][[0, B]], low_mask_all=rs["low_mask_all"].to(torch.uint8),
                       high_mask_all=rs["high_mask_all"].to(torch.uint8), label_l_small=rs["label_l_small"].to(torch.uint8),
                       label_u_small=rs["label_u_small"].to(torch.uint8), loss=loss, grad_rep=rep.grad,
                       new_keys=np.array(new_keys), rng_state=rng_state,
                       bank_len=np.array(len1), queue_ptr=np.array([int(p[0]) for p in ptrs]), njobs=np.int64(len(jobs)))
        facts[-1]["size"] = size
    bank = [memobank[c][0] for c in range(C)]
    pad = lambda b: torch.cat((b, torch.zeros(max(0, 2 - b.shape[0]), D)))      # (fewer than two rows: zero padded)
    _, size = save(f"contra_65_{tag}", num_steps=np.int64(steps), num_classes=np.int64(C), queue_size=np.array(qs),
                   alpha_t=np.float64(alpha_t), prefill=np.int64(prefill), D=np.int64(D), fill=np.array(fill), B=np.int64(B),
                   bank_sum=torch.stack([b.double().sum(0) for b in bank]),
                   bank_head=torch.stack([pad(b)[:2] for b in bank]), bank_tail=torch.stack([pad(b)[-2:] if b.shape[0] >= 2 else pad(b)[:2] for b in bank]))
    facts.append(dict(size=size))
    return facts


def gen_relsplit(ns, seed, B, C, tag, S=65, s=17, alpha_t=20.0):
    inp = make_inputs(seed, B, S, s, C, 8, 0.0)
    out = GG.relsplit_reference(ns, inp["pred_u_large_teacher"], inp["label_u_aug"], inp["label_l"], alpha_t, (s, s), C)
    most = int(max(out["label_l_small"].sum(1).max(), out["label_u_small"].sum(1).max()))
    out = {k: (v.to(torch.uint8) if isinstance(v, torch.Tensor) and k != "entropy" else v) for k, v in out.items()}
    _, size = save(f"relsplit_65_{tag}", low_t_train=inp["low_t_train"][B:], label_l=inp["label_l"].to(torch.uint8),
                   label_u_aug=inp["label_u_aug"].to(torch.uint8), size=np.int64(S), alpha_t=np.float64(alpha_t),
                   num_classes=np.int64(C), **out)
    assert size <= MAX_BYTES, size
    return most


def main():
    which = set(sys.argv[1:])
    ns = ref_shim.load()
    want = lambda k: not which or k in which
    sizes_ok = lambda facts: all(f["size"] <= MAX_BYTES for f in facts)
    if want("contra_c33"):
        f = gen_contra(ns, 141, 33, "c33", boost=5.0)
        assert sizes_ok(f)
        assert any(32 in st["valid"] and st["anchors"][32] > 0 for st in f[:2]), "class 32: valid with an anchor list"
        assert any(st["new_keys"][32] > 0 for st in f[:2]), "class 32: an enqueued key"
    if want("contra_c40s"):
        f = gen_contra(ns, 142, 40, "c40s", boost=9.0, prefill=396, queue_size=400)
        assert sizes_ok(f)
        assert max(len(st["jobs"]) for st in f[:2]) > 32, "more than 32 jobs in a step"
        assert any(st["wrapped"] for st in f[:2]), "a ring wraps"
    if want("contra_c65"):
        f = gen_contra(ns, 143, 65, "c65", boost=5.0)
        assert sizes_ok(f)
        assert any(63 in st["valid"] and 64 in st["valid"] for st in f[:2]), "classes on both sides of bit 63 | 64 are valid"
    if want("contra_c150s"):
        f = gen_contra(ns, 144, 150, "c150s", boost=9.0, prefill=300, queue_size=400)
        assert sizes_ok(f)
        for st in f[:2]:
            assert len(st["jobs"]) > 32, "more than 32 jobs"
            assert len(st["valid"]) < 150 and any(i != vc for i, vc in st["jobs"]), "Q1's index mismatch is live"
        assert any(vc >= 128 or i >= 128 for st in f[:2] for i, vc in st["jobs"]), "a job whose class is >= 128"
    if want("contra_c255"):
        f = gen_contra(ns, 145, 255, "c255", steps=1, boost=9.0)
        if not sizes_ok(f):        # the upper limit is then covered by the stage-parity test alone
            for n in ("contra_65_c255.npz", "contra_65_c255_s0.npz"):
                os.remove(os.path.join(OUT, n))
            print("contra_65_c255: over the size cap, not kept")
    if want("relsplit"):
        assert gen_relsplit(ns, 146, 2, 150, "c150") >= 2
        assert gen_relsplit(ns, 147, 3, 150, "c150_b3") == 3, "three labels on one pixel under Q0"


if __name__ == "__main__":
    main()
