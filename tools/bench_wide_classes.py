"""Cost of the loss path with more than 32 classes: reliability split + phase 1 + InfoNCE forward and backward at the training
size (2 + 2 images, 769^2 -> 193^2, D = 256, banks pre-filled), inputs as in tools/bench_loss_path.py, for
    C = 19 narrow | C = 19 forced onto the wide route | C = 40 | C = 150.
Each case: 3 warm-up calls, then RUNS repetitions timed one by one with device events around the whole call (every launch and
the step's host synchronisation included); median, min, max and the inter-quartile range are reported.  Before anything is timed every case is run once
and checked: finite loss, keys and jobs present, and at C = 19 the same keys per class and jobs on both routes.  Writes
profiles/wide_classes.json.  GPU only:  python tools/bench_wide_classes.py [--runs 30]"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2pl_amd import hipops as H  # noqa: E402
from u2pl_amd.utils import loss_helper as LH  # noqa: E402

DEV = "cuda"
CFG = dict(negative_high_entropy=True, low_rank=3, high_rank=20, current_class_threshold=0.3,
           current_class_negative_threshold=1, low_entropy_threshold=20, num_negatives=50, num_queries=256,
           temperature=0.5)


def times_us(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return np.array(out)


def stats(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return dict(median_us=round(float(med), 1), min_us=round(float(t.min()), 1), max_us=round(float(t.max()), 1),
                iqr_us=round(float(q3 - q1), 1), runs=int(t.size))


def case(C, force_wide, runs):
    B, S, s, D = 2, 769, 193, 256
    g = torch.Generator(device=DEV).manual_seed(2)
    low = torch.randn(2 * B, C, s, s, device=DEV, generator=g) * 3
    label_l = torch.randint(0, C, (B, S, S), device=DEV, generator=g)
    label_l[:, :8] = 255
    if C > 32:      # randn * 3 logits leave almost no pixel above the anchor threshold at many classes: sharpen the labelled class
        iy = torch.linspace(0, S - 1, s, device=DEV).long()
        cls = torch.cat((label_l[:, iy][:, :, iy].clamp(max=C - 1), torch.randint(0, C, (B, s, s), device=DEV, generator=g)))
        low = low + 9.0 * torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).float()
    low = low.contiguous(memory_format=torch.channels_last)
    rep = torch.randn(2 * B, D, s, s, device=DEV, generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rep_t = torch.randn(2 * B, D, s, s, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    large = H.bilinear_up(low[B:], (S, S))
    _, label_u = H.pseudo_label(large + torch.randn(large.shape, device=DEV, generator=g))
    del large
    prob = torch.softmax(low, 1).contiguous(memory_format=torch.channels_last)
    bank = H.DeviceMemoryBank(C, [50000] + [30000] * (C - 1), D, DEV)
    for c in range(C):
        bank.load_logical(c, torch.randn(bank.cap[c], D, device=DEV, generator=g))
    orig = H.contra_phase1
    if force_wide:
        H.contra_phase1 = lambda *a, **k: orig(*a, wide=True, **k)
    info = {}

    def step():
        rep.grad = None
        rs = H.reliability_split(low[B:], (S, S), label_l, label_u, (s, s), [80.0, 20.0, 80.0])
        keys, loss = LH.contra_memobank_core(rep, rs["lbits"], B, prob[:B], prob[B:], rs["low_mask"], rs["high_mask"], CFG, bank,
                                             rep_t)
        loss.backward()
        assert bool(torch.isfinite(loss)), "non-finite loss"
        info.update(per_class=[int(k) for k in keys], new_keys=int(sum(keys)), njobs=int(LH.LAST_STATS.get("njobs", 0)), valid_seg=int(LH.LAST_STATS.get("valid_seg", 0)))

    try:
        step()                   # un-timed: what the case computes, checked by main() before anything is timed
        torch.cuda.synchronize()
        check = dict(info)
        if runs == 0:
            return check
        t = times_us(step, runs)
    finally:
        H.contra_phase1 = orig
    assert info == check, "a timed call computed something else than the first"
    info.pop("per_class")
    return dict(C=C, route="wide" if (force_wide or C > H.MAXC) else "narrow", **info, **stats(t))


def main():
    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else 30
    # before timing: the narrow and the forced-wide route at C = 19 enqueue the same keys per class and build the same jobs
    na, wi = case(19, False, 0), case(19, True, 0)
    assert na == wi and na["new_keys"] > 0 and na["njobs"] > 0, (na, wi)
    for C in (40, 150):
        chk = case(C, False, 0)
        assert chk["new_keys"] > 0 and chk["njobs"] > 32, chk
    res = dict(what="reliability split + phase 1 + InfoNCE forward and backward, 2 + 2 images, 769^2 -> 193^2, D = 256",
               device=torch.cuda.get_device_name(0),
               commit=subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None,
               cases=[case(19, False, runs), case(19, True, runs), case(40, False, runs), case(150, False, runs)])
    out = os.path.join(ROOT, "profiles", "wide_classes.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print("wrote", out)


if __name__ == "__main__":
    main()
