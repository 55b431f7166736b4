"""Reliability-map timing: the fused u2pl_predict_entropy_f32 against the composition of kernels the tree had before it
(H.predict_map for the labels + H.entropy_map_up(label=None) for the entropy, two launches), and the whole filtered epilogue,
at the two real workloads:
  cityscapes   19 x 193 x 193 -> 1024 x 2048   (769^2 input, decoder stride 4)
  voc          21 x 129 x 129 ->  375 x  500   (513^2 input)
Prints ONE JSON line.  Per workload, us per call between two device events (median of 7 rounds of 50 calls; the variants
alternate inside a round):
  fused_dev        predict_entropy (logits): one launch, labels + entropy
  unfused_dev      predict_map (labels only) + entropy_map_up into a fresh select workspace (which also fills the select's
                   pass-0 histogram, work the fused kernel does not do)
  fused_prob_dev   predict_entropy(prob=True) on a (C, H, W) accumulator at identity size: what --prob / --scales leave; there is
                   no earlier composition to compare with
  filtered_dev     predict_entropy + entropy_threshold (workspace, pass-0 histogram, two select passes, finish) + reliable_map with
                   palette and heat: everything --drop_percent --entropy adds after the network
  bytes_*          bytes each path's device work moves, from the shapes
Labels and entropy bits of the two paths, and the filtered maps against numpy, are compared at the timed sizes first.
Usage:  python tools/bench_reliability.py > profiles/reliability_map.json"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from u2pl_amd import hipops as H  # noqa: E402
from u2pl_amd.infer import colormap  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
WORKLOADS = dict(cityscapes=(19, (193, 193), (1024, 2048), "cityscapes"), voc=(21, (129, 129), (375, 500), "pascal"))


def events_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def bench(C, lo, hi, cmap, rounds=7, calls=50):
    x = torch.randn(1, C, *lo, generator=torch.Generator().manual_seed(0)).to(DEV) * 3
    pal_np = colormap(cmap)
    pal = torch.from_numpy(pal_np).to(DEV)
    px = hi[0] * hi[1]
    acc = torch.zeros((1, C, *hi), dtype=torch.float32, device=DEV)            # what two fused softmax views leave
    H.window_fuse(acc, None, x, (0, 0), hi, False, True, 0.5, False)
    H.window_fuse(acc, None, x.flip(3), (0, 0), hi, True, True, 0.5, False)

    def unfused():
        label = H.predict_map(x, hi)[0]
        return label, H.entropy_map_up(x, hi, None, H.new_select_ws(DEV, px))

    def filtered():
        label, ent = H.predict_entropy(x, hi)
        thr = H.entropy_threshold(ent, 80.0)
        return (label, ent, thr) + H.reliable_map(label, ent, thr, pal, C)

    # the outputs at the timed sizes, before anything is timed
    (la, ea), (lb, eb) = H.predict_entropy(x, hi), unfused()
    assert torch.equal(la, lb) and torch.equal(ea.view(torch.int32), eb.view(torch.int32))
    label, ent, thr, rgb, heat, nd = filtered()
    e_np = ent.cpu().numpy()
    want_thr = np.asarray(np.percentile(e_np.ravel(), 80.0)).astype(np.float32)
    assert thr.cpu().numpy().view(np.uint32)[0] == want_thr.view(np.uint32)
    want = np.where(e_np >= want_thr, np.uint8(255), la.cpu().numpy())
    assert np.array_equal(label.cpu().numpy(), want) and np.array_equal(rgb.cpu().numpy(), pal_np[want])
    assert int(nd) == int((want == 255).sum())
    x_np = (e_np * np.float32(255 / np.log(C))).astype(np.float32) + np.float32(0.5)
    assert np.array_equal(heat.cpu().numpy(), np.clip(x_np.astype(np.int32), 0, 255).astype(np.uint8))
    ep = H.predict_entropy(acc, hi, prob=True)[1].cpu().numpy().astype(np.float64)
    q = acc[0].cpu().numpy().astype(np.float64)
    q = q / q.sum(0)
    prob_err = float(np.abs(ep[0] + (q * np.log(np.where(q > 0, q, 1.0))).sum(0)).max())

    variants = dict(fused_dev=lambda: H.predict_entropy(x, hi), unfused_dev=unfused,
                    fused_prob_dev=lambda: H.predict_entropy(acc, hi, prob=True), filtered_dev=filtered)
    for fn in variants.values():                                               # warm-up of every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(events_us(fn, calls))
    res = {k: round(statistics.median(v), 1) for k, v in t.items()}
    res.update({k + "_minmax": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()})
    low = 4 * C * lo[0] * lo[1]
    res["bytes_fused_dev"] = low + px + 4 * px                                 # low-res read (L2 resident) + labels + entropy
    res["bytes_unfused_dev"] = 2 * low + px + 4 * px                           # the same outputs, the low-res tensor read by both
    res["bytes_fused_prob_dev"] = 2 * 4 * C * px + px + 4 * px                 # two sweeps over the accumulator
    # + the select: histogram pass and two radix passes over the entropy; + the epilogue: labels and entropy read, labels, RGB, heat
    res["bytes_filtered_dev"] = res["bytes_fused_dev"] + 3 * 4 * px + (px + 4 * px) + (px + 3 * px + px)
    res["fused_dev_over_unfused_dev"] = round(res["fused_dev"] / res["unfused_dev"], 3)
    res["prob_max_abs_err_vs_float64"] = prob_err
    res["dropped_share_at_80"] = round(float(int(nd)) / px, 5)
    return res


def main():
    out = dict(unit="us per call", device=torch.cuda.get_device_name(0), kernel_sources=kernel_source_hash())
    for name, (C, lo, hi, cmap) in WORKLOADS.items():
        out[name] = dict(shape=f"{C}x{lo[0]}x{lo[1]} -> {hi[0]}x{hi[1]}", **bench(C, lo, hi, cmap))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
