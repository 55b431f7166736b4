"""Device data pipeline timing at the Cityscapes training shape: 4 x 1024x2048 uint8 samples -> 769x769 crops.
Prints ONE JSON line (us per call, median of 5 rounds of 50 calls between two events):
  old          u2pl_augment_u8_f32 (equal sizes, no rotation / blur)
  ex_dense     u2pl_augment_ex_u8_f32 on the same inputs, mode 0
  ex_ragged    the same geometry on four samples of different sizes, packed
  rot / blur / rot_blur   the options on the dense batch; every sample carries the flag (the blur coin is forced)
Geometry: rand_resize [0.5, 2.0], flip, random crop, python `random` seeded with 0.
Usage:  python tools/bench_augment.py > profiles/augment_bench.json"""
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from u2pl_amd.dataset.device_aug import BLUR, AugmentPlan, RawSegDataset, augment_batch  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
BASE = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], ignore_label=255, rand_resize=[0.5, 2.0], flip=True,
            crop=dict(type="rand", size=[769, 769]))
SIZES = dict(dense=[(1024, 2048)] * 4, ragged=[(1024, 2048), (1000, 2040), (1024, 1900), (900, 2048)])


def batch_for(cfg, sizes, force_blur=False):
    rng = np.random.default_rng(0)
    plan = AugmentPlan(cfg)
    random.seed(0)
    items = []
    for h, w in sizes:
        rec = plan.draw(h, w)
        if force_blur:
            rec[7] |= BLUR
        items.append((torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
                      torch.from_numpy(rng.integers(0, 19, (h, w), dtype=np.uint8)), torch.from_numpy(rec)))
    return plan, [t.to(DEV) for t in RawSegDataset.collate_fn(items)]


def time_us(fn, calls=50, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls * 1e3)
    return round(statistics.median(out), 1)


def main():
    res = {}
    plan, batch = batch_for(BASE, SIZES["dense"])
    res["old"] = time_us(lambda: augment_batch(plan, *batch))
    plan_ex = AugmentPlan(BASE)
    wide = torch.zeros((4, 16), dtype=torch.int32, device=DEV)      # wide records send the dense batch to the new entry point
    wide[:, :7] = batch[2][:, :7]
    res["ex_dense"] = time_us(lambda: augment_batch(plan_ex, batch[0], batch[1], wide))
    plan_r, ragged = batch_for(BASE, SIZES["ragged"])
    res["ex_ragged"] = time_us(lambda: augment_batch(plan_r, *ragged))
    for name, opts in (("rot", dict(rand_rotation=[-10.0, 10.0])), ("blur", dict(GaussianBlur=True)),
                       ("rot_blur", dict(rand_rotation=[-10.0, 10.0], GaussianBlur=True))):
        p, b = batch_for(dict(BASE, **opts), SIZES["dense"], force_blur="GaussianBlur" in opts)
        res[name] = time_us(lambda: augment_batch(p, *b))
    print(json.dumps(dict(shape="4x1024x2048 -> 769x769", unit="us per call", **res,
                          ex_dense_over_old=round(res["ex_dense"] / res["old"], 3), device=torch.cuda.get_device_name(0),
                          kernel_sources=kernel_source_hash())))


if __name__ == "__main__":
    main()
