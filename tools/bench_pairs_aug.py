"""What the label table costs on the device data pipeline, and the byte-table kernel of --raw_ids.  A record, not a claim:
no threshold is attached to any figure.

  cityscapes   2 x 1024x2048 uint8 samples -> 769x769 crops (rand_resize [0.5, 2.0], flip, random crop), dense
  voc_packed   four VOC-sized samples of different sizes -> 513x513 crops, packed
      old      the entry point such a batch takes without a table (u2pl_augment_u8_f32 / u2pl_augment_ex_u8_f32)
      ex       (dense batch only) u2pl_augment_ex_u8_f32, mode 0: the kernel the table entry instantiates, without the table
      lut      u2pl_augment_lut_u8_f32 on the SAME device buffers and records, ADE20K-style table (offset -1, 150 classes)
    Batches and (wide) records are on the device before the clock starts: a call is the launch alone, no host copy.
  lut_u8       u2pl_lut_u8 in place on a 1024x2048 label map, with its traffic (one read + one write) over that time

Every figure: the median of 30 samples with the inter-quartile range, a sample = 50 calls between two device events; the
two entries of a pair alternate sample by sample, so both see the same machine.  The outputs of a pair are compared
first (image bits equal).  Python `random` seeded with 0.  These are times per CALL on the stream (host enqueue included:
at these sizes a call is a few microseconds of kernel); kernel times come from a profiler run of one case at a time,
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_pairs_aug.py --only cityscapes
Usage:  python tools/bench_pairs_aug.py [--only cityscapes|voc_packed|lut_u8] > profiles/pairs_dataset.json"""
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from u2pl_amd import hipops as H  # noqa: E402
from u2pl_amd.dataset.builder import build_label_lut  # noqa: E402
from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset, augment_batch, widen  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], ignore_label=255, rand_resize=[0.5, 2.0], flip=True)
CASES = dict(
    cityscapes=(dict(NORM, crop=dict(type="rand", size=[769, 769])), [(1024, 2048)] * 2),
    voc_packed=(dict(NORM, crop=dict(type="rand", size=[513, 513])), [(375, 500), (333, 500), (500, 375), (366, 500)]),
)
SAMPLES, CALLS = 30, 50


def batch_for(cfg, sizes):
    rng = np.random.default_rng(0)
    plan = AugmentPlan(cfg)
    random.seed(0)
    items = [(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
              torch.from_numpy(rng.integers(0, 256, (h, w), dtype=np.uint8)), torch.from_numpy(plan.draw(h, w))) for h, w in sizes]
    batch = RawSegDataset.collate_fn(items)
    wide = batch[2] if batch[2].shape[1] == 16 else widen(batch[2], *sizes[0])
    return [t.to(DEV) for t in batch], wide.to(DEV)


def stats(us):
    q1, med, q3 = np.percentile(np.asarray(us), [25, 50, 75])
    return dict(median_us=round(float(med), 1), iqr_us=round(float(q3 - q1), 1))


def time_alternating(fns, samples=SAMPLES, calls=CALLS):
    """fns: {name: callable} -> {name: stats}; one sample of each in turn, `samples` times"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / calls * 1e3)
    return {k: stats(v) for k, v in out.items()}


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    lut = build_label_lut(dict(ignore_label=255, label_map=dict(offset=-1)), 150)
    res = {}
    for name, (cfg, sizes) in CASES.items():
        if only not in (None, name):
            continue
        batch, wide = batch_for(cfg, sizes)
        wide_batch = [batch[0], batch[1], wide] + batch[3:]
        old_plan, lut_plan = AugmentPlan(cfg), AugmentPlan(cfg, lut=lut)
        (oi, ol), (ni, nl) = augment_batch(old_plan, *batch), augment_batch(lut_plan, *wide_batch)
        torch.cuda.synchronize()
        same = torch.equal(oi.view(torch.int32), ni.view(torch.int32))
        # labels: the table image of the old entry's labels, except that the crop's padding stays 0
        pad_ok = bool(((nl == torch.from_numpy(lut).to(DEV)[ol].long()) | ((ol == 0) & (nl == 0))).all())
        res[name] = dict(samples=[list(s) for s in sizes], crop=cfg["crop"]["size"], image_bits_equal=bool(same),
                         labels_consistent=pad_ok,
                         **time_alternating(dict(old=lambda: augment_batch(old_plan, *batch),
                                                 **(dict(ex=lambda: augment_batch(old_plan, *wide_batch)) if len(batch) == 3 else {}),
                                                 lut=lambda: augment_batch(lut_plan, *wide_batch))))
        res[name]["lut_over_old"] = round(res[name]["lut"]["median_us"] / res[name]["old"]["median_us"], 3)
        if "ex" in res[name]:
            res[name]["lut_over_ex"] = round(res[name]["lut"]["median_us"] / res[name]["ex"]["median_us"], 3)
    if only not in (None, "lut_u8"):
        print(json.dumps(dict(unit="us per call", samples=SAMPLES, calls_per_sample=CALLS, **res)))
        return
    n = 1024 * 2048
    lab = torch.from_numpy(np.random.default_rng(1).integers(0, 150, n, dtype=np.uint8)).to(DEV)
    inv = torch.from_numpy(np.random.default_rng(2).permutation(256).astype(np.uint8)).to(DEV)   # a permutation: in place
    # can repeat without the values collapsing
    res["lut_u8"] = dict(bytes=n, **time_alternating(dict(in_place=lambda: H.lut_u8(lab, inv)))["in_place"])
    res["lut_u8"]["GB_per_s"] = round(2 * n / res["lut_u8"]["median_us"] / 1e3, 1)
    print(json.dumps(dict(unit="us per call", samples=SAMPLES, calls_per_sample=CALLS, **res,
                          device=torch.cuda.get_device_name(0), kernel_sources=kernel_source_hash())))


if __name__ == "__main__":
    main()
