"""Prediction epilogue timing: the fused u2pl_predict_map_f32 against the composition the tree had before it
(H.bilinear_up -> argmax -> .to(uint8) -> device-to-host copy -> host palette[label]) at the two real workloads:
  cityscapes   19 x 193 x 193 -> 1024 x 2048   (769^2 input, decoder stride 4)
  voc          21 x 129 x 129 ->  375 x  500   (513^2 input)
Prints ONE JSON line.  Per workload, us per call (median of 7 rounds; the two paths alternate inside a round):
  fused_dev / fused_labels_dev   the kernel with / without the palette, between two device events (50 calls)
  unfused_dev                    bilinear_up + argmax + cast, between two device events (50 calls)
  fused_e2e / unfused_e2e        host clock from launch to the uint8 label map AND the RGB image in host memory
                                 (10 calls each, ends in the copies' synchronisation)
  bytes_*                        bytes each path's device work moves, from the shapes
The labels of both paths are compared at the timed sizes before anything is timed.
Usage:  python tools/bench_infer_epilogue.py > profiles/infer_epilogue.json"""
import json
import os
import statistics
import sys
import time

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


def host_us(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def bench(C, lo, hi, cmap, rounds=7):
    x = torch.randn(1, C, *lo, generator=torch.Generator().manual_seed(0)).to(DEV) * 3
    pal_np = colormap(cmap)
    pal = torch.from_numpy(pal_np).to(DEV)

    def unfused_dev():
        return H.bilinear_up(x, hi).argmax(1).to(torch.uint8)

    def unfused_e2e():
        label = unfused_dev().cpu().numpy()
        return label, pal_np[label]

    def fused_e2e():
        label, rgb = H.predict_map(x, hi, pal)
        return label.cpu().numpy(), rgb.cpu().numpy()

    variants = dict(fused_dev=(events_us, lambda: H.predict_map(x, hi, pal), 50),
                    unfused_dev=(events_us, unfused_dev, 50),
                    fused_labels_dev=(events_us, lambda: H.predict_map(x, hi), 50),
                    fused_e2e=(host_us, fused_e2e, 10), unfused_e2e=(host_us, unfused_e2e, 10))
    (la, ca), (lb, cb) = fused_e2e(), unfused_e2e()
    same = float((la == lb).mean())
    assert same == 1.0 and np.array_equal(ca, cb), same          # random-normal logits: no exact ties
    for _, fn, _ in variants.values():                           # warm-up of every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (timer, fn, calls) in variants.items():
            t[k].append(timer(fn, calls))
    res = {k: round(statistics.median(v), 1) for k, v in t.items()}
    res.update({k + "_minmax": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()})
    px, low = hi[0] * hi[1], 4 * C * lo[0] * lo[1]
    res["bytes_fused_dev"] = low + px + 3 * px                   # low-res read (L2 resident) + labels + RGB
    # up-sampled logits written and read again, int64 arg-max written and read, uint8 labels written
    res["bytes_unfused_dev"] = low + 2 * 4 * C * px + 2 * 8 * px + px
    res["fused_dev_over_unfused_dev"] = round(res["fused_dev"] / res["unfused_dev"], 3)
    return res


def main():
    out = dict(unit="us per call", device=torch.cuda.get_device_name(0), kernel_sources=kernel_source_hash())
    for name, (C, lo, hi, cmap) in WORKLOADS.items():
        out[name] = dict(shape=f"{C}x{lo[0]}x{lo[1]} -> {hi[0]}x{hi[1]}", **bench(C, lo, hi, cmap))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
