"""Test-time fusion timing: one view of one sliding window fused by u2pl_window_fuse_f32 against the composition of what
the tree had before it (H.bilinear_up -> flip -> softmax -> scale -> u2pl_window_accumulate_f32), at the two real workloads:
  cityscapes   19 x 193 x 193 -> a 769 x 769 window of a 1024 x 2048 accumulator   (decoder stride 4)
  voc          21 x 129 x 129 -> a 513 x 513 window of a  513 x  513 accumulator
Prints ONE JSON line.  Per workload and per (flip, softmax) setting, us per view between two device events (median of 7
rounds of 20 calls; the two paths alternate inside a round; every shape is warmed up), and the bytes each path's device work
moves, from the shapes.  Both paths' accumulators are compared at the timed sizes before anything is timed.  Only the
epilogue is timed: the two forward passes per window that --flip costs are the same in both paths.
Usage:  python tools/bench_tta_eval.py > profiles/tta_eval.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from u2pl_amd import hipops as H  # noqa: E402
from u2pl_amd._lib import call  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
WORKLOADS = dict(cityscapes=(19, (193, 193), (769, 769), (1024, 2048), (255, 1279)),
                 voc=(21, (129, 129), (513, 513), (513, 513), (0, 0)))


def events_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def bench(C, lo, win, full, origin, flip, softmax, rounds=7, calls=20):
    x = torch.randn(1, C, *lo, generator=torch.Generator().manual_seed(0)).to(DEV) * 3
    weight = 0.5 if flip else 1.0
    acc = {k: (torch.zeros(1, C, *full, device=DEV), torch.zeros(*full, device=DEV)) for k in ("fused", "composed")}

    def fused():
        H.window_fuse(*acc["fused"], x, origin, win, flip, softmax, weight, True)

    def composed():
        v = H.bilinear_up(x, win)
        if flip:
            v = v.flip(3)
        if softmax:
            v = torch.softmax(v, 1)
        if weight != 1.0:
            v = v * weight
        call("u2pl_window_accumulate_f32", *acc["composed"], C, full[0], full[1], v.contiguous(), origin[0], origin[1], win[0], win[1])

    fused()
    composed()
    diff = float((acc["fused"][0] - acc["composed"][0]).abs().max())
    assert diff <= 1e-6 and torch.equal(acc["fused"][1], acc["composed"][1]), diff
    for fn in (fused, composed):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = dict(fused=[], composed=[])
    for _ in range(rounds):
        t["fused"].append(events_us(fused, calls))
        t["composed"].append(events_us(composed, calls))
    res = {k: round(statistics.median(v), 1) for k, v in t.items()}
    res.update({k + "_minmax": [round(min(v), 1), round(max(v), 1)] for k, v in t.items()})
    px, low = 4 * C * win[0] * win[1], 4 * C * lo[0] * lo[1]
    res["bytes_fused"] = low + 2 * px + 2 * 4 * win[0] * win[1]                  # accumulator and count: read + write
    passes = 1 + 2 * (int(flip) + int(softmax) + int(weight != 1.0))               # bilinear_up's write; each torch op: read + write
    res["bytes_composed"] = low + passes * px + 3 * px + 2 * 4 * win[0] * win[1]   # accumulate: source read, accumulator read + write
    res["fused_over_composed"] = round(res["fused"] / res["composed"], 3)
    res["max_abs_difference"] = diff
    return res


def main():
    out = dict(unit="us per view", device=torch.cuda.get_device_name(0), kernel_sources=kernel_source_hash())
    for name, (C, lo, win, full, origin) in WORKLOADS.items():
        out[name] = dict(shape=f"{C}x{lo[0]}x{lo[1]} -> {win[0]}x{win[1]} at {origin} of {full[0]}x{full[1]}")
        for flip, softmax in ((0, 0), (1, 0), (0, 1), (1, 1)):
            out[name][f"flip{flip}_softmax{softmax}"] = bench(C, lo, win, full, origin, flip, softmax)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
