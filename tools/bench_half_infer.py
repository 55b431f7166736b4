"""fp16 prediction path against the fp32 eval-mode forward of the SAME build (that forward is the route every earlier
commit takes; this change does not touch it), ResNet-101 + DeepLabv3+ with 19 classes at the prediction workloads:
  769x769 batch 1, 769x769 batch 4, 1024x2048 batch 1
Per shape, ms per forward pass between two device events (median over the rounds; the two paths alternate inside a
round; every shape is warmed up first; the number of calls per window is chosen so that a window lasts >= 0.5 s):
  fp32_ms / half_ms        model(x)["pred"] under no_grad / HalfPredictor(model)(x) (includes its one counter read-back)
  half_over_fp32           ratio of the medians (< 1: the fp16 path is faster)
  fp32_peak_bytes / half_peak_bytes   peak of torch's allocator over one pass, above what was allocated before it
  half_plan_bytes          fp16 planes + scale / shift vectors + pooled activation buffers the predictor holds
  saturated, argmax_agreement         the outputs of both paths are compared at the timed size before anything is timed
Weights: the seeded default initialisation with BatchNorm statistics drawn around (0, 1) -- activations of trained-network
size, nowhere near fp16's range.
Usage:  python tools/bench_half_infer.py [--out profiles/half_infer.json] [--rounds 5] [--shapes 769x769x1 ...]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from u2pl_amd.half import HalfPredictor  # noqa: E402
from u2pl_amd.models.model_helper import ModelBuilder  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
SHAPES = ["769x769x1", "769x769x4", "1024x2048x1"]


def net_cfg(arch="resnet101", classes=19):
    return dict(num_classes=classes, sync_bn=False, ema_decay=0.99,
                encoder=dict(type=f"u2pl.models.resnet.{arch}",
                             kwargs=dict(multi_grid=True, zero_init_residual=False, fpn=True,
                                         replace_stride_with_dilation=[False, True, True], pretrained=False)),
                decoder=dict(type="u2pl.models.decoder.dec_deeplabv3_plus", kwargs=dict(inner_planes=256, dilations=[12, 24, 36])),
                aux_loss=dict(aux_plane=1024, loss_weight=0.4))


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def bench(model, half, shape, rounds):
    H, W, N = (int(v) for v in shape.split("x"))
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(H + N)).to(DEV).contiguous(memory_format=torch.channels_last)

    @torch.no_grad()
    def fp32():
        return model(x, need_aux=False, need_rep=False)["pred"]

    def fp16():
        return half(x)

    res = dict(fp32_peak_bytes=peak_bytes(fp32), half_peak_bytes=peak_bytes(fp16))      # (also the first warm-up pass of each)
    p32 = fp32()
    p16, saturated = fp16()
    res["saturated"] = saturated
    res["argmax_agreement"] = round(float((p32.argmax(1) == p16.argmax(1)).double().mean()), 5)
    res["max_abs_diff_over_max_abs"] = float((p32 - p16).abs().max() / p32.abs().max())
    del p32, p16
    calls = {}
    for name, fn in (("fp32", fp32), ("half", fp16)):
        fn()
        one = events_ms(fn, 2)
        calls[name] = max(2, min(20, int(500.0 / one) + 1))
    t = dict(fp32=[], half=[])
    for _ in range(rounds):
        for name, fn in (("fp32", fp32), ("half", fp16)):
            t[name].append(events_ms(fn, calls[name]))
    for name in t:
        res[name + "_ms"] = round(statistics.median(t[name]), 3)
        res[name + "_ms_minmax"] = [round(min(t[name]), 3), round(max(t[name]), 3)]
        res[name + "_calls_per_window"] = calls[name]
    res["half_over_fp32"] = round(res["half_ms"] / res["fp32_ms"], 3)
    res["half_plan_bytes"] = half.bytes_allocated()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "half_infer.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arch", default="resnet101")
    ap.add_argument("--shapes", nargs="+", default=SHAPES)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_infer.py needs the GPU: a timing taken elsewhere says nothing")
    torch.manual_seed(0)
    model = ModelBuilder(net_cfg(args.arch))
    g = torch.Generator().manual_seed(1)
    for m in model.modules():                     # running statistics and affine parameters of a network that has trained
        if hasattr(m, "running_var"):
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    model = model.to(DEV).eval()
    half = HalfPredictor(model)
    out = dict(unit="ms per forward pass", arch=args.arch, device=torch.cuda.get_device_name(0), rounds=args.rounds,
               kernel_sources=kernel_source_hash())
    for shape in args.shapes:
        half.release_buffers()                    # buffers of another shape are not this shape's bytes
        torch.cuda.empty_cache()
        out[shape] = bench(model, half, shape, args.rounds)
        print(shape, json.dumps(out[shape]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
