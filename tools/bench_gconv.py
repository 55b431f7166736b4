"""Times of the grouped-convolution kernels (csrc/gconv.hip) on the conv2 shapes of ResNeXt-101 32x4d / 32x8d at 769 x 769, batch 4
(GPU only).  The shapes are collected by a forward hook on every `conv2` of resnet101(groups=32, width_per_group=w,
replace_stride_with_dilation=[False, True, True]); per distinct shape the three C entry points are timed with HIP events
(REPS launches per event pair, median of ROUNDS pairs, every shape warmed up first) and written with
  * the achieved bytes/s against the floor of the layer's own bytes (x once + y once; the weight gradient reads dy and x),
  * the time of the existing DENSE route for a C -> C 3x3 of the same geometry (K.Conv2d forward under no_grad, and its
    data + weight gradient through autograd), which does `groups` times the multiplies.
Sanity line: a grouped launch slower than the dense one is a defect (`slower_than_dense`).
Output: profiles/gconv_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd._lib import call, query  # noqa: E402
from u2pl_amd.layout import _ws, new_act  # noqa: E402
from u2pl_amd.models import resnet  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
REPS, ROUNDS = 5, 5
HBM = 8.0e12            # bytes / s (MI355X peak)
CROP, BATCH = int(os.environ.get("GCONV_CROP", "769")), int(os.environ.get("GCONV_BATCH", "4"))


def collect(width):
    """distinct (C, groups, H, W, stride, dil) of the encoder's conv2 layers, in order of first use, with their counts"""
    net = resnet.resnet101(pretrained=False, groups=32, width_per_group=width,
                           replace_stride_with_dilation=[False, True, True]).to(DEV).eval()
    seen = {}

    def hook(mod, inp, out):
        x = inp[0]
        key = (mod.in_channels, mod.groups, x.shape[2], x.shape[3], mod.stride, mod.dilation)
        seen[key] = seen.get(key, 0) + 1
    hs = [m.conv2.register_forward_hook(hook) for m in net.modules() if isinstance(m, resnet.Bottleneck)]
    with torch.no_grad():
        net(torch.randn(BATCH, 3, CROP, CROP, device=DEV).contiguous(memory_format=CL))
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    del net
    torch.cuda.empty_cache()
    return seen


def timed(fn):
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / REPS)
    return statistics.median(ts) * 1e-3         # seconds


def one_shape(C, groups, H, W, stride, dil, count, width):
    N, R = BATCH, 3
    pad = dil
    Ho, Wo = (H + 2 * pad - dil * 2 - 1) // stride + 1, (W + 2 * pad - dil * 2 - 1) // stride + 1
    torch.manual_seed(0)
    x = torch.relu(torch.randn(N, C, H, W, device=DEV)).contiguous(memory_format=CL)
    gy = torch.randn(N, C, Ho, Wo, device=DEV).contiguous(memory_format=CL)
    w = (torch.randn(C, C // groups, R, R, device=DEV) / (3.0 * (C // groups) ** 0.5)).contiguous(memory_format=CL)
    y, dx, dw = new_act(N, C, Ho, Wo, DEV), new_act(N, C, H, W, DEV), torch.empty_like(w)
    wsb = _ws(query("u2pl_gconv2d_wgrad_workspace_bytes", N, Ho, Wo, C, C, R, R, groups), DEV)
    geo = (N, H, W, C, Ho, Wo, C, R, R, stride, pad, dil, groups)
    fns = dict(fwd=lambda: call("u2pl_gconv2d_fwd_f32", x, C, w, None, y, C, *geo),
               dgrad=lambda: call("u2pl_gconv2d_dgrad_f32", gy, C, w, dx, C, *geo),
               wgrad=lambda: call("u2pl_gconv2d_wgrad_f32", gy, C, x, C, dw, wsb, 0, *geo))
    nbytes = 4.0 * C * N * (H * W + Ho * Wo)
    row = dict(width_per_group=width, C=C, groups=groups, cg=C // groups, N=N, H=H, W=W, stride=stride, dil=dil, layers=count,
               bytes_x_plus_y=nbytes, floor_us=round(nbytes / HBM * 1e6, 1), wgrad_workspace_mb=round(wsb.numel() / 2 ** 20, 1))
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        t = timed(fn)
        row[name] = dict(us=round(t * 1e6, 1), tb_per_s=round(nbytes / t / 1e12, 3), frac_of_floor=round(nbytes / HBM / t, 3))
    # the dense route on a C -> C 3x3 of the same geometry
    dense = K.Conv2d(C, C, 3, stride=stride, padding=pad, dilation=dil, bias=False).to(DEV)
    with torch.no_grad():
        dense(x)
        torch.cuda.synchronize()
        t_f = timed(lambda: dense(x))
    xg = x.detach().requires_grad_(True)
    yd = dense(xg)

    def bwd():
        yd.backward(gy, retain_graph=True)
        K.wgrad_stream_sync()
    bwd()
    torch.cuda.synchronize()
    t_b = timed(bwd)
    row["dense"] = dict(fwd_us=round(t_f * 1e6, 1), dgrad_plus_wgrad_us=round(t_b * 1e6, 1))
    row["slower_than_dense"] = bool(row["fwd"]["us"] > row["dense"]["fwd_us"]
                                    or row["dgrad"]["us"] + row["wgrad"]["us"] > row["dense"]["dgrad_plus_wgrad_us"])
    return row


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gconv_shapes.json")
    rows = []
    for width in (4, 8):
        for (C, groups, H, W, stride, dil), count in collect(width).items():
            row = one_shape(C, groups, H, W, stride, dil, count, width)
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    tot = {}
    for width in (4, 8):
        sel = [r for r in rows if r["width_per_group"] == width]
        tot["32x%dd" % width] = {k: round(sum(r[k]["us"] * r["layers"] for r in sel) / 1e3, 3) for k in ("fwd", "dgrad", "wgrad")}
        tot["32x%dd" % width]["floor_ms_one_pass"] = round(sum(r["floor_us"] * r["layers"] for r in sel) / 1e3, 3)
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), crop=CROP, batch=BATCH,
               device=torch.cuda.get_device_name(0), reps=REPS, rounds=ROUNDS, hbm_peak_bytes_per_s=HBM,
               note="us = median over rounds of (HIP-event time of reps back-to-back launches / reps); floor = (x + y bytes) / peak",
               per_pass_ms_all_conv2_layers=tot, any_slower_than_dense=any(r["slower_than_dense"] for r in rows), shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(written=out, totals=tot, any_slower_than_dense=rec["any_slower_than_dense"])))


if __name__ == "__main__":
    main()
