"""Times of the depthwise kernels (csrc/dwconv.hip) at the shapes of the separable DeepLabv3+ decoder for 2 + 2 images of 769 x 769
(GPU only), each beside tools/micro/stream_yardstick.hip moving the same read and write totals, and of the decoder's forward plus
backward, dense against separable.

Kernels: C = 2048 at 97 x 97 with d = 12 / 24 / 36 (the ASPP branches), C = 1280 at 97 x 97 (head.0), C = 512 and 256 at 193 x 193 (the
towers), and C = 256 at 193 x 193 with stride 2 (no layer of the decoder: the stride-2 path of a light encoder).  Bytes from shapes:
forward x once + y once, data gradient dy once + dx once, weight gradient dy once + x once (its workspace, slabs x 36 C bytes, is
listed but not counted).  The yardstick is launched with the same totals: where the read and the written totals differ (stride 2)
as one launch with a read and a write stream of the smaller total plus a read-only launch of the rest (the data gradient writes
more than it reads: that rest is a Tensor.fill_).  One sample = a HIP-event
pair around REPS back-to-back launches; kernel and yardstick samples alternate; reported: the median of SAMPLES samples with the
quartiles, bytes / median, and `ratio_to_yardstick` = yardstick median / kernel median (1.0: the kernel moves its bytes as fast as
a plain stream does on this chip; this is not a share of the 8 TB/s peak).

Decoder: dec_deeplabv3_plus(in_planes=2048) in train mode, x1 (4, 256, 193, 193) and x4 (4, 2048, 97, 97), forward + backward of
pred and rep, the dense and the separable model alternating on the same inputs.

Output: profiles/dwconv_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd._lib import call, query, stream_ptr  # noqa: E402
from u2pl_amd.layout import _ws, new_act  # noqa: E402
from u2pl_amd.models.decoder import dec_deeplabv3_plus  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
REPS, SAMPLES, WARMUP = 4, 30, 3
BATCH = int(os.environ.get("DWCONV_BATCH", "4"))
SCALE = int(os.environ.get("DWCONV_SCALE", "1"))        # > 1: shrink the maps (a dry run of the tool, not a measurement)
SHAPES = [(2048, 97, 1, 12), (2048, 97, 1, 24), (2048, 97, 1, 36), (1280, 97, 1, 1), (512, 193, 1, 1), (256, 193, 1, 1),
          (256, 193, 2, 1)]                             # (C, H = W, stride, dil)


def yardstick_lib():
    src = os.path.join(ROOT, "tools", "micro", "stream_yardstick.hip")
    out = os.path.join(ROOT, "tools", "tmp", "libstream_yardstick.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-shared", "-fPIC", "-o", out, src])
    y = ctypes.CDLL(out)
    y.stream_yardstick.restype = ctypes.c_int
    y.stream_yardstick.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_long, ctypes.c_void_p]
    return y


def yardstick_plan(reads, write):
    """reads: byte totals of the read streams, write: bytes written (0: none) -> [(nr, nw, n4, offset in float4)]: launches that
    together read and write exactly those totals (rounded down to 16 bytes).  nr = 0 (more written than read: the stride-2 data
    gradient): the yardstick has no write-only form, that part is a Tensor.fill_ of the bytes"""
    left = [b // 16 for b in reads] + [write // 16]
    plan, off = [], 0
    while any(left):
        m = min(v for v in left if v)
        nr, nw = sum(1 for v in left[:-1] if v), int(left[-1] > 0)
        plan.append((nr, nw, m, off))
        left = [v - m if v else 0 for v in left]
        off += m
    return plan


def samples(fns, reps=REPS):
    """fns: {name: callable}; -> {name: [seconds per call]}: SAMPLES event pairs of `reps` calls per name, the names alternating"""
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(SAMPLES):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) / reps * 1e-3)
    return ts


def summary(ts, nbytes=None):
    q = statistics.quantiles(ts, n=4)
    out = dict(median_us=round(statistics.median(ts) * 1e6, 1), q1_us=round(q[0] * 1e6, 1), q3_us=round(q[2] * 1e6, 1))
    if nbytes is not None:
        out["tb_per_s"] = round(nbytes / statistics.median(ts) / 1e12, 3)
    return out


def one_shape(ylib, C, HW, stride, dil):
    N, H = BATCH, max(HW // SCALE, 3)
    pad = dil
    Ho = (H + 2 * pad - 2 * dil - 1) // stride + 1
    torch.manual_seed(0)
    x = torch.relu(torch.randn(N, C, H, H, device=DEV)).contiguous(memory_format=CL)
    gy = torch.randn(N, C, Ho, Ho, device=DEV).contiguous(memory_format=CL)
    w = (torch.randn(C, 1, 3, 3, device=DEV) / 3.0).contiguous(memory_format=CL)
    y, dx, dw = new_act(N, C, Ho, Ho, DEV), new_act(N, C, H, H, DEV), torch.empty_like(w)
    wsb = _ws(query("u2pl_dwconv2d_wgrad_workspace_bytes", N, Ho, Ho, C, C, 3, 3, C), DEV)
    geo = (N, H, H, C, Ho, Ho, C, 3, 3, stride, pad, dil, C)
    bx, by = 4 * N * C * H * H, 4 * N * C * Ho * Ho
    ya, yb = torch.randn(max(bx, by) // 4, device=DEV), torch.randn(max(bx, by) // 4, device=DEV)
    yw = torch.empty(max(bx, by) // 4, device=DEV)
    kernels = dict(fwd=(lambda: call("u2pl_dwconv2d_fwd_f32", x, C, w, None, y, C, *geo), [bx], by),
                   dgrad=(lambda: call("u2pl_dwconv2d_dgrad_f32", gy, C, w, dx, C, *geo), [by], bx),
                   wgrad=(lambda: call("u2pl_dwconv2d_wgrad_f32", gy, C, x, C, dw, wsb, 0, *geo), [by, bx], 0))
    row = dict(C=C, N=N, H=H, W=H, stride=stride, dil=dil, Ho=Ho, Wo=Ho, wgrad_workspace_mb=round(wsb.numel() / 2 ** 20, 2))
    for name, (fn, reads, write) in kernels.items():
        plan = yardstick_plan(reads, write)
        fills = {off: yw[4 * off:4 * (off + n4)] for nr, _, n4, off in plan if nr == 0}

        def yard():
            for nr, nw, n4, off in plan:
                if nr == 0:
                    fills[off].fill_(1.0)
                    continue
                rc = ylib.stream_yardstick(nr, nw, ya.data_ptr() + 16 * off, yb.data_ptr() + 16 * off, None, None,
                                           yw.data_ptr() + 16 * off if nw else None, None, n4, stream_ptr())
                assert rc == 0, rc
        ts = samples(dict(kernel=fn, yardstick=yard))
        nbytes = sum(reads) + write
        row[name] = dict(bytes_read=sum(reads), bytes_written=write, **summary(ts["kernel"], nbytes),
                         yardstick=dict(launches=[(nr, nw) for nr, nw, _, _ in plan], **summary(ts["yardstick"], nbytes)),
                         ratio_to_yardstick=round(statistics.median(ts["yardstick"]) / statistics.median(ts["kernel"]), 3))
    return row


def decoder_pair():
    N, h1, h4 = BATCH, max(193 // SCALE, 5), max(97 // SCALE, 3)
    torch.manual_seed(1)
    x1 = torch.relu(torch.randn(N, 256, h1, h1, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    x4 = torch.relu(torch.randn(N, 2048, h4, h4, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    gp = torch.randn(N, 19, h1, h1, device=DEV).contiguous(memory_format=CL)
    gr = torch.randn(N, 256, h1, h1, device=DEV).contiguous(memory_format=CL)
    decs = {name: dec_deeplabv3_plus(in_planes=2048, separable=sep).to(DEV).train()
            for name, sep in (("dense", False), ("separable", True))}

    def step(dec):
        def run():
            out = dec([x1, None, None, x4])
            ((out["pred"] * gp).sum() + (out["rep"] * gr).sum()).backward()
            K.wgrad_stream_sync()
        return run
    ts = samples({name: step(dec) for name, dec in decs.items()}, reps=1)
    out = {name: dict(parameters=sum(p.numel() for p in decs[name].parameters()), **summary(ts[name])) for name in decs}
    out["separable_over_dense"] = round(statistics.median(ts["separable"]) / statistics.median(ts["dense"]), 3)
    out["inputs"] = dict(x1=[N, 256, h1, h1], x4=[N, 2048, h4, h4], mode="train, forward + backward of pred and rep")
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dwconv_shapes.json")
    ylib = yardstick_lib()
    rows = []
    for C, HW, stride, dil in SHAPES:
        row = one_shape(ylib, C, HW, stride, dil)
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    dec = decoder_pair()
    print(json.dumps(dec), flush=True)
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), batch=BATCH, scale=SCALE,
               device=torch.cuda.get_device_name(0), reps=REPS, samples=SAMPLES, warmup=WARMUP,
               note="one sample = HIP-event time of reps back-to-back launches / reps (decoder: one forward + backward); median and "
                    "quartiles over the samples; kernel and yardstick (dense and separable) samples alternate; tb_per_s = bytes from "
                    "shapes / median; ratio_to_yardstick = yardstick median / kernel median",
               shapes=rows, decoder_forward_backward=dec)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(written=out)))


if __name__ == "__main__":
    main()
