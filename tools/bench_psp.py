"""Times of the pyramid-pooling kernels (csrc/pool.hip) and of the PSPNet decoder (models.decoder.dec_pspnet) for 2 + 2 images
(GPU only): in-plane counts 2048 and 512 at 97 x 97 (769 x 769 crops) and 65 x 65 (513 x 513), levels (1, 2, 3, 6).

Kernels: u2pl_pyramid_pool_fwd_f32 (bytes from shapes: x once PER LEVEL -- the kernel re-reads x for every level -- plus the
pooled outputs) and u2pl_pyramid_pool_bwd_f32 with the add operand (the pooled gradients and add read once, dx written once),
each beside tools/micro/stream_yardstick.hip moving the same read and written totals.  One sample = a HIP-event pair around REPS
back-to-back launches; kernel and yardstick samples alternate; reported: the median of SAMPLES samples with the quartiles,
bytes / median, and `ratio_to_yardstick` = yardstick median / kernel median (1.0: the kernel moves its bytes as fast as a plain
stream does on this chip; this is not a share of the 8 TB/s peak).  `x_once_tb_per_s` of the forward counts x once: what a
single-read multi-level forward would have to beat.

Decoder: dec_pspnet(in_planes, rep_head=True) in train mode, forward + backward of pred and rep, one sample per step.

Output: profiles/psp_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash.  A record,
not a gate."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dwconv import REPS, SAMPLES, WARMUP, samples, summary, yardstick_lib, yardstick_plan  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd._lib import call, stream_ptr  # noqa: E402
from u2pl_amd.layout import new_act  # noqa: E402
from u2pl_amd.models.decoder import dec_pspnet  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
BATCH = int(os.environ.get("PSP_BATCH", "4"))
SCALE = int(os.environ.get("PSP_SCALE", "1"))           # > 1: shrink the maps (a dry run of the tool, not a measurement)
BINS = (1, 2, 3, 6)
SHAPES = [(2048, 97), (2048, 65), (512, 97), (512, 65)]  # (in_planes, H = W)


def kernels(ylib, C, HW):
    N, H = BATCH, max(HW // SCALE, 3)
    torch.manual_seed(0)
    x = torch.randn(N, C, H, H, device=DEV).contiguous(memory_format=CL)
    add = torch.randn(N, C, H, H, device=DEV).contiguous(memory_format=CL)
    ys = [new_act(N, C, b, b, DEV) for b in BINS]
    gs = [torch.randn(N, C, b, b, device=DEV).contiguous(memory_format=CL) for b in BINS]
    dx = new_act(N, C, H, H, DEV)
    bx, bp = 4 * N * C * H * H, 4 * N * C * sum(b * b for b in BINS)
    yargs = [a for y in ys for a in (y, C)]
    gargs = [a for g in gs for a in (g, C)]
    todo = dict(fwd=(lambda: call("u2pl_pyramid_pool_fwd_f32", x, C, N, H, H, C, *BINS, *yargs), [len(BINS) * bx], bp),
                bwd=(lambda: call("u2pl_pyramid_pool_bwd_f32", *gargs, add, C, N, H, H, C, *BINS, dx, C), [bx + bp], bx))
    n = max(len(BINS) * bx, bx + bp) // 4
    ya, yw = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    row = dict(C=C, N=N, H=H, W=H, bins=list(BINS))
    for name, (fn, reads, write) in todo.items():
        plan = yardstick_plan(reads, write)

        def yard():
            for nr, nw, n4, off in plan:
                rc = ylib.stream_yardstick(nr, nw, ya.data_ptr() + 16 * off, None, None, None,
                                           yw.data_ptr() + 16 * off if nw else None, None, n4, stream_ptr())
                assert rc == 0, rc
        ts = samples(dict(kernel=fn, yardstick=yard))
        nbytes = sum(reads) + write
        row[name] = dict(bytes_read=sum(reads), bytes_written=write, **summary(ts["kernel"], nbytes),
                         yardstick=dict(launches=[(nr, nw) for nr, nw, _, _ in plan], **summary(ts["yardstick"], nbytes)),
                         ratio_to_yardstick=round(statistics.median(ts["yardstick"]) / statistics.median(ts["kernel"]), 3))
        if name == "fwd":
            row[name]["x_once_tb_per_s"] = round((bx + bp) / statistics.median(ts["kernel"]) / 1e12, 3)
    return row


def decoder(C, HW):
    N, H = BATCH, max(HW // SCALE, 3)
    torch.manual_seed(1)
    x = torch.relu(torch.randn(N, C, H, H, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    gp = torch.randn(N, 19, H, H, device=DEV).contiguous(memory_format=CL)
    gr = torch.randn(N, 256, H, H, device=DEV).contiguous(memory_format=CL)
    dec = dec_pspnet(in_planes=C, rep_head=True).to(DEV).train()

    def step():
        out = dec(x)
        ((out["pred"] * gp).sum() + (out["rep"] * gr).sum()).backward()
        K.wgrad_stream_sync()
    ts = samples(dict(step=step), reps=1)
    return dict(parameters=sum(p.numel() for p in dec.parameters()), input=[N, C, H, H],
                mode="train, forward + backward of pred and rep", **summary(ts["step"]))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "psp_shapes.json")
    ylib = yardstick_lib()
    rows = []
    for C, HW in SHAPES:
        row = kernels(ylib, C, HW)
        torch.cuda.empty_cache()
        row["decoder_forward_backward"] = decoder(C, HW)
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), batch=BATCH, scale=SCALE,
               device=torch.cuda.get_device_name(0), reps=REPS, samples=SAMPLES, warmup=WARMUP,
               note="one sample = HIP-event time of reps back-to-back launches / reps (decoder: one forward + backward); median and "
                    "quartiles over the samples; kernel and yardstick samples alternate; tb_per_s = bytes from shapes / median (the "
                    "forward's bytes count x once per level, as the kernel reads it); ratio_to_yardstick = yardstick median / kernel "
                    "median",
               shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(written=out)))


if __name__ == "__main__":
    main()
