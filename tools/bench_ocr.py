"""Times of the object-contextual kernels (csrc/ocr.hip) and of the OCRNet decoder (models.decoder.dec_ocrnet) for 2 + 2 images of
769 x 769 crops (97 x 97 feature maps; GPU only), K = 19 and 150 regions.

Kernels, at the decoder's default widths (inner_planes 512, key_planes 256): the four entry points, each beside
tools/micro/stream_yardstick.hip moving the same read and written totals.  Bytes from shapes, every operand once: pool forward
reads s and x and writes m and f; pool backward reads g_f, m, x, f and add and writes dx and ds; attention forward reads q, kk, v and
writes w and y; attention backward reads g_y, w, q, kk, v and writes dq, dk, dv.  (The slab workspaces and the re-reads of s, of
the region rows and of x per region chunk are the kernels' own traffic: they are not in the byte count, so they lower the ratio.)
One sample = a HIP-event pair around REPS back-to-back calls; kernel and yardstick samples alternate; reported: the median of
SAMPLES samples with the quartiles, bytes / median, and `ratio_to_yardstick` = yardstick median / kernel median (1.0: the entry
point moves its bytes as fast as a plain stream does on this chip).

Decoders: dec_ocrnet(in_planes, num_classes=K, rep_head=True) in train mode, forward + backward of pred, region and rep, beside
dec_pspnet(in_planes, rep_head=True) and dec_deeplabv3_plus(in_planes) from the same run, in_planes 512 and 2048, samples
alternating.

Output: profiles/ocr_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash.  A record,
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
from u2pl_amd._lib import call, query, stream_ptr  # noqa: E402
from u2pl_amd.models.decoder import dec_deeplabv3_plus, dec_ocrnet, dec_pspnet  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
BATCH = int(os.environ.get("OCR_BATCH", "4"))
SCALE = int(os.environ.get("OCR_SCALE", "1"))           # > 1: shrink the maps (a dry run of the tool, not a measurement)
HW, INNER, KEY = 97, 512, 256
REGIONS = (19, 150)
IN_PLANES = (512, 2048)


def kernels(ylib, Kr):
    N, H = BATCH, max(HW // SCALE, 3)
    P, C, D = H * H, INNER, KEY
    torch.manual_seed(0)

    def r(*shape):
        return torch.randn(*shape, device=DEV)
    s, x, add, gf = r(N * P, Kr), r(N * P, C), r(N * P, C), r(N * Kr, C)
    m, f, dx, ds = (torch.empty_like(t) for t in (s, gf, x, s))
    q, gy, kk, v = r(N * P, D), r(N * P, D), r(N * Kr, D), r(N * Kr, D)
    w, y, dq, dk, dv = (torch.empty_like(t) for t in (s, q, q, kk, kk))
    ws = torch.empty(max(query("u2pl_region_pool_fwd_ws_floats", N, P, Kr, C), query("u2pl_region_pool_bwd_ws_floats", N, P, Kr, C),
                         query("u2pl_region_attn_bwd_ws_floats", N, P, Kr, D)), device=DEV)
    sc = KEY ** -0.5
    call("u2pl_region_pool_fwd_f32", s, Kr, x, C, 1.0, N, P, Kr, C, m, Kr, f, C, ws)
    call("u2pl_region_attn_fwd_f32", q, D, kk, D, v, D, sc, N, P, Kr, D, w, Kr, y, D)
    b = lambda *ts: [4 * t.numel() for t in ts]     # noqa: E731
    todo = dict(
        pool_fwd=(lambda: call("u2pl_region_pool_fwd_f32", s, Kr, x, C, 1.0, N, P, Kr, C, m, Kr, f, C, ws), b(s, x), b(m, f)),
        pool_bwd=(lambda: call("u2pl_region_pool_bwd_f32", gf, C, m, Kr, x, C, f, C, add, C, 1.0, N, P, Kr, C, dx, C, ds, Kr, ws),
                  b(gf, m, x, f, add), b(dx, ds)),
        attn_fwd=(lambda: call("u2pl_region_attn_fwd_f32", q, D, kk, D, v, D, sc, N, P, Kr, D, w, Kr, y, D), b(q, kk, v), b(w, y)),
        attn_bwd=(lambda: call("u2pl_region_attn_bwd_f32", gy, D, w, Kr, q, D, kk, D, v, D, sc, N, P, Kr, D, dq, D, dk, D, dv, D, ws),
                  b(gy, w, q, kk, v), b(dq, dk, dv)))
    n = max(sum(rd) + sum(wr) for _, rd, wr in todo.values()) // 4
    ya, yw = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    row = dict(K=Kr, N=N, H=H, W=H, C=C, D=D, workspace_floats=ws.numel())
    for name, (fn, reads, writes) in todo.items():
        plan = yardstick_plan([sum(reads)], sum(writes))
        # (more written than read -- the attention forward: the yardstick has no write-only form, that part is a Tensor.fill_)
        fills = {off: yw[4 * off:4 * (off + n4)] for nr, _, n4, off in plan if nr == 0}

        def yard():
            for nr, nw, n4, off in plan:
                if nr == 0:
                    fills[off].fill_(1.0)
                    continue
                rc = ylib.stream_yardstick(nr, nw, ya.data_ptr() + 16 * off, None, None, None,
                                           yw.data_ptr() + 16 * off if nw else None, None, n4, stream_ptr())
                assert rc == 0, rc
        ts = samples(dict(kernel=fn, yardstick=yard))
        nbytes = sum(reads) + sum(writes)
        row[name] = dict(bytes_read=sum(reads), bytes_written=sum(writes), **summary(ts["kernel"], nbytes),
                         yardstick=dict(launches=[(nr, nw) for nr, nw, _, _ in plan], **summary(ts["yardstick"], nbytes)),
                         ratio_to_yardstick=round(statistics.median(ts["yardstick"]) / statistics.median(ts["kernel"]), 3))
    return row


def decoders(C, Kr):
    N, H = BATCH, max(HW // SCALE, 3)
    h1 = 2 * H - 1
    torch.manual_seed(1)
    x1 = torch.relu(torch.randn(N, 256, h1, h1, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    x4 = torch.relu(torch.randn(N, C, H, H, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    decs = dict(dec_ocrnet=dec_ocrnet(in_planes=C, num_classes=Kr, rep_head=True), dec_pspnet=dec_pspnet(in_planes=C, num_classes=Kr, rep_head=True),
                dec_deeplabv3_plus=dec_deeplabv3_plus(in_planes=C, num_classes=Kr))
    grads = {}

    def step(name):
        dec = decs[name].to(DEV).train()

        def run():
            out = dec([x1, None, None, x4])
            if name not in grads:
                grads[name] = {k: torch.randn_like(o) for k, o in out.items()}
            sum((out[k] * g).sum() for k, g in grads[name].items()).backward()
            K.wgrad_stream_sync()
        return run
    ts = samples({name: step(name) for name in decs}, reps=1)
    out = {name: dict(parameters=sum(p.numel() for p in decs[name].parameters()), **summary(ts[name])) for name in decs}
    for name in ("dec_pspnet", "dec_deeplabv3_plus"):
        out["dec_ocrnet_over_" + name] = round(statistics.median(ts["dec_ocrnet"]) / statistics.median(ts[name]), 3)
    out["inputs"] = dict(in_planes=C, K=Kr, x1=[N, 256, h1, h1], x4=[N, C, H, H], mode="train, forward + backward of every output "
                         "(dec_deeplabv3_plus also reads x1 and predicts at its size)")
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ocr_shapes.json")
    ylib = yardstick_lib()
    rows, drows = [], []
    for Kr in REGIONS:
        rows.append(kernels(ylib, Kr))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
        for C in IN_PLANES:
            drows.append(decoders(C, Kr))
            print(json.dumps(drows[-1]), flush=True)
            torch.cuda.empty_cache()
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), batch=BATCH, scale=SCALE,
               device=torch.cuda.get_device_name(0), reps=REPS, samples=SAMPLES, warmup=WARMUP,
               note="one sample = HIP-event time of reps back-to-back calls / reps (decoders: one forward + backward); median and "
                    "quartiles over the samples; kernel and yardstick samples alternate; tb_per_s = bytes from shapes (every operand "
                    "once) / median; ratio_to_yardstick = yardstick median / kernel median",
               kernels=rows, decoders=drows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(written=out)))


if __name__ == "__main__":
    main()
