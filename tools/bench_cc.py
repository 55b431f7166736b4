"""Times of the criss-cross attention kernels (csrc/ccattn.hip) and of the CCNet decoder (models.decoder.dec_ccnet); GPU only.

Kernels, at the decoder's default widths (inner_planes 512 = C, key_planes 64 = D): the two entry points at N = 4 x 97 x 97 (2 + 2
crops of 769 x 769), 4 x 65 x 65 and 1 x 129 x 257 (a whole 1024 x 2048 image at stride 8), each beside
tools/micro/stream_yardstick.hip moving the same read and written totals.  Bytes from shapes, every operand once: the forward reads
q, k, v and res and writes w and out; the backward reads g, w, q, k and v and writes dq, dk and dv (dgamma is one float).  (The
backward's workspace -- t / e, as large as w -- and the re-reads of the rows of a line, once per group of CC_PT pixels, are the
kernels' own traffic: they are not in the byte count, so they lower the ratio.)  One sample = a HIP-event pair around REPS
back-to-back calls; kernel and yardstick samples alternate; reported: the median of SAMPLES samples with the quartiles, bytes /
median, and `ratio_to_yardstick` = yardstick median / kernel median (1.0: the entry point moves its bytes as fast as a plain stream
does on this chip).

Decoders: dec_ccnet(in_planes, rep_head=True) in train mode with gamma = 0.5, forward + backward of pred and rep, beside
dec_ocrnet, dec_pspnet (both rep_head=True) and dec_deeplabv3_plus from the same run, in_planes 512 and 2048, 4 x 97 x 97, samples
alternating.

Output: profiles/cc_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash.  A record,
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
from u2pl_amd.models.decoder import dec_ccnet, dec_deeplabv3_plus, dec_ocrnet, dec_pspnet  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
SCALE = int(os.environ.get("CC_SCALE", "1"))           # > 1: shrink the maps (a dry run of the tool, not a measurement)
INNER, KEY = 512, 64
SHAPES = ((4, 97, 97), (4, 65, 65), (1, 129, 257))      # (N, H, W)
IN_PLANES = (512, 2048)


def kernels(ylib, N, H, W):
    H, W = max(H // SCALE, 3), max(W // SCALE, 3)
    P, L, C, D = N * H * W, H + W - 1, INNER, KEY
    torch.manual_seed(0)

    def r(*shape):
        return torch.randn(*shape, device=DEV)
    q, k, v, res, g = r(P, D) * D ** -0.25, r(P, D) * D ** -0.25, r(P, C), r(P, C), r(P, C)
    gamma = torch.full((1,), 0.5, device=DEV)
    w, out, dq, dk, dv, dgamma = torch.empty(P, L, device=DEV), torch.empty_like(v), torch.empty_like(q), torch.empty_like(k), \
        torch.empty_like(v), torch.empty(1, device=DEV)
    ws = torch.empty(query("u2pl_cc_attn_bwd_ws_floats", N, H, W, D, C), device=DEV)

    def fwd():
        call("u2pl_cc_attn_fwd_f32", q, D, k, D, v, C, res, C, gamma, 1.0, N, H, W, D, C, w, L, out, C)

    def bwd():
        call("u2pl_cc_attn_bwd_f32", g, C, w, L, q, D, k, D, v, C, gamma, 1.0, N, H, W, D, C, dq, D, dk, D, dv, C, dgamma, ws)
    fwd()
    b = lambda *ts: [4 * t.numel() for t in ts]     # noqa: E731
    todo = dict(fwd=(fwd, b(q, k, v, res), b(w, out)), bwd=(bwd, b(g, w, q, k, v), b(dq, dk, dv)))
    n = max(sum(rd) + sum(wr) for _, rd, wr in todo.values()) // 4
    ya, yw = torch.randn(n, device=DEV), torch.empty(n, device=DEV)
    row = dict(N=N, H=H, W=W, L=L, C=C, D=D, workspace_floats=ws.numel())
    for name, (fn, reads, writes) in todo.items():
        plan = yardstick_plan([sum(reads)], sum(writes))
        # (more written than read: the yardstick has no write-only form, that part is a Tensor.fill_)
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


def decoders(C):
    N, H = 4, max(97 // SCALE, 3)
    h1 = 2 * H - 1
    torch.manual_seed(1)
    x1 = torch.relu(torch.randn(N, 256, h1, h1, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    x4 = torch.relu(torch.randn(N, C, H, H, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    decs = dict(dec_ccnet=dec_ccnet(in_planes=C, rep_head=True), dec_ocrnet=dec_ocrnet(in_planes=C, rep_head=True),
                dec_pspnet=dec_pspnet(in_planes=C, rep_head=True), dec_deeplabv3_plus=dec_deeplabv3_plus(in_planes=C))
    with torch.no_grad():
        decs["dec_ccnet"].cca.gamma.fill_(0.5)
    grads = {}

    def step(name):
        dec = decs[name].to(DEV).train()

        def run():
            out = dec([x1, None, None, x4])
            if name not in grads:
                grads[name] = {n_: torch.randn_like(o) for n_, o in out.items()}
            sum((out[n_] * g).sum() for n_, g in grads[name].items()).backward()
            K.wgrad_stream_sync()
        return run
    ts = samples({name: step(name) for name in decs}, reps=1)
    out = {name: dict(parameters=sum(p.numel() for p in decs[name].parameters()), **summary(ts[name])) for name in decs}
    for name in ("dec_ocrnet", "dec_pspnet", "dec_deeplabv3_plus"):
        out["dec_ccnet_over_" + name] = round(statistics.median(ts["dec_ccnet"]) / statistics.median(ts[name]), 3)
    out["inputs"] = dict(in_planes=C, x1=[N, 256, h1, h1], x4=[N, C, H, H], mode="train, forward + backward of every output "
                         "(dec_deeplabv3_plus also reads x1 and predicts at its size; dec_ccnet: recurrence 2, shared, gamma 0.5)")
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cc_shapes.json")
    ylib = yardstick_lib()
    rows, drows = [], []
    for N, H, W in SHAPES:
        rows.append(kernels(ylib, N, H, W))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    for C in IN_PLANES:
        drows.append(decoders(C))
        print(json.dumps(drows[-1]), flush=True)
        torch.cuda.empty_cache()
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), scale=SCALE,
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
