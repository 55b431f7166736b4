"""Times of the dense attention kernels (csrc/attn.hip) and of the Non-local decoder (models.decoder.dec_nonlocal); GPU only.

Kernels: the two entry points at the shapes of SHAPES -- 2 + 2 crops of 769 x 769 at stride 8 (4 x 97 x 97) with all keys and with
the kv_stride 2 sub-grid (49 x 49 keys), 4 x 65 x 65, a whole 1024 x 2048 image (1 x 129 x 257), a transformer-like case (8 heads of
32 + 32 channels, 97 x 97 queries, 49 x 49 keys) and DANet's 512 value channels.  The yardstick is the fp32 matrix pipe, not a stream:
the kernels read their operands Pq / 64 times over through L2 by design and write almost nothing, so a stream of "the same bytes"
says nothing about them.  `flops_nominal` = 2 Pq Pk (D + Dv) per image and head (the forward's two products); `flops_executed`
counts every product the launches run, recomputation included: forward 2 Pq Pk (chunks D + Dv) (each chunk of 128 value channels
recomputes S); backward 2 Pq Pk [(2 D + Dv) for dq: S, dP, dS k + (2 D + Dv) for dk: S, dP, dS^T q + (chunks D + Dv) for dv: S per
chunk, P^T g].  `pipe_fraction` = flops_executed / median / 157.3 TF (the fp32 MFMA peak of the chip), `nominal_fraction` the
same with flops_nominal (backward: 2.5 x the forward's, the usual count of five products against two).

Comparisons from the same run, as information: K.region_attention (csrc/ocr.hip, vector ALU) against K.dense_attention on the same
operands at 150 and 255 keys (4 x 97 x 97 queries, D = Dv = 64), forward and forward + backward through the autograd Functions;
K.criss_cross_attention at 4 x 97 x 97 (D 64, C 256); torch's own fp32 F.scaled_dot_product_attention on the device at the 97 x 97
shape (the error text if the call fails).  Decoders: dec_nonlocal (kv_stride 1 and 2; the zero-initialised norm weight set to 0.5)
in train mode, forward + backward of pred and rep, beside dec_ccnet, dec_ocrnet, dec_pspnet and dec_deeplabv3_plus, in_planes 512
and 2048, 4 x 97 x 97, samples alternating.

One sample = a HIP-event pair around REPS back-to-back calls; reported: the median of SAMPLES samples with the quartiles.
Output: profiles/attn_shapes.json by default (argv[1] overrides), stamped with U2PL_COMMIT and the kernel-source hash.  A record,
not a gate."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dwconv import REPS, SAMPLES, WARMUP, samples, summary  # noqa: E402
from u2pl_amd import nn as K  # noqa: E402
from u2pl_amd._lib import call, query  # noqa: E402
from u2pl_amd.models.decoder import dec_ccnet, dec_deeplabv3_plus, dec_nonlocal, dec_ocrnet, dec_pspnet  # noqa: E402
from u2pl_amd.roofline import kernel_source_hash  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
SCALE = int(os.environ.get("ATTN_SCALE", "1"))         # > 1: shrink the maps (a dry run of the tool, not a measurement)
PEAK = 157.3e12                                        # fp32 MFMA, MI355X
DVC = 128                                              # ATTN_DVC
# (name, N, heads, (Hq, Wq), (Hk, Wk), D, Dv)
SHAPES = (("4x97x97", 4, 1, (97, 97), (97, 97), 64, 256), ("4x97x97_keys_49x49", 4, 1, (97, 97), (49, 49), 64, 256),
          ("4x65x65", 4, 1, (65, 65), (65, 65), 64, 256), ("1x129x257", 1, 1, (129, 257), (129, 257), 64, 256),
          ("4x97x97_8_heads_keys_49x49", 4, 8, (97, 97), (49, 49), 32, 32), ("4x97x97_danet", 4, 1, (97, 97), (97, 97), 64, 512))
IN_PLANES = (512, 2048)


def sc(n):
    return max(n // SCALE, 3)


def kernels(name, N, heads, hwq, hwk, D, Dv):
    Pq, Pk = sc(hwq[0]) * sc(hwq[1]), sc(hwk[0]) * sc(hwk[1])
    torch.manual_seed(0)

    def r(*shape):
        return torch.randn(*shape, device=DEV)
    q, k = r(N * Pq, heads * D) * D ** -0.25, r(N * Pk, heads * D) * D ** -0.25
    v, g = r(N * Pk, heads * Dv), r(N * Pq, heads * Dv)
    o, lse = torch.empty_like(g), torch.empty(N * heads * Pq, device=DEV)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(max(query("u2pl_attn_bwd_ws_floats", N, heads, Pq, Pk, D, Dv), 4), device=DEV)
    geo = (N, heads, Pq, Pk, D, Dv)

    def fwd():
        call("u2pl_attn_fwd_f32", q, heads * D, k, heads * D, v, heads * Dv, 1.0, *geo, o, heads * Dv, lse, None)

    def bwd():
        call("u2pl_attn_bwd_f32", g, heads * Dv, q, heads * D, k, heads * D, v, heads * Dv, o, heads * Dv, lse, 1.0, *geo,
             dq, heads * D, dk, heads * D, dv, heads * Dv, ws)
    fwd()
    ch = -(-Dv // DVC)
    pair = 2.0 * N * heads * Pq * Pk
    flops = dict(fwd=(pair * (D + Dv), pair * (ch * D + Dv)), bwd=(2.5 * pair * (D + Dv), pair * (2 * (2 * D + Dv) + ch * D + Dv)))
    ts = samples(dict(fwd=fwd, bwd=bwd))
    row = dict(name=name, N=N, heads=heads, Pq=Pq, Pk=Pk, D=D, Dv=Dv, workspace_floats=ws.numel())
    for n_ in ("fwd", "bwd"):
        med = statistics.median(ts[n_])
        row[n_] = dict(flops_nominal=flops[n_][0], flops_executed=flops[n_][1], **summary(ts[n_]),
                       tflops_executed=round(flops[n_][1] / med / 1e12, 2), pipe_fraction=round(flops[n_][1] / med / PEAK, 4),
                       nominal_fraction=round(flops[n_][0] / med / PEAK, 4))
    return row


def _fb(fn, ins, g):
    """forward + backward through an autograd Function"""
    def run():
        for t in ins:
            t.grad = None
        fn(*ins).backward(g)
    return run


def comparisons():
    N, H, D = 4, sc(97), 64
    torch.manual_seed(2)
    q = (torch.randn(N, D, H, H, device=DEV) * D ** -0.25).contiguous(memory_format=CL).requires_grad_(True)
    out = {}
    for Kr in (150, 255):
        kk, v = ((torch.randn(N, D, Kr, 1, device=DEV) * D ** -0.25).contiguous(memory_format=CL).requires_grad_(True) for _ in range(2))
        g = torch.randn(N, D, H, H, device=DEV).contiguous(memory_format=CL)
        fns = dict(region=lambda q_, k_, v_: K.region_attention(q_, k_, v_, 1.0), dense=lambda q_, k_, v_: K.dense_attention(q_, k_, v_, 1, 1.0))
        todo = {}
        for n_, fn in fns.items():
            todo[n_ + "_fwd"] = (lambda fn=fn: fn(q.detach(), kk.detach(), v.detach()))
            todo[n_ + "_fwd_bwd"] = _fb(fn, (q, kk, v), g)
        ts = samples(todo)
        row = {n_: summary(t) for n_, t in ts.items()}
        row["dense_over_region_fwd"] = round(statistics.median(ts["dense_fwd"]) / statistics.median(ts["region_fwd"]), 3)
        row["dense_over_region_fwd_bwd"] = round(statistics.median(ts["dense_fwd_bwd"]) / statistics.median(ts["region_fwd_bwd"]), 3)
        out["region_attention_K%d" % Kr] = dict(N=N, H=H, W=H, D=D, K=Kr, **row)
    # criss-cross attention at the same map, D 64, C 256
    C = 256
    k, v = (torch.randn(N, c, H, H, device=DEV).contiguous(memory_format=CL).requires_grad_(True) for c in (D, C))
    gamma = torch.full((1,), 0.5, device=DEV, requires_grad=True)
    g = torch.randn(N, C, H, H, device=DEV).contiguous(memory_format=CL)
    cc = lambda q_, k_, v_: K.criss_cross_attention(q_, k_, v_, gamma, None, 1.0)      # noqa: E731
    de = lambda q_, k_, v_: K.dense_attention(q_, k_, v_, 1, 1.0)                      # noqa: E731
    ts = samples(dict(criss_cross_fwd=lambda: cc(q.detach(), k.detach(), v.detach()), criss_cross_fwd_bwd=_fb(cc, (q, k, v), g),
                      dense_fwd=lambda: de(q.detach(), k.detach(), v.detach()), dense_fwd_bwd=_fb(de, (q, k, v), g)))
    out["criss_cross_attention"] = dict(N=N, H=H, W=H, D=D, C=C, **{n_: summary(t) for n_, t in ts.items()})
    # torch's own fp32 attention on the device
    try:
        qt, kt, vt = (t.detach().permute(0, 2, 3, 1).reshape(N, 1, H * H, -1).contiguous() for t in (q, k, v))
        ts = samples(dict(sdpa_fwd=lambda: F.scaled_dot_product_attention(qt, kt, vt, scale=1.0)))
        out["torch_sdpa_fp32"] = dict(N=N, Pq=H * H, Pk=H * H, D=D, Dv=C, **summary(ts["sdpa_fwd"]))
    except Exception as e:      # noqa: BLE001 (the record keeps the text)
        out["torch_sdpa_fp32"] = dict(error="%s: %s" % (type(e).__name__, str(e)[:400]))
    return out


def decoders(C):
    N, H = 4, sc(97)
    h1 = 2 * H - 1
    torch.manual_seed(1)
    x1 = torch.relu(torch.randn(N, 256, h1, h1, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    x4 = torch.relu(torch.randn(N, C, H, H, device=DEV)).contiguous(memory_format=CL).requires_grad_(True)
    decs = dict(dec_nonlocal=dec_nonlocal(in_planes=C, rep_head=True), dec_nonlocal_kv_stride_2=dec_nonlocal(in_planes=C, kv_stride=2, rep_head=True),
                dec_ccnet=dec_ccnet(in_planes=C, rep_head=True), dec_ocrnet=dec_ocrnet(in_planes=C, rep_head=True),
                dec_pspnet=dec_pspnet(in_planes=C, rep_head=True), dec_deeplabv3_plus=dec_deeplabv3_plus(in_planes=C))
    with torch.no_grad():
        decs["dec_ccnet"].cca.gamma.fill_(0.5)
        for n_ in ("dec_nonlocal", "dec_nonlocal_kv_stride_2"):
            decs[n_].nl.project[1].weight.fill_(0.5)
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
    out["inputs"] = dict(in_planes=C, x1=[N, 256, h1, h1], x4=[N, C, H, H], mode="train, forward + backward of every output "
                         "(dec_deeplabv3_plus also reads x1 and predicts at its size; dec_ccnet: recurrence 2, shared, gamma 0.5; "
                         "dec_nonlocal: key 64, value 256, one head, norm weight 0.5)")
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "attn_shapes.json")
    rows, drows = [], []
    for shape in SHAPES:
        rows.append(kernels(*shape))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    comp = comparisons()
    print(json.dumps(comp), flush=True)
    torch.cuda.empty_cache()
    for C in IN_PLANES:
        drows.append(decoders(C))
        print(json.dumps(drows[-1]), flush=True)
        torch.cuda.empty_cache()
    rec = dict(commit=os.environ.get("U2PL_COMMIT", ""), kernel_sources=kernel_source_hash(), scale=SCALE,
               device=torch.cuda.get_device_name(0), reps=REPS, samples=SAMPLES, warmup=WARMUP, peak_fp32_mfma_tflops=PEAK / 1e12,
               note="one sample = HIP-event time of reps back-to-back calls / reps (decoders: one forward + backward); median and "
                    "quartiles over the samples, names alternating; pipe_fraction = flops_executed / median / peak (every product "
                    "the launches run, recomputation included); nominal_fraction = flops_nominal / median / peak; no counter run",
               kernels=rows, comparisons=comp, decoders=drows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(written=out)))


if __name__ == "__main__":
    main()
