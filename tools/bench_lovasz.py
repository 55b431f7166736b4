"""Where the time of the Lovasz-Softmax route goes (GPU only): per stage of csrc/lovasz.hip the time, the algorithmic bytes and
the ratio to a plain float4 stream moving the same bytes (tools/micro/stream_yardstick.hip, one read and one write stream), and
the whole forward + backward of H.lovasz_softmax beside H.cross_entropy's at the same shape.  One run, medians of 30.

    python tools/bench_lovasz.py            # writes profiles/lovasz.json

Bytes (4-byte words, P pixels, C classes, cc classes of a chunk; every chunk counted):
    errors    reads the C logits and the 8-byte target of every pixel once per chunk, writes cc keys and cc payloads
    sort      one pass = one read and one write of keys and payloads: 16 cc P bytes, four passes (the histogram launch's second
              read of the keys and the tile tables are left out: the yardstick is what a pass must move at the least)
    gradient  reads keys and payloads, writes the plane: 12 cc P (the tile count launch's re-read of the payloads left out)
    backward  reads logits, plane and target, writes dz: 12 C P + 8 P
The permutation scatter of the gradient stage and the digit scatter of a sort pass are uncoalesced by nature; the ratio says
how far each stage is from a coalesced stream, not what a scatter could reach at best -- that limit is not known here."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bn_stream import yardstick_lib  # noqa: E402
from u2pl_amd import hipops as H  # noqa: E402
from u2pl_amd._lib import call, stream_ptr  # noqa: E402

DEV = "cuda"
REPS = 30
SHAPES = [(2, 19, 769, 769), (2, 150, 513, 513)]
OUT = os.path.join(ROOT, "profiles", "lovasz.json")
YARD_CAP = 256 << 20                 # bytes per yardstick stream and launch


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def stage_times(z, t, chunk):
    """one forward + backward through the stage entry points with an event between the calls -> us per stage (all chunks)"""
    N, C, Hh, W = z.shape
    P = N * Hh * W
    plan = H.lovasz_plan(P, C, chunk)
    work = torch.empty(plan["total"], dtype=torch.uint8, device=DEV)
    gplane = torch.empty((C, P), dtype=torch.float32, device=DEV)
    out3 = torch.empty(3, dtype=torch.float32, device=DEV)
    grad = torch.empty_like(z)
    one = torch.ones((), device=DEV)
    acc = dict(errors=[], sort=[], gradient=[], finish=[], backward=[])
    for _ in range(REPS + 1):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))
        mark(None)
        for c0 in range(0, C, plan["cap"]):
            call("u2pl_lovasz_errors_f32", z, t, 255, N, C, Hh, W, c0, work, plan["class_chunk"])
            mark("errors")
            call("u2pl_lovasz_sort", P, C, c0, work, plan["class_chunk"])
            mark("sort")
            call("u2pl_lovasz_grad_f32", P, C, c0, 1, work, plan["class_chunk"], gplane)
            mark("gradient")
        call("u2pl_lovasz_finish_f32", P, C, 1, work, plan["class_chunk"], out3)
        mark("finish")
        call("u2pl_lovasz_bwd_f32", z, t, 255, N, C, Hh, W, gplane, out3, one, 1.0, grad)
        mark("backward")
        torch.cuda.synchronize()
        tot = dict.fromkeys(acc, 0.0)
        for (_, a), (name, b) in zip(marks, marks[1:]):
            tot[name] += a.elapsed_time(b) * 1e3
        for k in acc:
            acc[k].append(tot[k])
    return {k: statistics.median(v[1:]) for k, v in acc.items()}, plan


def yard_us(ylib, nbytes):
    """a 1R + 1W float4 stream moving nbytes in all, in launches of at most YARD_CAP per stream"""
    per = min(nbytes // 2, YARD_CAP) // 16 * 16
    launches = max(1, round(nbytes / 2 / per))
    a, b = torch.empty(per, dtype=torch.uint8, device=DEV), torch.empty(per, dtype=torch.uint8, device=DEV)
    ts = []
    for _ in range(REPS + 1):
        e0, e1 = _events(2)
        e0.record()
        for _k in range(launches):
            rc = ylib.stream_yardstick(1, 1, a.data_ptr(), None, None, None, b.data_ptr(), None, per // 16, stream_ptr())
            assert rc == 0, rc
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts[1:]), per * 2 * launches


def whole(fn, z):
    ts = []
    for _ in range(REPS + 1):
        x = z.clone().requires_grad_(True)
        e0, e1 = _events(2)
        e0.record()
        fn(x).backward()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts[1:])


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_lovasz.py needs the GPU")
    ylib = yardstick_lib()
    g = torch.Generator(device=DEV).manual_seed(0)
    doc = dict(device=torch.cuda.get_device_name(0), reps=REPS, shapes=[])
    for N, C, Hh, W in SHAPES:
        z = torch.randn(N, C, Hh, W, device=DEV, generator=g) * 2
        t = torch.randint(0, C, (N, Hh, W), device=DEV, generator=g)
        t[:, :8] = 255
        P = N * Hh * W
        us, plan = stage_times(z, t, None)
        chunks = [min(plan["cap"], C - c0) for c0 in range(0, C, plan["cap"])]
        nbytes = dict(errors=sum(4 * C * P + 8 * P + 8 * cc * P for cc in chunks),
                      sort=sum(plan["passes"] * 16 * cc * P for cc in chunks),
                      gradient=sum(12 * cc * P for cc in chunks), backward=12 * C * P + 8 * P)
        stages = {}
        for k, v in us.items():
            row = dict(us=round(v, 1))
            if k in nbytes:
                yu, moved = yard_us(ylib, nbytes[k])
                yu *= nbytes[k] / moved
                row.update(bytes=nbytes[k], tbps=round(nbytes[k] / v / 1e6, 3), yard_us=round(yu, 1), ratio=round(yu / v, 3))
            stages[k] = row
        lov = whole(lambda x: H.lovasz_softmax(x, t, 255), z)
        ce = whole(lambda x: H.cross_entropy(x, t, 255), z)
        row = dict(N=N, C=C, H=Hh, W=W, P=P, class_chunk=plan["class_chunk"], chunks=plan["chunks"], tiles=plan["tiles"],
                   workspace_bytes=plan["total"], plane_bytes=4 * C * P, stages=stages, lovasz_fwd_bwd_us=round(lov, 1),
                   cross_entropy_fwd_bwd_us=round(ce, 1))
        print(json.dumps(row), flush=True)
        doc["shapes"].append(row)
        del z, t
        torch.cuda.empty_cache()
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
