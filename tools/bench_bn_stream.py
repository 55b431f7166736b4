"""How close the BatchNorm passes run to a plain float4 stream of the same bytes (GPU only).

Every case is one C entry point at one (M, C) of the flagship step, timed with HIP events (median of 5 rounds x 20 launches)
beside its yardstick: tools/micro/stream_yardstick.hip with the same number of 16-byte read and write streams per element, on
the same buffers, in the same process, the two alternating round by round.  Each case runs twice: "hot" re-uses one buffer set
(a 38 MB tensor then sits in the 256 MB Infinity Cache), "rotating" cycles through buffer sets whose footprint exceeds 512 MB.

    python tools/bench_bn_stream.py --tag parent        # merges the run into profiles/bn_stream.json under that tag
    python tools/bench_bn_stream.py --tag new --step-ms 110.1 110.3 110.2      # also records bench.py's ms_per_step of that build

Bytes are algorithmic: streams x M x C x 4 (per-channel vectors, partial sums and the maxima are left out: < 0.1 %).  The
`_bits` cases move the ReLU mask as a bit plane, 1/32 of a stream: it is left out of their bytes like the per-channel vectors, so
their yardstick is the stream count WITHOUT the mask (the from-y cases beside them count y as a full stream)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2pl_amd._lib import call, query, stream_ptr  # noqa: E402

DEV = "cuda"
REPS, ROUNDS = 20, 5
SHAPES = [(592900, 64), (592900, 128), (148996, 64), (148996, 256), (37636, 128), (37636, 256), (37636, 512), (37636, 1024),
          (37636, 2048)]
ROWS_PER_IMAGE = {592900: 148225, 148996: 37249, 37636: 9409}        # 4 images of 385^2, 193^2, 97^2
ROTATE_BYTES = 512 << 20
OUT = os.path.join(ROOT, "profiles", "bn_stream.json")
# case -> (read streams, write streams)
CASES = {
    "bn_apply": (1, 1), "bn_apply_relu": (1, 1), "bn_apply_res_relu": (2, 1),
    "bn_bwd_apply_mask_x": (2, 1), "bn_bwd_apply_mask_y_dres": (3, 2), "bn_bwd_apply_mask_x_pg": (2, 1),
    "bn_bwd_sums": (3, 0), "bn_bwd_sums_mx": (2, 0), "bn_stats": (1, 0), "colsum": (1, 0),
    "bn_apply_res_relu_bits": (2, 1), "bn_bwd_sums_bits": (2, 0), "bn_bwd_apply_bits_dres": (2, 2), "bn_bwd_apply_bits": (2, 1),
}


def yardstick_lib():
    src = os.path.join(ROOT, "tools", "micro", "stream_yardstick.hip")
    out = os.path.join(ROOT, "tools", "tmp", "libstream_yardstick.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-shared", "-fPIC", "-o", out, src])
    lib = ctypes.CDLL(out)
    lib.stream_yardstick.restype = ctypes.c_int
    lib.stream_yardstick.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.c_long, ctypes.c_void_p]
    return lib


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(REPS):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


class BufferSet:
    """the tensors of one launch: five [M, C] activations (the case uses the first nr + nw of them) and the layer's vectors"""

    def __init__(self, M, C, g):
        self.t = [torch.randn(M * C, device=DEV, generator=g) for _ in range(5)]
        self.mean, self.gamma, self.beta = (torch.randn(C, device=DEV, generator=g) * 0.1 for _ in range(3))
        self.invstd = torch.rand(C, device=DEV, generator=g) + 0.5
        self.sums = torch.randn(2 * C, device=DEV, generator=g, dtype=torch.float64)
        self.gsink, self.bsink = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        self.ws = torch.empty(max(1, query("u2pl_colreduce_workspace_bytes", M, 1, C)), device=DEV, dtype=torch.uint8)
        self.out = torch.empty(2 * C, device=DEV, dtype=torch.float64)
        self.amax = torch.zeros(REPS, 2, 2048, device=DEV)
        self.bits = torch.randint(-2 ** 31, 2 ** 31, (M * (C // 32),), device=DEV, generator=g, dtype=torch.int32)


def launcher(case, M, C, sets):
    rpi = ROWS_PER_IMAGE[M]

    def fn(i):
        b = sets[i % len(sets)]
        a0, a1, a2, a3, a4 = b.t
        ax, ar = b.amax[i % REPS, 0], b.amax[i % REPS, 1]
        if case == "bn_apply_res_relu_bits":
            call("u2pl_bn_apply_bits_f32", a0, C, b.mean, b.invstd, b.gamma, b.beta, a1, C, 1, None, rpi, a2, C, M, C, ax, b.bits,
                 C // 32)
        elif case == "bn_bwd_sums_bits":
            call("u2pl_bn_bwd_sums_bits_f32", a0, C, a1, C, b.bits, C // 32, b.mean, b.invstd, None, rpi, M, C, b.ws, b.out)
        elif case.startswith("bn_bwd_apply_bits"):
            dres = a3 if case.endswith("dres") else None
            call("u2pl_bn_bwd_apply_bits_f32", a0, C, a1, C, b.bits, C // 32, b.mean, b.invstd, b.gamma, None, rpi, b.sums, float(M),
                 a2, C, dres, C, M, C, None, None, None, 0, ax, ar if dres is not None else None)
        elif case.startswith("bn_apply"):
            res = a1 if "res" in case else None
            y = a2 if res is not None else a1
            call("u2pl_bn_apply_amax_f32", a0, C, b.mean, b.invstd, b.gamma, b.beta, res, C, int(case != "bn_apply"), None, rpi, y,
                 C, M, C, ax)
        elif case == "bn_bwd_apply_mask_x":
            call("u2pl_bn_bwd_apply_amax_f32", a0, C, a1, C, None, 0, b.mean, b.invstd, b.gamma, None, rpi, b.sums, float(M), a2,
                 C, None, 0, M, C, None, None, None, 0, ax, None, b.beta)
        elif case == "bn_bwd_apply_mask_x_pg":
            call("u2pl_bn_bwd_apply_amax_f32", a0, C, a1, C, None, 0, b.mean, b.invstd, b.gamma, None, rpi, b.sums, float(M), a2,
                 C, None, 0, M, C, b.sums, b.gsink, b.bsink, 0, ax, None, b.beta)
        elif case == "bn_bwd_apply_mask_y_dres":
            call("u2pl_bn_bwd_apply_amax_f32", a0, C, a1, C, a2, C, b.mean, b.invstd, b.gamma, None, rpi, b.sums, float(M), a3,
                 C, a4, C, M, C, None, None, None, 0, ax, ar, None)
        elif case == "bn_bwd_sums":
            call("u2pl_bn_bwd_sums_f32", a0, C, a1, C, a2, C, b.mean, b.invstd, None, rpi, M, C, b.ws, b.out)
        elif case == "bn_bwd_sums_mx":
            call("u2pl_bn_bwd_sums_mx_f32", a0, C, a1, C, b.mean, b.invstd, b.gamma, b.beta, None, rpi, M, C, b.ws, b.out)
        elif case == "bn_stats":
            call("u2pl_bn_stats_f32", a0, C, M, C, b.mean, b.ws, b.out)
        elif case == "colsum":
            call("u2pl_colsum_f32", a0, C, M, 1, C, b.ws, b.out)
        else:
            raise ValueError(case)
    return fn


def yard_launcher(ylib, nr, nw, M, C, sets):
    n4 = M * C // 4

    def fn(i):
        t = sets[i % len(sets)].t
        r = [t[k].data_ptr() if k < nr else None for k in range(4)]
        w = [t[nr + k].data_ptr() if k < nw else None for k in range(2)]
        rc = ylib.stream_yardstick(nr, nw, r[0], r[1], r[2], r[3], w[0], w[1], n4, stream_ptr())
        assert rc == 0, rc
    return fn


def run_shape(ylib, M, C, g):
    sets = [BufferSet(M, C, g) for _ in range(ROTATE_BYTES // (M * C * 4) + 1)]    # rotating: every case's footprint > 512 MB ...
    rows = []
    for case, (nr, nw) in CASES.items():
        nrot = ROTATE_BYTES // ((nr + nw) * M * C * 4) + 1                       # ... with as many sets as this case needs
        for mode, use in (("hot", sets[:1]), ("rotating", sets[:nrot])):
            k, y = launcher(case, M, C, use), yard_launcher(ylib, nr, nw, M, C, use)
            k(0), y(0)
            tk, ty = [], []
            for _ in range(ROUNDS):
                for b in use:
                    b.amax.zero_()
                tk.append(timed(k))
                ty.append(timed(y))
            nbytes = (nr + nw) * M * C * 4
            us_k, us_y = statistics.median(tk), statistics.median(ty)
            row = dict(case=case, M=M, C=C, mode=mode, streams="%dR+%dW" % (nr, nw), bytes=nbytes, sets=len(use), us=round(us_k, 2),
                       tbps=round(nbytes / us_k / 1e6, 3), yard_us=round(us_y, 2), yard_tbps=round(nbytes / us_y / 1e6, 3),
                       ratio=round(us_y / us_k, 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", required=True)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step-ms", type=float, nargs="*", default=None, help="ms_per_step of bench.py runs of this build")
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indices into SHAPES (default: all)")
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    entry = doc.setdefault(a.tag, {})
    if a.step_ms is not None:
        entry["step_ms"] = a.step_ms
    if a.step_ms is None or a.shapes is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_bn_stream.py needs the GPU")
        ylib = yardstick_lib()
        g = torch.Generator(device=DEV).manual_seed(0)
        rows = []
        for k, (M, C) in enumerate(SHAPES):
            if a.shapes is None or k in a.shapes:
                rows += run_shape(ylib, M, C, g)
                torch.cuda.empty_cache()
        entry["device"] = torch.cuda.get_device_name(0)
        entry["cases"] = rows
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
