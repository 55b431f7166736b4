"""What the once-per-step rebuild of the derived weight operands costs (GPU only): R101-DeepLabv3+ student (forward + transposed +
Winograd planes) and teacher (forward planes) after one 769^2 step registered every operand; `operands.presplit` timed with HIP
events, bytes written from the buffers' sizes, bytes read from the job list (what the library's rebuild reads by construction),
and beside it tools/micro/stream_yardstick.hip (one 16-byte read and one 16-byte write stream) moving the same number of bytes.

    python tools/bench_presplit.py [--tag T --out profiles/presplit.json] [--reps 6]

--out: the record of this run is stored under the top-level key T of the JSON file (other keys are kept)."""
import argparse, ctypes, json, os, subprocess, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from u2pl_amd import configs, nn as K  # noqa: E402
from u2pl_amd.models.model_helper import ModelBuilder  # noqa: E402
from u2pl_amd.trainer import SemiTrainer  # noqa: E402
from u2pl_amd.utils.loss_helper import get_criterion  # noqa: E402
from u2pl_amd._lib import lib, query, stream_ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="run")
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=6)
args = ap.parse_args()


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


def read_bytes(specs, from_taps):
    """bytes the rebuild reads by construction.  from_taps (u2pl_weight_rebuild2h_f32): each weight once for its maximum, once per
    plain / transposed operand for the pieces, the nine taps twice per Winograd operand.  Otherwise (transform launch + maxima pass
    + split pass): the source twice per plain / transposed operand; per Winograd operand the taps once and the fp32 U (which is also
    WRITTEN once: counted in `scratch_written`) twice."""
    rd = wr = 0
    seen = set()
    for wid, sp in specs:
        src = 4 * sp["rows"] * sp["K"] * sp["batch"]
        if sp["how"] == "wino":
            taps = 4 * 9 * sp["O"] * sp["C"]
            if from_taps:
                rd += 2 * taps
            else:
                rd += taps + 2 * src
                wr += src
        elif from_taps:
            rd += src + (0 if wid in seen else src)
            seen.add(wid)
        else:
            rd += 2 * src
    return rd, wr


dev = torch.device("cuda", 0)
torch.manual_seed(2)
np.random.seed(2)
os.environ["U2PL_GRAPHS"] = "0"
cfg = configs.cityscapes_semi(arch="resnet101", crop=769, batch_size=2, sync_bn=True)
C = cfg["net"]["num_classes"]
model, teacher = ModelBuilder(cfg["net"]).to(dev), ModelBuilder(cfg["net"]).to(dev)
tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=163)
gen = torch.Generator(device=dev).manual_seed(2)
b = bench.synth_batch(2, 769, C, dev, gen)
tr.base_lr = 1e-6
for _ in range(2):
    tr.train_step(*b, epoch=1)
torch.cuda.synchronize()
from_taps = hasattr(lib().cdll, "u2pl_weight_rebuild2h_f32")
ylib = yardstick_lib()
out = {"device": torch.cuda.get_device_name(0), "rebuild": "from_taps" if from_taps else "transform_maxima_split"}
for name, arena in (("student", tr.arena), ("teacher", tr.t_arena)):
    ents = [(p.data_ptr(), e) for p in arena.params for e in (p.__dict__.get("_u2pl_derived") or {}).values() if "spec" in e]
    nbytes = sum(e["buf"].numel() for _, e in ents)
    rd, scratch_wr = read_bytes([(wid, e["spec"]) for wid, e in ents], from_taps)
    kinds = {}
    for p in arena.params:
        for k, e in (p.__dict__.get("_u2pl_derived") or {}).items():
            kinds[k] = kinds.get(k, 0) + 1
    moved = nbytes + rd + scratch_wr
    n4 = moved // 32
    ya, yb = torch.empty(n4 * 4, dtype=torch.float32, device=dev), torch.empty(n4 * 4, dtype=torch.float32, device=dev)
    ya.normal_()
    ts, ys = [], []
    for _ in range(args.reps):
        K.bump_weight_epoch(arena)
        torch.cuda.synchronize()
        k0 = query("u2pl_kernel_launches")
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        n = K.presplit(arena.params, arena)
        e1.record()
        rc = ylib.stream_yardstick(1, 1, ya.data_ptr(), None, None, None, yb.data_ptr(), None, n4, stream_ptr())
        e2.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        launches = query("u2pl_kernel_launches") - k0
        ts.append(e0.elapsed_time(e1))
        ys.append(e1.elapsed_time(e2))
    del ya, yb
    out[name] = dict(operands=n, kinds=kinds, launches=launches, bytes_written=nbytes, bytes_read=rd, scratch_written=scratch_wr,
                     ms=[round(t, 3) for t in ts], GBps_written=round(nbytes / (min(ts) * 1e-3) / 1e9, 1),
                     yard_streams="1R+1W", yard_bytes=n4 * 32,
                     yard_note="one read and one write stream of (read + written + scratch) / 2 bytes each: the same TOTAL as the "
                               "rebuild, equally split (the rebuild itself writes about four bytes for every byte it reads)",
                     yard_ms=[round(t, 3) for t in ys],
                     ratio=round(min(ys) / min(ts), 3))
print(json.dumps({args.tag: out}))
if args.out:
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec[args.tag] = out
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
