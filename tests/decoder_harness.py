"""What the GPU tests of the decoder heads share (tests/test_gpu_{psp,ocr,cc,attn}.py; the whole-path part also serves
test_gpu_{dwconv,gconv,lovasz}.py).  A plain helper module like model_utils and the *_bounds modules: no tests, no fixtures.

Raw calls: `call` / `query` through the C ABI on framed buffers.  Rows: an input lies in a pitched buffer whose gaps hold NaN (no
kernel may read them), an output in a sentinel frame that must survive; Ws: a NaN-filled workspace with a sentinel tail;
_twice: every call runs twice into fresh frames and must give the same bits.

Float64 twins: `figures` runs a decoder (Dropout2d p = 0, BatchNorm affine away from (1, 0), 4 x 128 x 9 x 9, train mode) and its
twin written from F.conv2d / F.batch_norm (_seq64) and gives max|got - ref| / max|ref| of every output, dx and every parameter
gradient; `assert_no_worse_than_deeplabv3` holds them to 2x the largest figure of dec_deeplabv3(in_planes=128,
dilations=(1, 2, 12)) against its own twin on the same device.

The whole path: ResNet-50 + a decoder through ModelBuilder at 65 x 65 (a 9 x 9 decoder input): decoder_cfg, build_net, net_input,
step_calls, and train_steps: four SemiTrainer.train_step calls with fixed seeds, with or without graph replay."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from glue_bounds import SENTINEL_BITS, bits_equal
from model_utils import net_cfg
from split_bounds import recorded_calls

DEV = "cuda"
CL = torch.channels_last
f32 = np.float32
SENT = np.array([SENTINEL_BITS], dtype=np.uint32).view(f32)[0]
S_NET = 65


# ---- raw calls in frames -------------------------------------------------------------------------------------------------------
def call(*a):
    from u2pl_amd._lib import call as c
    return c(*a)


def query(*a):
    from u2pl_amd._lib import lib, query as q
    lib()
    return q(*a)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Rows:
    """rows [M, C] of a [N, M / N, C] array inside a buffer of M + 2 rows of ld floats filled with `fill`, starting at row 1 and
    column `off`: NaN for an input (no kernel may read the gaps), the sentinel for an output (no kernel may write the frame).
    wide: a channel-wide tensor (pitch a multiple of 4, 16-byte aligned base); else a K-wide one (any pitch >= K)"""

    def __init__(self, shape, pitched, fill, data=None, wide=True):
        self.shape = shape
        M, C = shape[0] * shape[1], shape[2]
        self.M, self.C = M, C
        self.ld, self.off = ((C + 12, 8) if wide else (C + 5, 3)) if pitched else (C, 0)
        host = np.full((M + 2, self.ld), fill, dtype=f32)
        if data is not None:
            host[1:M + 1, self.off:self.off + C] = np.asarray(data, dtype=f32).reshape(M, C)
        self.buf = D(host)
        self.ptr = self.buf[1:, self.off:]      # the kernel's base pointer: row r, column c at ptr + r ld + c

    def get(self):
        return self.buf.cpu().numpy()[1:self.M + 1, self.off:self.off + self.C].copy().reshape(self.shape)

    def assert_frame_intact(self, what):
        bits = self.buf.cpu().numpy().view(np.uint32).copy()
        bits[1:self.M + 1, self.off:self.off + self.C] = SENTINEL_BITS
        assert (bits == SENTINEL_BITS).all(), f"{what}: wrote outside its {self.M} x {self.C} rows (ld {self.ld})"


class Ws:
    """a NaN-filled workspace of n floats followed by eight sentinels"""

    def __init__(self, n):
        self.n = n
        host = np.full(n + 8, np.nan, dtype=f32)
        host[n:] = SENT
        self.buf = D(host)

    def assert_tail_intact(self, what):
        assert bool((self.buf[self.n:].view(torch.int32) == SENTINEL_BITS).all()), f"{what}: wrote past its {self.n} workspace floats"


def _ptr(r):
    return (None, 0) if r is None else (r.ptr, r.ld)


def _twice(what, run, outs):
    """run() twice into fresh sentinel-framed outputs made by outs() -> the first run's arrays; both runs must agree bit for bit"""
    res = []
    for _ in range(2):
        o = outs()
        ws = run(o)
        torch.cuda.synchronize()
        for k, r in o.items():
            if r is not None:
                r.assert_frame_intact("%s %s" % (what, k))
        if ws is not None:
            ws.assert_tail_intact(what)
        res.append({k: r.get() for k, r in o.items() if r is not None})
    assert all(bits_equal(res[0][k], res[1][k]) for k in res[0]), "two runs of %s differ" % what
    return res[0]


def _merge(a, b):
    return {k: max(a.get(k, 0.0), b.get(k, 0.0)) for k in set(a) | set(b)}


def _show(what, worst):
    print("\n  %s: largest error / bound  %s" % (what, "  ".join("%s %.3f" % (k, worst[k]) for k in sorted(worst))), end="")


# ---- a decoder against its float64 twin ----------------------------------------------------------------------------------------
def _seq64(seq, p, prefix, x):
    """an nn.Sequential of a decoder in float64 (Dropout2d: p = 0 in these tests; the pooling marker is the caller's)"""
    from u2pl_amd import nn as K
    for i, m in enumerate(seq):
        name = "%s.%d" % (prefix, i)
        if isinstance(m, K.Conv2d):
            x = F.conv2d(x, p[name + ".weight"], p.get(name + ".bias"), stride=m.stride, padding=m.padding, dilation=m.dilation)
        elif isinstance(m, K.BatchNorm2d):
            x = F.batch_norm(x, None, None, p[name + ".weight"], p[name + ".bias"], training=True, eps=m.eps)
        elif isinstance(m, torch.nn.ReLU):
            x = torch.relu(x)
        elif isinstance(m, torch.nn.AdaptiveAvgPool2d):
            x = F.adaptive_avg_pool2d(x, m.output_size)
        else:
            assert isinstance(m, torch.nn.Dropout2d) and m.p == 0, m
    return x


def _v3_twin(dec, p, x):
    h, w = x.shape[2:]
    a = dec.aspp
    pooled = F.interpolate(_seq64(a.conv1, p, "aspp.conv1", x), size=(h, w), mode="bilinear", align_corners=True)
    feats = [pooled] + [_seq64(getattr(a, n), p, "aspp." + n, x) for n in ("conv2", "conv3", "conv4", "conv5")]
    return dict(pred=_seq64(dec.head, p, "head", torch.cat(feats, 1)))


def figures(dec, twin, keys, zero_grad=None, seed=0):
    """-> ({name: max|got - ref| / scale}, {name: shape}) over the outputs `keys`, dx and every parameter gradient; scale is
    max|ref| but for zero_grad = (suffixes, is_zero): a parameter whose exact gradient is zero (a bias that shifts every score of
    a softmax alike, or that a train-mode BatchNorm subtracts again) has roundings of the float64 twin as its reference, and
    max|ref| is no scale for it.  Such a gradient must satisfy is_zero(max|ref|, wsum) and its figure is taken relative to wsum,
    the gradient of the same convolution's weight summed over the input channels: what it would be made of if the shift did
    matter.  (The generator: seed + 1, x first, then the G of each key in order; the affine re-draw reads the global one.)"""
    from u2pl_amd import nn as K
    for m in dec.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    with torch.no_grad():
        for n_, q in dec.named_parameters():
            if q.dim() == 1 and isinstance(dec.get_submodule(n_.rsplit(".", 1)[0]), K.BatchNorm2d):   # affine away from (1, 0)
                q.copy_(torch.rand(q.shape) + 0.5 if n_.endswith("weight") else torch.randn(q.shape) * 0.1)
    dec = dec.to(DEV).train()
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.relu(torch.randn(4, 128, 9, 9, generator=g)).contiguous(memory_format=CL)
    xd = x.to(DEV).requires_grad_(True)
    out = dec(xd)
    if not isinstance(out, dict):
        out = dict(pred=out)
    G = {k: torch.randn(out[k].shape, generator=g) for k in keys}
    sum((out[k] * G[k].to(DEV).contiguous(memory_format=CL)).sum() for k in keys).backward()
    K.wgrad_stream_sync()
    torch.cuda.synchronize()
    p = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()
         and "running" not in k}
    x64 = x.double().clone().requires_grad_(True)
    ref_out = twin(dec, p, x64)
    sum((ref_out[k] * G[k].double()).sum() for k in keys).backward()
    ref = dict(dx=x64.grad, **{k: ref_out[k].detach() for k in keys}, **{k: v.grad for k, v in p.items()})
    got = dict(dx=xd.grad, **{k: out[k] for k in keys})
    for n_, q in dec.named_parameters():
        assert q.grad is not None, n_
        got[n_] = q.grad
    assert set(got) == set(ref)
    scale = {k: float(ref[k].abs().max()) for k in got}
    if zero_grad is not None:
        suffixes, is_zero = zero_grad
        for n_ in [n_ for n_ in got if n_.endswith(suffixes)]:
            wsum = float(ref[n_[:-4] + "weight"].abs().sum(1).max())
            assert is_zero(scale[n_], wsum), (n_, scale[n_], wsum)
            scale[n_] = wsum
    fig = {k: float((got[k].detach().cpu().double() - ref[k]).abs().max()) / scale[k] for k in got}
    return fig, {k: tuple(ref[k].shape) for k in got}


def assert_no_worse_than_deeplabv3(label, make_dec, twin, keys, required, zero_grad=None, show_v3=False):
    """the yardstick first, then make_dec() under the same seed (the order in which the global generator is read); both tables are
    printed with show_v3, else the decoder's alone"""
    from u2pl_amd.models.decoder import dec_deeplabv3
    torch.manual_seed(0)
    v3, v3shape = figures(dec_deeplabv3(in_planes=128, dilations=(1, 2, 12)), _v3_twin, ("pred",))
    torch.manual_seed(0)
    fig, shape = figures(make_dec(), twin, keys, zero_grad)
    top = max(v3.values())
    print("\ndecoder figures (max|got - ref| / max|ref|); largest dec_deeplabv3 figure %.3e" % top)
    for k in sorted(v3) if show_v3 else ():
        print("   %-36s %-18s dec_deeplabv3 %.3e" % (k, v3shape[k], v3[k]))
    for k in sorted(fig):
        print("   %-36s %-18s %-13s %.3e" % (k, shape[k], label, fig[k]))
    assert set(required) <= set(fig)
    assert all(np.isfinite(v) for v in fig.values()) and all(np.isfinite(v) for v in v3.values())
    bad = {k: (v, top) for k, v in fig.items() if not v <= 2 * top}
    assert not bad, bad


# ---- the whole path ------------------------------------------------------------------------------------------------------------
def decoder_cfg(decoder=None):
    """the net section of a ResNet-50 with the given decoder section (None: the default DeepLabv3+ one)"""
    cfg = net_cfg("resnet50", 19, True)
    cfg["encoder"]["kwargs"]["zero_init_residual"] = False   # (a zero bn3 weight would cut the gradient of each block's branch)
    if decoder is not None:
        cfg["decoder"] = copy.deepcopy(decoder)
    return cfg


def build_net(cfg, seed=0):
    from u2pl_amd.models.model_helper import ModelBuilder
    torch.manual_seed(seed)
    return ModelBuilder(cfg).to(DEV)


def net_input(n=4, seed=1):
    return torch.randn(n, 3, S_NET, S_NET, generator=torch.Generator().manual_seed(seed)).to(DEV)


def step_calls(model, x, keys=("pred", "rep", "aux")):
    """one forward and backward of model under a recorder -> ({entry point: [argument tuples]}, outputs)"""
    from u2pl_amd import nn as K
    with recorded_calls(K) as seen:
        outs = model(x)
        g = torch.Generator().manual_seed(2)
        loss = sum((outs[k] * torch.randn(outs[k].shape, generator=g).to(DEV)).sum() for k in keys)
        loss.backward()
        K.wgrad_stream_sync()
    torch.cuda.synchronize()
    return seen, outs


def assert_eval_forward_ignores_the_graph(net, keys=("pred", "rep")):
    model, x = net
    model.eval()
    try:
        with torch.no_grad():
            a = model(x)                          # the teacher's path
        b = model(x)                              # records an autograd graph
        assert b["pred"].requires_grad and a["pred"].shape == (4, 19, 9, 9) and a["rep"].shape == (4, 256, 9, 9)
        for k in keys:
            assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k].detach()), k
    finally:
        model.train()


def assert_default_config_is_untouched(net, entry, prefix):
    """the default decoder's C-ABI calls: none that starts with `prefix`, and the same list whether or not `net` (whose step does
    call `entry`) has run in the process: the head's Functions keep no state that another model could meet"""
    counts = []
    for head_first in (False, True):
        if head_first:
            net[0].train()
            assert entry in step_calls(*net)[0]
            net[0].zero_grad(set_to_none=True)
        model = build_net(net_cfg("resnet50", 19, True)).train()
        seen, _ = step_calls(model, net_input(2, 3))
        assert len(seen) > 10
        assert not [n_ for n_ in seen if n_.startswith(prefix)]
        counts.append({k: len(v) for k, v in seen.items()})
    assert counts[0] == counts[1]


def train_steps(monkeypatch, graphs_on, edit_cfg, probe=None, steps=4, S=S_NET):
    """`steps` SemiTrainer.train_step calls of a ResNet-50 student and teacher on S x S crops under edit_cfg(cfg), seeds fixed (the
    models 0; the batches 5; numpy, torch and the device 30, 40, 50 + step) -> meters, both arenas, the graph counters and what
    probe(model) gave after each step.  The criterion is loss_helper.get_criterion as the module holds it at the call."""
    from u2pl_amd import configs, graphs as G
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils import loss_helper

    monkeypatch.setenv("U2PL_GRAPHS", "1" if graphs_on else "0")
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S, batch_size=2, sync_bn=False, epochs=20)
    cfg["criterion"]["kwargs"]["min_kept"] = 1500
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    edit_cfg(cfg)
    torch.manual_seed(0)
    model, teacher = ModelBuilder(copy.deepcopy(cfg["net"])), ModelBuilder(copy.deepcopy(cfg["net"]))
    teacher.load_state_dict(model.state_dict())
    model, teacher = model.to(DEV), teacher.to(DEV)
    tr = SemiTrainer(cfg, model, teacher, loss_helper.get_criterion(cfg), steps_per_epoch=4)
    g = torch.Generator().manual_seed(5)
    stats0 = dict(G.STATS)
    meters, probes = [], []
    for step in range(steps):
        il, iu = torch.randn(2, 3, S, S, generator=g), torch.randn(2, 3, S, S, generator=g)
        ll = torch.randint(0, 19, (2, S, S), generator=g)
        ll[:, :6] = 255
        np.random.seed(30 + step)
        torch.manual_seed(40 + step)
        torch.cuda.manual_seed(50 + step)
        meters.append(tr.train_step(il.to(DEV), ll.to(DEV), iu.to(DEV), epoch=step // 4).cpu().numpy())
        if probe is not None:
            probes.append(probe(model))
    torch.cuda.synchronize()
    return dict(meters=np.stack(meters), w=tr.arena.flat.clone(), t=tr.t_arena.flat.clone(), probes=probes,
                stats={k: G.STATS[k] - stats0[k] for k in stats0})


def assert_replay_equals_eager(a, b):
    """a: train_steps with graph replay, b: without"""
    assert a["stats"]["replays"] > 0 and a["stats"]["aborted"] == 0 and b["stats"]["replays"] == 0
    assert np.isfinite(a["meters"]).all()
    assert np.array_equal(a["meters"], b["meters"]), (a["meters"], b["meters"])
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["t"], b["t"])
