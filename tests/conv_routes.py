"""The convolution routes of u2pl_amd/nn.py as lists of C entry points: the cases and the recording function shared by
tests/test_gpu_conv_routes.py and tools/gen_conv_routes.py (which writes tests/golden/conv_routes.json).

A case is the smallest layer at which one dispatch branch of _ConvFn / _GroupedConvFn / conv_bn_eval is taken; N = 2 and
H = W = 9 unless noted, U2PL_WINO_MIN_GAIN at its default.  Only the NAMES are kept -- no scalar arguments, no timings -- so the
fixture survives workspace and tile-plan tuning and changes exactly when a layer changes route."""
import torch

from u2pl_amd import _lib

DEV = "cuda"


def _case(name, cin, cout, k, stride=1, pad=0, dil=1, groups=1, bias=False, hw=9, bn=True, xgrad=True, bf16=0):
    return dict(name=name, cin=cin, cout=cout, k=k, stride=stride, pad=pad, dil=dil, groups=groups, bias=bias, hw=hw, bn=bn,
                xgrad=xgrad, bf16=bf16)


CASES = [
    # stem: im2col path, forward and conv_bn_eval, weight gradient of the patch matrix, statistics by the stand-alone pass
    # (an image needs no gradient: the 3-channel data gradient is not a route of the network)
    _case("stem_3_32_s2", 3, 32, 3, stride=2, pad=1, hw=17, xgrad=False),
    # Winograd without pre-split planes (n_cols <= 64): the U fallback in _wino_conv
    _case("wino_64_64", 64, 64, 3, pad=1),
    # Winograd on pre-split planes: fused statistics, data gradient with and without a join, weight gradient reusing the saved V
    _case("wino_128_128", 128, 128, 3, pad=1),
    # gain 1.27 < 1.7 at 9 x 9: direct pre-split kernel with fused statistics, general data gradient, direct weight gradient
    _case("dil2_128_128", 128, 128, 3, pad=2, dil=2),
    # strided: never Winograd
    _case("s2_128_128", 128, 128, 3, stride=2, pad=1),
    # pointwise data gradient through the bnact epilogue when joined, the plain data gradient when not
    _case("pw_128_128", 128, 128, 1),
    # forward on pre-split planes, data gradient not (n_cols = 32): transpose + direct kernel
    _case("pw_32_128", 32, 128, 1),
    # narrow head: padded gradient columns, padded weight, bias gradient into a sink and into a fresh tensor
    _case("head_128_19", 128, 19, 1, bias=True, bn=False),
    # pooled branch: u2pl_dense_small_f32, statistics returned as None, conv_bn_eval returns None
    _case("pooled_128_128", 128, 128, 1, hw=1),
    # grouped Function: same fork, same bias path
    _case("grouped_128_128_g32", 128, 128, 3, pad=1, groups=32),
    # bf16-operand student (recording calls only): direct kernels, no Winograd, no pre-split
    _case("bf16_128_128", 128, 128, 3, pad=1, bf16=1),
]
SETTINGS = [(h, wino) for h in (True, False) for wino in (0, 4)]       # CONV_H["on"], CONV_ALGO["wino"]


def modes(case):
    """train: forward + backward; train_join: two such layers on one input under a GradJoin (the backward of the second runs
    first and parks its data gradient, the first folds it in); train_sink: gradients into arena-style sinks; nograd: the
    teacher's train-mode forward; eval: eval-mode BatchNorm in the convolution's epilogue (conv_bn_eval)"""
    return (["train"] + (["train_join"] if case["xgrad"] else []) + (["train_sink"] if case["bias"] else []) + ["nograd"]
            + (["eval"] if case["bn"] else []))


def setting_key(h, wino):
    return "h%d_wino%d" % (int(h), wino)


def _layer(Kn, c):
    conv = Kn.Conv2d(c["cin"], c["cout"], c["k"], stride=c["stride"], padding=c["pad"], dilation=c["dil"], bias=c["bias"],
                     groups=c["groups"]).to(DEV)
    return conv, (Kn.BatchNorm2d(c["cout"]).to(DEV) if c["bn"] else None)


def _apply(Kn, conv, bn, x, link=None):
    return conv(x, grad_link=link) if bn is None else Kn.conv_bn(conv, bn, x, grad_link=link)


def run_mode(Kn, c, mode):
    """one fresh seeded layer of case c through `mode` -> {name: tensor} of every result (output, dx, dw, db)"""
    torch.manual_seed(1234)
    conv, bn = _layer(Kn, c)
    x = torch.randn(2, c["hw"], c["hw"], c["cin"], device=DEV).permute(0, 3, 1, 2)
    out = {}
    if mode in ("nograd", "eval"):
        if mode == "eval":
            bn.eval()
        with torch.no_grad():
            out["y"] = _apply(Kn, conv, bn, x)
        return out
    x.requires_grad_(c["xgrad"])
    layers = [(conv, bn)]
    link = None
    if mode == "train_join":
        layers.append(_layer(Kn, c))
        link = Kn.grad_join(x, 2)
        assert link is not None
    if mode == "train_sink":
        for p in (conv.weight, conv.bias):
            p._u2pl_grad = torch.zeros_like(p)
    ys = [_apply(Kn, cv, b, x, link) for cv, b in layers]
    gy = torch.randn_like(ys[0])
    torch.autograd.backward(ys, [gy] * len(ys))
    Kn.wgrad_stream_sync()
    for i, (y, (cv, b)) in enumerate(zip(ys, layers)):
        out["y%d" % i] = y.detach()
        for n, p in (("dw", cv.weight), ("db", cv.bias)):
            if p is not None:
                out["%s%d" % (n, i)] = p._u2pl_grad if mode == "train_sink" else p.grad
    if c["xgrad"]:
        out["dx"] = x.grad
    return out


def record(Kn, c, h, wino, mode):
    """-> the names of the C entry points that `mode` of case c issues, in order, under CONV_H = h and Winograd tile `wino`.
    The caller saves and restores CONV_ALGO / CONV_H / CONV_WS"""
    Kn.CONV_H["on"], Kn.CONV_WS["on"] = h, True
    Kn.CONV_ALGO.update(wino=wino, bf16=c["bf16"])
    _lib.PROFILE = []
    try:
        run_mode(Kn, c, mode)
        return [e[0] for e in _lib.PROFILE]
    finally:
        _lib.PROFILE = None


def record_all(Kn):
    """-> {case: {setting: {mode: [names]}}}"""
    return {c["name"]: {setting_key(h, wino): {m: record(Kn, c, h, wino, m) for m in modes(c)} for h, wino in SETTINGS}
            for c in CASES}
