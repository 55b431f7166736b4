"""fp16 prediction path: the eval-mode forward pass with fp16 activations and fp16 weights in HBM (csrc/half.hip,
DESIGN section 3.9).

  HalfPredictor(model)   walks the project's own module classes (models.resnet.ResNet with Bottleneck / BasicBlock,
                         models.base.ASPP, dec_deeplabv3_plus, dec_deeplabv3, ModelBuilder with fpn true or false) and
                         builds the plan once: fp16 weight planes [Cout][R][S][Cin], per-layer fp32 scale / shift of the
                         eval-mode BatchNorm (evaluated in float64, rounded once), activation buffers per input shape.
  predictor(x)           fp32 NHWC image batch -> (pred, saturated): the decoder's low-resolution logits as fp32
                         (N, C, h, w) and the number of stored activations that had to be clamped to +-65504.  A pass
                         with saturated > 0 is not to be trusted: the callers (infer.infer_image, evaluate.net_process)
                         run it again on the fp32 path.
  predictor.refresh()    rebuilds planes, scales and shifts after the model's weights changed.

Rounding points: every stored activation is rounded to fp16 once, from the fp32 epilogue value (after BatchNorm scale /
shift, residual add and ReLU); the pool, the global average and the up-samples round once each; the classifier's last
1x1 writes fp32.  Weights are rounded as they are: BatchNorm is not folded into them.  Grouped convolutions and encoder /
decoder classes this module does not know raise at construction -- they keep the fp32 path.  There is no fallback to
PyTorch arithmetic anywhere: without the library every call raises.
"""
import torch
import torch.nn as nn

from . import nn as K
from ._lib import HipError, call
from .models.base import ASPP
from .models.decoder import dec_deeplabv3, dec_deeplabv3_plus
from .models.model_helper import ModelBuilder
from .models.resnet import BasicBlock, Bottleneck, ResNet


def fold_bn(conv, bn):
    """(scale, shift) fp32 CPU tensors (either may be None) of `bn(conv(x))` in eval mode: scale = gamma / sqrt(running_var
    + eps), shift = beta - mean * scale (+ bias * scale), evaluated in float64 and rounded once.  Without a BatchNorm:
    (None, bias)."""
    bias = None if conv.bias is None else conv.bias.detach().double().cpu()
    if bn is None:
        return None, None if bias is None else bias.float()
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    shift = bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * scale
    if bias is not None:
        shift = shift + bias * scale
    return scale.float(), shift.float()


class _Unit:
    """one fused layer: convolution (+ eval BatchNorm) (+ ReLU); the residual is given at run time"""

    def __init__(self, name, conv, bn, relu):
        if not isinstance(conv, K.Conv2d):
            raise TypeError(f"HalfPredictor: {name} is a {type(conv).__name__}, expected u2pl_amd.nn.Conv2d")
        if conv.groups != 1:
            raise ValueError(f"HalfPredictor: {name} is a grouped convolution (groups={conv.groups}); the fp16 path has no "
                             "grouped kernel -- use the fp32 path")
        if bn is not None and not isinstance(bn, K.BatchNorm2d):
            raise TypeError(f"HalfPredictor: {name} is followed by a {type(bn).__name__}, expected u2pl_amd.nn.BatchNorm2d")
        self.name, self.conv, self.bn, self.relu = name, conv, bn, relu
        self.w16 = self.scale = self.shift = None

    def refresh(self):
        conv = self.conv
        scale, shift = fold_bn(conv, self.bn)
        dev = conv.weight.device
        self.scale = None if scale is None else scale.to(dev)
        self.shift = None if shift is None else shift.to(dev)
        self.w16 = None
        if dev.type == "cuda":
            Cout, Cin, R, S = conv.weight.shape
            w = conv.weight.detach().float().contiguous()          # torch OIHW order, whatever the memory format was
            self.w16 = torch.empty((Cout, R, S, Cin), dtype=torch.float16, device=dev)
            call("u2pl_half_weight_f16", w, Cout, Cin, R, S, self.w16)


def _units(seq, name):
    """[_Unit] of an nn.Sequential of Conv2d / BatchNorm2d / ReLU / Dropout2d entries (Dropout2d: identity in eval mode)"""
    out, mods, i = [], list(seq), 0
    while i < len(mods):
        conv, bn, relu = mods[i], None, False
        j = i + 1
        if j < len(mods) and isinstance(mods[j], K.BatchNorm2d):
            bn = mods[j]
            j += 1
        if j < len(mods) and isinstance(mods[j], nn.ReLU):
            relu = True
            j += 1
        if j < len(mods) and isinstance(mods[j], nn.Dropout2d):
            j += 1
        out.append(_Unit(f"{name}.{i}", conv, bn, relu))
        i = j
    return out


class _Act:
    """an fp16 activation: `t` is a 2-D view [pixels][C] whose row stride is the pitch (a channel slice of a wider buffer)"""

    def __init__(self, t, N, H, W):
        self.t, self.N, self.H, self.W = t, N, H, W

    @property
    def C(self):
        return self.t.shape[1]

    @property
    def ld(self):
        return self.t.stride(0)


_out_size = K._out_size


def _pool_size(n):
    o = (n - 1 + 1) // 2 + 1           # ceil((n + 2 - 3) / 2) + 1
    return o - 1 if (o - 1) * 2 >= n + 1 else o


class HalfPredictor:
    def __init__(self, model):
        if not isinstance(model, ModelBuilder):
            raise TypeError(f"HalfPredictor: expected a ModelBuilder, got {type(model).__name__}")
        enc, dec = model.encoder, model.decoder
        if type(enc) is not ResNet:
            raise TypeError(f"HalfPredictor: encoder class {type(enc).__name__} is not known to the fp16 path (it keeps the "
                            "fp32 path)")
        if type(dec) not in (dec_deeplabv3_plus, dec_deeplabv3):
            raise TypeError(f"HalfPredictor: decoder class {type(dec).__name__} is not known to the fp16 path (it keeps the "
                            "fp32 path)")
        if isinstance(dec, dec_deeplabv3_plus) and not model.fpn:
            raise ValueError("HalfPredictor: dec_deeplabv3_plus needs the encoder's four feature maps (fpn=True)")
        self.model = model
        self.plus = isinstance(dec, dec_deeplabv3_plus)
        stem = list(enc.conv1)
        self.stem = _units(nn.Sequential(*stem[:-1]), "encoder.conv1") + [_Unit("encoder.conv1.6", stem[-1], enc.bn1, True)]
        self.blocks = []          # per layer: [(unit1, unit2, unit3 | None, downsample unit | None)]
        for li in range(1, 5):
            layer = []
            for bi, blk in enumerate(getattr(enc, f"layer{li}")):
                nm = f"encoder.layer{li}.{bi}"
                if type(blk) not in (Bottleneck, BasicBlock):
                    raise TypeError(f"HalfPredictor: {nm} is a {type(blk).__name__}, not known to the fp16 path")
                ds = None if blk.downsample is None else _Unit(nm + ".downsample.0", blk.downsample[0], blk.downsample[1], False)
                u1 = _Unit(nm + ".conv1", blk.conv1, blk.bn1, True)
                if isinstance(blk, Bottleneck):
                    u2, u3 = _Unit(nm + ".conv2", blk.conv2, blk.bn2, True), _Unit(nm + ".conv3", blk.conv3, blk.bn3, True)
                else:
                    u2, u3 = _Unit(nm + ".conv2", blk.conv2, blk.bn2, True), None
                layer.append((u1, u2, u3, ds))
            self.blocks.append(layer)
        aspp = dec.aspp
        if type(aspp) is not ASPP:
            raise TypeError(f"HalfPredictor: decoder.aspp is a {type(aspp).__name__}, not known to the fp16 path")
        self.aspp_pool = _units(nn.Sequential(*list(aspp.conv1)[1:]), "decoder.aspp.conv1")[0]
        self.aspp_branches = [_units(getattr(aspp, f"conv{k}"), f"decoder.aspp.conv{k}")[0] for k in (2, 3, 4, 5)]
        self.head = _units(dec.head, "decoder.head")
        if self.plus:
            self.low = _units(dec.low_conv, "decoder.low_conv")[0]
            self.classifier = _units(dec.classifier, "decoder.classifier")
        self.units = list(self.stem)
        for layer in self.blocks:
            for us in layer:
                self.units += [u for u in us if u is not None]
        self.units += [self.aspp_pool] + self.aspp_branches + self.head
        if self.plus:
            self.units += [self.low] + self.classifier
        for u in self.units[1:]:
            if u.conv.in_channels % 32:
                raise ValueError(f"HalfPredictor: {u.name} has {u.conv.in_channels} input channels; the fp16 GEMM needs a "
                                 "multiple of 32")
        self._activation_bytes = 0
        self._pool = {}           # (pixels, channels) -> [free fp16 buffers]: grows to the pass's live set, then reused
        self.sat = None
        self.calls = 0            # forward passes / those that saturated (the closing log line of infer.py, eval.py)
        self.saturated_calls = 0
        self.refresh()

    # ------------------------------------------------------------------ plan
    def refresh(self):
        """rebuild the fp16 weight planes and the fp32 scale / shift vectors from the model's current weights"""
        for u in self.units:
            u.refresh()
        dev = next(self.model.parameters()).device
        self.sat = torch.zeros(1, dtype=torch.int32, device=dev) if dev.type == "cuda" else None

    def bytes_allocated(self):
        """bytes of fp16 planes, scale / shift vectors and pooled activation buffers this predictor holds"""
        n = 0
        for u in self.units:
            for t in (u.w16, u.scale, u.shift):
                n += 0 if t is None else t.numel() * t.element_size()
        return n + self._activation_bytes

    def release_buffers(self):
        """drop the pooled activation buffers (they are per input shape; the next pass allocates its own)"""
        self._pool.clear()
        self._activation_bytes = 0

    def _take(self, M, C, dev):
        free = self._pool.setdefault((M, C), [])
        if free:
            return free.pop()
        self._activation_bytes += 2 * M * C
        return torch.empty((M, C), dtype=torch.float16, device=dev)

    def _give(self, act):
        t = act.t
        if t.is_contiguous() and t.storage_offset() == 0:      # (slices of concat buffers go back with their buffer)
            self._pool.setdefault((t.shape[0], t.shape[1]), []).append(t)

    # ------------------------------------------------------------------ layers
    def _conv(self, u, a, res=None, out=None, out_f32=False):
        conv = u.conv
        R, S = conv.kernel_size
        Ho, Wo = _out_size(a.H, R, conv.stride, conv.padding, conv.dilation), _out_size(a.W, S, conv.stride, conv.padding, conv.dilation)
        M, Cout = a.N * Ho * Wo, conv.out_channels
        if u.w16 is None:
            raise HipError("HalfPredictor: the model is not on the GPU (there is no CPU fallback)")
        if out is None:
            out = torch.empty((M, Cout), dtype=torch.float32, device=a.t.device) if out_f32 else self._take(M, Cout, a.t.device)
        if tuple(out.shape) != (M, Cout) or a.C != conv.in_channels or (res is not None and tuple(res.t.shape) != (M, Cout)):
            raise HipError(f"HalfPredictor: shape mismatch at {u.name}")
        call("u2pl_hconv2d_fwd_f16", a.t, a.ld, u.w16, u.scale, u.shift, None if res is None else res.t,
             0 if res is None else res.ld, out, out.stride(0), a.N, a.H, a.W, conv.in_channels, Ho, Wo, Cout, R, S, conv.stride,
             conv.padding, conv.dilation, int(u.relu), int(out_f32), 0, self.sat)
        return out if out_f32 else _Act(out, a.N, Ho, Wo)

    def _stem_first(self, u, x, N, H, W):
        conv = u.conv
        R, S = conv.kernel_size
        Ho, Wo = _out_size(H, R, conv.stride, conv.padding, conv.dilation), _out_size(W, S, conv.stride, conv.padding, conv.dilation)
        out = self._take(N * Ho * Wo, conv.out_channels, x.device)
        call("u2pl_hconv2d_stem_f16", x, conv.in_channels, u.w16, u.scale, u.shift, out, out.stride(0), N, H, W, conv.in_channels,
             Ho, Wo, conv.out_channels, R, S, conv.stride, conv.padding, conv.dilation, int(u.relu), self.sat)
        return _Act(out, N, Ho, Wo)

    def _block(self, us, x):
        u1, u2, u3, ds = us
        o1 = self._conv(u1, x)
        idt = x if ds is None else self._conv(ds, x)
        if u3 is None:                                   # BasicBlock
            y = self._conv(u2, o1, res=idt)
        else:
            o2 = self._conv(u2, o1)
            y = self._conv(u3, o2, res=idt)
            self._give(o2)
        self._give(o1)
        if ds is not None:
            self._give(idt)
        return y

    def _upsample(self, a, size, out):
        H, W = size
        call("u2pl_hbilinear_f16", a.t, a.ld, a.N, a.H, a.W, a.C, out, out.stride(0), H, W)
        return _Act(out, a.N, H, W)

    def _aspp(self, x):
        dev, inner = x.t.device, self.aspp_pool.conv.out_channels
        M = x.N * x.H * x.W
        cat = self._take(M, 5 * inner, dev)
        pooled = self._take(x.N, x.C, dev)
        call("u2pl_hgap_f16", x.t, x.ld, x.N, x.H * x.W, x.C, pooled)
        p = self._conv(self.aspp_pool, _Act(pooled, x.N, 1, 1))
        self._upsample(p, (x.H, x.W), cat[:, :inner])
        self._give(p)
        self._give(_Act(pooled, x.N, 1, 1))
        for k, u in enumerate(self.aspp_branches):       # each branch writes its channels of the concat buffer
            self._conv(u, x, out=cat[:, (k + 1) * inner:(k + 2) * inner])
        return _Act(cat, x.N, x.H, x.W)

    # ------------------------------------------------------------------ the pass
    @torch.no_grad()
    def __call__(self, x):
        """x: fp32 image batch (N, 3, H, W), read as NHWC memory: channels_last, what hipops.infer_input hands out and
        ModelBuilder uses (a planar batch is converted first).  -> (pred fp32 (N, C, h, w), saturated int)"""
        if not x.is_cuda or self.sat is None:
            raise HipError("HalfPredictor needs the model and the image on the GPU (there is no CPU fallback)")
        if x.dtype != torch.float32 or x.dim() != 4:
            raise HipError("HalfPredictor: expected a 4-d float32 image batch")
        if x.shape[1] != 3:
            raise HipError("HalfPredictor: expected an (N, 3, H, W) batch")
        x = x.contiguous(memory_format=torch.channels_last)      # NHWC in memory, pitch 3
        N, _, H, W = x.shape
        self.sat.zero_()
        a = self._stem_first(self.stem[0], x, N, H, W)
        for u in self.stem[1:]:
            b = self._conv(u, a)
            self._give(a)
            a = b
        Ho, Wo = _pool_size(a.H), _pool_size(a.W)
        pooled = self._take(N * Ho * Wo, a.C, x.device)
        call("u2pl_hmaxpool3s2_f16", a.t, a.ld, N, a.H, a.W, a.C, Ho, Wo, pooled, pooled.stride(0))
        self._give(a)
        a = _Act(pooled, N, Ho, Wo)
        x1 = None                                            # layer1's output, kept for the DeepLabv3+ decoder
        for li, layer in enumerate(self.blocks):
            for us in layer:
                b = self._block(us, a)
                if a is not x1:
                    self._give(a)
                a = b
            if li == 0 and self.plus:
                x1 = a
        cat = self._aspp(a)
        self._give(a)
        h = self._conv(self.head[0], cat)
        self._give(cat)
        if not self.plus:
            pred = self._conv(self.head[1], h, out_f32=True)
            self._give(h)
            ph, pw = h.H, h.W
        else:
            cat2 = self._take(x1.t.shape[0], 2 * self.low.conv.out_channels, x.device)
            lc = self.low.conv.out_channels
            self._conv(self.low, x1, out=cat2[:, :lc])
            self._upsample(h, (x1.H, x1.W), cat2[:, lc:])
            self._give(h)
            z = _Act(cat2, N, x1.H, x1.W)
            t1 = self._conv(self.classifier[0], z)
            t2 = self._conv(self.classifier[1], t1)
            pred = self._conv(self.classifier[2], t2, out_f32=True)
            for t in (z, t1, t2, x1):
                self._give(t)
            ph, pw = x1.H, x1.W
        self.calls += 1
        saturated = int(self.sat.item())                 # the one read-back of the call
        if saturated:
            self.saturated_calls += 1
        return pred.view(N, ph, pw, -1).permute(0, 3, 1, 2), saturated

    def log_line(self):
        return f"half: {self.calls} forward passes, {self.saturated_calls} redone in fp32"
