"""-m gpu: the fp16 prediction path (csrc/half.hip, u2pl_amd/half.py): every kernel against float64 with the bound of
tests/half_bounds.py or bit for bit, the saturation count, whole networks against a float64 emulation that rounds where the
plan stores, the fp32 fallback, evaluate(half=...) and the two command lines."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import half_bounds as HB
from model_utils import formula_state_dict, net_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SENT16, SENT32 = 0x7ACE, 0x7F7ACE01          # sentinel bit patterns of the output buffers (fp16 / fp32 words)


def _rows(x):
    """(N,C,H,W) float64 -> (N*H*W, C) array"""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)).reshape(-1, x.shape[1]))


def _half_weight(w):
    from u2pl_amd._lib import call
    Cout, Cin, R, S = w.shape
    out = torch.empty((Cout, R, S, Cin), dtype=torch.float16, device=DEV)
    call("u2pl_half_weight_f16", torch.from_numpy(w.astype(np.float32)).to(DEV).contiguous(), Cout, Cin, R, S, out)
    return out


def _run_conv(x, w, scale, shift, res, relu, stride, pad, dil, out_f32=False, x_off=0, ldx=None, y_off=0, ldy=None, tile=0):
    """-> (y (N,Cout,Ho,Wo) float64, the whole output buffer as integer words, saturation count)"""
    from u2pl_amd._lib import call
    N, Cin, H, W = x.shape
    Cout, _, R, S = w.shape
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    ldx, ldy = ldx or Cin, ldy or Cout
    xb = torch.full((N * H * W, ldx), 777.0, dtype=torch.float16, device=DEV)
    xb[:, x_off:x_off + Cin] = torch.from_numpy(_rows(x)).to(DEV).half()
    M = N * Ho * Wo
    if out_f32:
        yb = torch.from_numpy(np.full((M, ldy), SENT32, np.int32)).to(DEV).view(torch.float32)
    else:
        yb = torch.from_numpy(np.full((M, ldy), SENT16, np.int16)).to(DEV).view(torch.float16)
    rb = None if res is None else torch.from_numpy(_rows(res)).to(DEV).half().contiguous()
    sc = None if scale is None else torch.from_numpy(np.asarray(scale, np.float32)).to(DEV)
    sh = None if shift is None else torch.from_numpy(np.asarray(shift, np.float32)).to(DEV)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("u2pl_hconv2d_fwd_f16", xb[:, x_off:], ldx, _half_weight(w), sc, sh, rb, 0 if rb is None else Cout, yb[:, y_off:], ldy,
         N, H, W, Cin, Ho, Wo, Cout, R, S, stride, pad, dil, int(relu), int(out_f32), tile, sat)
    torch.cuda.synchronize()
    words = yb.view(torch.int32 if out_f32 else torch.int16).cpu().numpy()
    y = yb[:, y_off:y_off + Cout].double().cpu().numpy().reshape(N, Ho, Wo, Cout).transpose(0, 3, 1, 2)
    return y, words, int(sat.item())


# name: (N, Ho, Wo, Cin, Cout, k, stride, dil, res, relu, scale, out_f32, x_off, ldx, y_off, ldy)
CONV_CASES = {
    "99px_32to19_1x1":            (1, 9, 11, 32, 19, 1, 1, 1, True, True, True, False, 0, None, 3, 40),
    "578px_96to21_3x3":           (2, 17, 17, 96, 21, 3, 1, 1, True, True, True, False, 0, None, 0, None),
    "578px_256to64_3x3_s2":       (2, 17, 17, 256, 64, 3, 2, 1, False, True, True, False, 0, None, 64, 192),
    "99px_256to160_1x1_s2_down":  (1, 9, 11, 256, 160, 1, 2, 1, False, False, True, False, 0, None, 0, None),
    "578px_96to256_3x3_d2":       (2, 17, 17, 96, 256, 3, 1, 2, True, True, True, False, 0, None, 256, 1280),
    "81px_32to160_3x3_d12":       (1, 9, 9, 32, 160, 3, 1, 12, False, True, True, False, 0, None, 0, None),
    "578px_96to64_1x1_slice_in":  (2, 17, 17, 96, 64, 1, 1, 1, False, True, True, False, 8, 136, 0, None),
    "99px_96to19_1x1_bias_f32":   (1, 9, 11, 96, 19, 1, 1, 1, False, False, False, True, 0, None, 2, 24),
    "578px_256to21_1x1_f32":      (2, 17, 17, 256, 21, 1, 1, 1, True, True, True, True, 0, None, 0, None),
    "578px_256to256_3x3":         (2, 17, 17, 256, 256, 3, 1, 1, True, False, True, False, 0, None, 0, None),
    "99px_32to160_3x3_noscale":   (1, 9, 11, 32, 160, 3, 1, 1, True, True, False, False, 0, None, 1, 168),
}


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    N, Ho, Wo, Cin, Cout, k, stride, dil, has_res, relu, has_scale, out_f32 = CONV_CASES[name][:12]
    rng = np.random.default_rng(sum(map(ord, name)))
    pad = dil * (k - 1) // 2
    H, W = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1            # the output size above for 1x1 / 'same' 3x3 at this stride
    x, w = HB.draw(rng, (N, Cin, H, W)), HB.draw(rng, (Cout, Cin, k, k), lo=-10, hi=0)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32) * rng.choice([-1, 1], Cout) if has_scale else None
    shift = rng.uniform(-2, 2, Cout).astype(np.float32)
    res = HB.draw(rng, (N, Cout, Ho, Wo)) if has_res else None
    ref, bound = HB.layer_ref(x, w, scale, shift, res, relu, stride, pad, dil, out_f32)
    assert ref.shape == (N, Cout, Ho, Wo) and np.abs(ref).max() < 6e4
    return x, w, scale, shift, res, relu, stride, pad, dil, out_f32, ref, bound


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_within_the_float64_bound(name, tile):
    x, w, scale, shift, res, relu, stride, pad, dil, out_f32, ref, bound = _conv_case(name)
    x_off, ldx, y_off, ldy = CONV_CASES[name][12:]
    y, words, sat = _run_conv(x, w, scale, shift, res, relu, stride, pad, dil, out_f32, x_off, ldx, y_off, ldy, tile)
    ex = HB.excess(y, ref, bound)
    print(f"{name} tile {tile}: max |got - ref64| / bound = {ex:.4f}, max |ref| {np.abs(ref).max():.4g}")
    assert np.isfinite(y).all() and ex <= 1.0
    assert sat == 0
    Cout = w.shape[0]
    outside = np.ones(words.shape[1], bool)
    outside[y_off:y_off + Cout] = False
    sent = np.int32(SENT32) if out_f32 else np.int16(SENT16)
    assert (words[:, outside] == sent).all()          # every element outside the slice keeps its bits
    if name == "81px_32to160_3x3_d12":                # only the centre tap is inside: the 1x1 of the centre weights
        ref1, _ = HB.layer_ref(x, w[:, :, 1:2, 1:2], scale, shift, res, relu)
        assert np.allclose(ref1, ref, rtol=1e-12, atol=1e-12)


def test_conv_two_runs_give_identical_bits():
    x, w, scale, shift, res, relu, stride, pad, dil, out_f32, _, _ = _conv_case("578px_96to256_3x3_d2")
    a = _run_conv(x, w, scale, shift, res, relu, stride, pad, dil, out_f32)[1]
    b = _run_conv(x, w, scale, shift, res, relu, stride, pad, dil, out_f32)[1]
    assert np.array_equal(a, b)


def _run_stem(x, w, scale, shift, relu, stride, pad, dil, y_off=0, ldy=None):
    from u2pl_amd._lib import call
    N, Cin, H, W = x.shape
    Cout, _, R, S = w.shape
    Ho, Wo = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1, (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    ldy = ldy or Cout
    xb = torch.from_numpy(_rows(x).astype(np.float32)).to(DEV)
    yb = torch.from_numpy(np.full((N * Ho * Wo, ldy), SENT16, np.int16)).to(DEV).view(torch.float16)
    sat = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("u2pl_hconv2d_stem_f16", xb, Cin, _half_weight(w), None if scale is None else torch.from_numpy(scale).to(DEV),
         None if shift is None else torch.from_numpy(shift).to(DEV), yb[:, y_off:], ldy, N, H, W, Cin, Ho, Wo, Cout, R, S, stride,
         pad, dil, int(relu), sat)
    torch.cuda.synchronize()
    y = yb[:, y_off:y_off + Cout].double().cpu().numpy().reshape(N, Ho, Wo, Cout).transpose(0, 3, 1, 2)
    return y, yb.view(torch.int16).cpu().numpy(), int(sat.item())


def test_stem_from_the_fp32_image_65_to_33():
    rng = np.random.default_rng(65)
    x = rng.standard_normal((2, 3, 65, 65)).astype(np.float32).astype(np.float64)       # an fp32 image, not fp16 values
    w = HB.draw(rng, (64, 3, 3, 3), lo=-6, hi=0)
    scale, shift = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.uniform(-1, 1, 64).astype(np.float32)
    ref, bound = HB.layer_ref(x, w, scale, shift, None, True, 2, 1, 1)
    assert ref.shape == (2, 64, 33, 33)
    y, words, sat = _run_stem(x, w, scale, shift, True, 2, 1, 1, y_off=8, ldy=80)
    ex = HB.excess(y, ref, bound)
    print(f"stem: max |got - ref64| / bound = {ex:.4f}")
    assert ex <= 1.0 and sat == 0
    assert (words[:, :8] == np.int16(SENT16)).all() and (words[:, 72:] == np.int16(SENT16)).all()


def test_saturation_is_clamped_and_counted_exactly():
    """exact results a_p * b_c, all fp16-representable: every magnitude is below 6e4 (57344 at most) or above 7e4 (71680 at least)"""
    a = np.array([1.0, 2.0, 256.0, -320.0])
    b = np.array([100.0, 224.0, -288.0])
    rng = np.random.default_rng(7)
    N, H, W, Cin, Cout = 2, 9, 11, 32, 21
    x = np.zeros((N, Cin, H, W))
    x[:, 5] = rng.choice(a, (N, H, W))
    w = np.zeros((Cout, Cin, 1, 1))
    w[:, 5, 0, 0] = rng.choice(b, Cout)
    exact = x[:, 5][:, None] * w[:, 5, 0, 0][None, :, None, None]
    mag = np.abs(exact)
    assert ((mag < 6e4) | (mag > 7e4)).all() and (mag > 7e4).sum() > 100
    assert np.array_equal(exact[mag < 6e4], exact[mag < 6e4].astype(np.float16).astype(np.float64))
    want = np.where(mag > 7e4, np.sign(exact) * 65504.0, exact)
    counts = []
    for rep in range(2):                               # a second call with a zeroed counter reports the same number
        y, _, sat = _run_conv(x, w, None, None, None, False, 1, 0, 1, y_off=3, ldy=32)
        assert np.isfinite(y).all() and np.array_equal(y, want)
        counts.append(sat)
    assert counts == [int((mag > 7e4).sum())] * 2
    # the direct (stem) kernel clamps and counts the same way
    xs = np.zeros((N, 3, H, W))
    xs[:, 1] = x[:, 5]
    ws = np.zeros((Cout, 3, 1, 1))
    ws[:, 1] = w[:, 5]
    y, _, sat = _run_stem(xs, ws, None, None, False, 1, 0, 1)
    assert np.array_equal(y, want) and sat == counts[0]


@pytest.mark.parametrize("size", [33, 34])
def test_maxpool_bit_equal_to_torch_cpu(size):
    from u2pl_amd._lib import call
    g = torch.Generator().manual_seed(size)
    N, C = 2, 24
    x = (torch.randn(N, C, size, size, generator=g) * 4).half()
    want = F.max_pool2d(x.float(), 3, 2, 1, ceil_mode=True).half()          # (exact: a maximum of fp16 values)
    Ho = want.shape[2]
    assert Ho == {33: 17, 34: 18}[size]
    xb = torch.full((N * size * size, 40), 9.0, dtype=torch.float16, device=DEV)
    xb[:, 8:8 + C] = x.permute(0, 2, 3, 1).reshape(-1, C).to(DEV)
    yb = torch.from_numpy(np.full((N * Ho * Ho, 32), SENT16, np.int16)).to(DEV).view(torch.float16)
    call("u2pl_hmaxpool3s2_f16", xb[:, 8:], 40, N, size, size, C, Ho, Ho, yb[:, 8:], 32)
    got = yb[:, 8:].reshape(N, Ho, Ho, C).permute(0, 3, 1, 2).contiguous().cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert (yb.view(torch.int16)[:, :8].cpu() == SENT16).all()


@pytest.mark.parametrize("lo,hi", [(9, 33), (1, 9), (17, 25)])
def test_bilinear_bit_equal_to_the_fp32_kernel_rounded_once(lo, hi):
    from u2pl_amd import hipops as H
    from u2pl_amd._lib import call
    g = torch.Generator().manual_seed(lo * 100 + hi)
    N, C = 2, 16
    x = (torch.randn(N, C, lo, lo, generator=g) * 8).half()
    want = H.bilinear_up(x.float().to(DEV), (hi, hi)).half().cpu()
    xb = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    yb = torch.from_numpy(np.full((N * hi * hi, 48), SENT16, np.int16)).to(DEV).view(torch.float16)
    call("u2pl_hbilinear_f16", xb, C, N, lo, lo, C, yb[:, 16:], 48, hi, hi)
    got = yb[:, 16:32].reshape(N, hi, hi, C).permute(0, 3, 1, 2).cpu()
    assert torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16))
    words = yb.view(torch.int16).cpu()
    assert (words[:, :16] == SENT16).all() and (words[:, 32:] == SENT16).all()


@pytest.mark.parametrize("hw", [81, 289])
def test_global_average_within_its_bound(hw):
    from u2pl_amd._lib import call
    g = torch.Generator().manual_seed(hw)
    N, C = 2, 96
    x = (torch.randn(N, hw, C, generator=g) * 3 + 1).half()
    xb = torch.zeros((N * hw, 104), dtype=torch.float16, device=DEV)
    xb[:, 8:] = x.reshape(-1, C).to(DEV)
    out = torch.empty((N, C), dtype=torch.float16, device=DEV)
    call("u2pl_hgap_f16", xb[:, 8:], 104, N, hw, C, out)
    ref = x.double().mean(1)
    bound = hw * 2.0 ** -24 * x.double().abs().mean(1) + 2.0 ** -11 * ref.abs()
    err = (out.cpu().double() - ref).abs()
    print(f"gap over {hw}: max err / bound = {(err / bound).max().item():.4f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------- whole networks
def _r16(t):
    return t.half().to(t.dtype)


class _RefV3(nn.Module):
    """float64 reference of ModelBuilder(fpn=False, dec_deeplabv3, aux head): the oracle's encoder and ASPP, the head here"""

    def __init__(self, arch, C):
        super().__init__()
        from oracle import model_ref as MR
        self.encoder = MR.Encoder(arch)
        self.decoder = nn.Module()
        self.decoder.aspp = MR.Aspp(2048)
        self.decoder.head = nn.Sequential(nn.Conv2d(1280, 256, 3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(True),
                                          nn.Dropout2d(0.1), nn.Conv2d(256, C, 1))
        self.auxor = MR.AuxHead(1024, C)

    def forward(self, x):
        return {"pred": self.decoder.head(self.decoder.aspp(self.encoder(x)[3]))}


def _cfg(kind, C):
    cfg = net_cfg("resnet50", C, True)
    if kind == "v3":
        cfg["encoder"]["kwargs"]["fpn"] = False
        cfg["decoder"] = dict(type="u2pl.models.decoder.dec_deeplabv3", kwargs=dict(inner_planes=256, dilations=[12, 24, 36]))
    return cfg


@functools.lru_cache(maxsize=None)
def _net_case(kind, C, size, N):
    """model on the GPU with formula weights, its image batch, and the float64 `exact` / `rounded` predictions"""
    from oracle import model_ref as MR
    from u2pl_amd.models.model_helper import ModelBuilder
    m = ModelBuilder(_cfg(kind, C))
    sd = formula_state_dict(m)
    m.load_state_dict(sd)
    x = torch.randn(N, 3, size, size, generator=torch.Generator().manual_seed(size + C))
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}

    def ref_net(state):
        r = (MR.RefNet("resnet50", C, True, p_drop=0.0) if kind == "plus" else _RefV3("resnet50", C)).double().eval()
        r.load_state_dict(state)
        return r

    with torch.no_grad():
        exact = ref_net(sd64)(x.double())["pred"]
        # the same network with fp16 weights and activations rounded where the plan stores them: after every ReLU, after
        # the downsample branch, the pools and each up-sample
        net = ref_net({k: _r16(v) if v.dim() == 4 else v for k, v in sd64.items()})
        for name, mod in net.named_modules():
            if isinstance(mod, (nn.ReLU, nn.MaxPool2d, nn.AdaptiveAvgPool2d)) or name.endswith(".downsample"):
                mod.register_forward_hook(lambda _m, _i, out: _r16(out))
        saved = MR.F
        MR.F = types.SimpleNamespace(interpolate=lambda *a, **k: _r16(F.interpolate(*a, **k)))
        try:
            rounded = net(x.double())["pred"]
        finally:
            MR.F = saved
    return m.to(DEV).eval(), x, exact, rounded


NET_CASES = [("plus", 19, 65, 2), ("plus", 21, 97, 1), ("v3", 19, 65, 2)]


@pytest.mark.parametrize("kind,C,size,N", NET_CASES)
def test_network_against_the_float64_emulation(kind, C, size, N):
    """measured multiples are printed; DESIGN section 3.9 quotes them"""
    from u2pl_amd.half import HalfPredictor
    m, x, exact, rounded = _net_case(kind, C, size, N)
    dev = (rounded - exact).abs()
    e_max, e_rms = dev.max().item(), dev.pow(2).mean().sqrt().item()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    pred, saturated = HalfPredictor(m)(xd)
    assert tuple(pred.shape) == tuple(exact.shape) and pred.dtype == torch.float32
    err = (pred.cpu().double() - exact).abs()
    g_max, g_rms = err.max().item(), err.pow(2).mean().sqrt().item()
    with torch.no_grad():
        out32 = m(xd, need_aux=False, need_rep=False)
    out32 = (out32["pred"] if isinstance(out32, dict) else out32).cpu()
    top2 = exact.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 2 * e_max
    left_out = 1.0 - clear.double().mean().item()
    wrong = int(((pred.cpu().argmax(1) != out32.argmax(1)) & clear).sum())
    print(f"{kind} C={C} {size}^2: E_max {e_max:.3f} E_rms {e_rms:.3f} max|logit| {exact.abs().max().item():.0f}; half path "
          f"max {g_max:.3f} = {g_max / e_max:.3f} E_max, rms {g_rms:.3f} = {g_rms / e_rms:.3f} E_rms; saturated {saturated}; "
          f"pixels left out by the margin {left_out:.4f}; arg-max differences outside it {wrong}")
    assert g_max <= 2 * e_max and g_rms <= 2 * e_rms
    assert saturated == 0
    assert left_out <= 0.10
    assert wrong == 0


def _lut():
    from u2pl_amd.infer import normalise_lut
    return torch.from_numpy(normalise_lut([123.675, 116.28, 103.53], [58.395, 57.12, 57.375])).to(DEV)


def test_infer_image_falls_back_to_fp32_when_the_pass_saturates():
    """the 65^2 image scaled by 40: with formula weights the activations pass 65504"""
    from u2pl_amd import infer as I
    from u2pl_amd.half import HalfPredictor
    m = _net_case("plus", 19, 65, 2)[0]
    half = HalfPredictor(m)
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (65, 65, 3), dtype=np.uint8)).to(DEV)
    lut = _lut()
    label, _, pred, fell_back = I.infer_image(m, img, lut, (65, 65), half=half)
    assert not fell_back and label.shape == (65, 65)
    out = I.infer_image(m, img, lut * 40, (65, 65))
    assert len(out) == 3
    label40, rgb40, pred40, fell_back = I.infer_image(m, img, lut * 40, (65, 65), half=half)
    assert fell_back and rgb40 is None
    assert torch.equal(label40, out[0]) and torch.equal(pred40.view(torch.int32), out[2].view(torch.int32))
    assert (half.calls, half.saturated_calls) == (2, 1)
    assert half.log_line() == "half: 2 forward passes, 1 redone in fp32"


def test_evaluate_with_half_on_the_sliding_window_case():
    """70 x 100 sliding-window image of tests/test_gpu_eval.py's data: per-class histograms within the pixels the margin
    rule leaves out"""
    from conftest import golden
    from u2pl_amd import evaluate as E
    from u2pl_amd.half import HalfPredictor
    m, _, exact, rounded = _net_case("plus", 19, 65, 2)
    e_max = (rounded - exact).abs().max().item()
    x = torch.from_numpy(golden("evalwin_70x100")["x"])[0]
    lab = torch.randint(0, 19, (70, 100), generator=torch.Generator().manual_seed(4)).numpy().astype(np.uint8)
    lab[:3] = 255
    kw = dict(base_size=100, crop=(65, 65), scales=(1.0,), use_crop=True)
    half = HalfPredictor(m)
    maps = {}
    miou32, _ = E.evaluate(m, [(x, lab)], 19, on_prediction=lambda i, g: maps.__setitem__("fp32", g), **kw)
    miou16, _ = E.evaluate(m, [(x, lab)], 19, on_prediction=lambda i, g: maps.__setitem__("half", g), half=half, **kw)
    logits = E.predict_image(m, x.unsqueeze(0).to(DEV), 19, kw["base_size"], kw["crop"], kw["scales"], True).cpu().double()
    top2 = logits.topk(2, dim=0).values
    unclear = int(((top2[0] - top2[1]) < 2 * e_max).sum())
    h32 = np.bincount(maps["fp32"].ravel(), minlength=19)
    h16 = np.bincount(maps["half"].ravel(), minlength=19)
    print(f"mIoU fp32 {miou32:.6f} half {miou16:.6f}; pixels inside the margin {unclear} of {lab.size}; "
          f"histogram differences {np.abs(h32 - h16).sum()}; {half.log_line()}")
    assert half.calls == 4 and half.saturated_calls == 0          # 2 x 2 windows
    assert unclear <= 0.10 * lab.size
    assert np.abs(h32 - h16).max() <= unclear
    assert int((maps["fp32"] != maps["half"]).sum()) <= unclear


def test_half_command_lines(tmp_path):
    import make_synth_dataset as M
    import yaml
    from PIL import Image
    from u2pl_amd import infer as I
    from u2pl_amd.half import HalfPredictor
    from u2pl_amd.models.model_helper import ModelBuilder

    d, s = M.make_cityscapes(str(tmp_path), H=70, W=100)
    cfgp = M.write_city_config(str(tmp_path), d, s, crop=65, epochs=1)
    cfg = yaml.load(open(cfgp), Loader=yaml.Loader)
    model = ModelBuilder(cfg["net"])
    sd = formula_state_dict(model)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"teacher_state": {"module." + k: v for k, v in sd.items()}}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(script, out, *extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--config", cfgp, "--model_path", ckpt,
                            "--save_folder", out, "--half", *extra], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout + r.stderr

    names = [ln.strip() for ln in open(cfg["dataset"]["val"]["data_list"]) if ln.strip()]
    lut = torch.from_numpy(I.normalise_lut(cfg["dataset"]["mean"], cfg["dataset"]["std"])).to(DEV)
    half = HalfPredictor(model)
    out = str(tmp_path / "viewer")
    text = run("infer.py", out, "--input_scale", "65", "65")
    redone = 0
    for rel in names:
        name = os.path.basename(rel)
        img = np.array(Image.open(os.path.join(d, rel)).convert("RGB"))
        gray, color = np.array(Image.open(os.path.join(out, "gray", name))), np.array(Image.open(os.path.join(out, "color", name)))
        assert gray.dtype == np.uint8 and gray.shape == img.shape[:2] and color.shape == (*img.shape[:2], 3)
        label, _, _, fell_back = I.infer_image(model, torch.from_numpy(img).to(DEV), lut, (65, 65), half=half)
        redone += int(fell_back)
        assert np.array_equal(gray, label.cpu().numpy())
    assert f"half: {len(names)} forward passes, {redone} redone in fp32" in text
    out = str(tmp_path / "results")
    text = run("eval.py", out, "--crop", "--base_size", "100")
    assert "mIoU" in text
    line = [ln for ln in text.splitlines() if ln.startswith("half: ")]
    assert len(line) == 1
    passes, again = int(line[0].split()[1]), int(line[0].split()[4])
    assert passes == 4 * len(names) and 0 <= again <= passes       # 2 x 2 windows of 65 x 65 per 70 x 100 image
    for rel in names:
        name = os.path.basename(rel).split(".")[0] + ".png"
        assert np.array(Image.open(os.path.join(out, "gray", name))).shape == (70, 100)
        assert np.array(Image.open(os.path.join(out, "color", name))).shape == (70, 100, 3)
