"""Thin torch <-> C-ABI glue for the loss/reliability/contrastive kernels.

Everything numeric happens in libu2pl_hip.so; torch supplies device memory,
the current HIP stream and the autograd tape (torch.autograd.Function)."""
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, query

SEL_WORD_VAL = 40
SEL_WORD_THR = 56
MAXC = 32          # the narrow route: a pixel's class bits in one 32-bit word (csrc/contrast.hip)
WIDE_MAXC = 255    # the wide route: class bits as word planes (csrc/contrast_wide.hip); label value 255 is the ignore value


def wide_words(C):
    """32-bit planes that hold the class bits of C classes"""
    return (int(C) + 31) // 32


def check_num_classes(C, what="num_classes"):
    """2 .. 255 classes train; more cannot, labels are bytes and 255 is the ignore value"""
    if int(C) > WIDE_MAXC:
        raise ValueError(f"{what} = {int(C)}: too many classes, at most {WIDE_MAXC} are supported "
                         "(label value 255 is the ignore value)")
    if int(C) < 1:
        raise ValueError(f"{what} = {int(C)}: expected a positive class count")


def _class_bits(num_classes, pixels, dev, wide=None):
    """the class-bit tensor of `pixels` = (N, h, w) and what selects its C symbols -> (bits, suffix, extra arguments):
    one int32 word per pixel, "" and (); or -- wide: num_classes > 32 unless the caller forces it -- word planes
    (W, N, h, w), "_wide" and (num_classes,), the class count the *_wide reliability entry points take"""
    if wide is None:
        wide = num_classes is not None and int(num_classes) > MAXC
    if not wide:
        return torch.empty(tuple(pixels), dtype=torch.int32, device=dev), "", ()
    check_num_classes(num_classes)
    bits = torch.empty((wide_words(num_classes),) + tuple(pixels), dtype=torch.int32, device=dev)
    return bits, "_wide", (int(num_classes),)


def _f32c(x):
    if x.dtype != torch.float32:
        raise _lib.HipError("expected float32 tensor")
    return x


def _chk_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.HipError("u2pl_amd ops need GPU tensors; there is no CPU fallback")


def _strides_nchw(x):
    """(sn, sc, sh, sw) in elements of a 4-d tensor."""
    return x.stride(0), x.stride(1), x.stride(2), x.stride(3)


# --------------------------------------------------------------------------- bilinear
class _BilinearUp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        _chk_cuda(x)
        N, C, h, w = x.shape
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
        call("u2pl_bilinear_up_f32", _f32c(x), *_strides_nchw(x), N, C, h, w, out, H, W)
        ctx.in_meta = (x.shape, x.stride())
        return out

    @staticmethod
    def backward(ctx, g):
        shape, stride = ctx.in_meta
        N, C, h, w = shape
        g = g.contiguous()
        gin = torch.empty_strided(shape, stride, dtype=torch.float32, device=g.device)
        call("u2pl_bilinear_up_bwd_f32", g, N, C, g.shape[2], g.shape[3], gin, *stride, h, w)
        return gin, None, None


def bilinear_up(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) -> NCHW contiguous."""
    return _BilinearUp.apply(x, int(size[0]), int(size[1]))


# --------------------------------------------------------------------------- prediction maps (infer.py, eval.py dumps)
def _u8c(x, what):
    if x.dtype != torch.uint8:
        raise _lib.HipError(f"{what}: expected a uint8 tensor")
    return x.contiguous()


def predict_map(logits_low, size, palette=None):
    """argmax_c F.interpolate(logits_low, size, 'bilinear', align_corners=True) -> (label uint8 (N,H,W), rgb uint8
    (N,H,W,3) = palette[label] or None); the (N,C,H,W) logits are never written.  logits_low may be any strided
    (N,C,h,w) view; palette: (256,3) uint8 on the same device.  Lowest class index wins a tie."""
    _chk_cuda(logits_low, palette)
    N, C, h, w = logits_low.shape
    H, W = int(size[0]), int(size[1])
    label = torch.empty((N, H, W), dtype=torch.uint8, device=logits_low.device)
    rgb = None
    if palette is not None:
        if tuple(palette.shape) != (256, 3):
            raise _lib.HipError("palette: expected shape (256, 3)")
        palette = _u8c(palette, "palette")
        rgb = torch.empty((N, H, W, 3), dtype=torch.uint8, device=logits_low.device)
    call("u2pl_predict_map_f32", _f32c(logits_low), *_strides_nchw(logits_low), N, C, h, w, H, W, label, palette, rgb)
    return label, rgb


def lut_u8(x, lut, out=None):
    """out[i] = lut[x[i]] over a contiguous uint8 tensor (u2pl_lut_u8); lut: (256,) uint8 on the same device.  out=None
    writes in place (out is x); -> out.  --raw_ids: class indices to the dataset's raw ids."""
    _chk_cuda(x, lut, out)
    if tuple(lut.shape) != (256,):
        raise _lib.HipError("lut: expected shape (256,)")
    lut = _u8c(lut, "lut")
    if x.dtype != torch.uint8 or not x.is_contiguous():
        raise _lib.HipError("lut_u8: expected a contiguous uint8 tensor")
    if out is None:
        out = x
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != x.numel():
        raise _lib.HipError("lut_u8: out must be a contiguous uint8 tensor of x's size")
    call("u2pl_lut_u8", x, out, x.numel(), lut)
    return out


def window_fuse(pred, count, logits, origin, size, flip=False, softmax=False, weight=1.0, bump=True):
    """One view of test-time flip / probability fusion, in place: F.interpolate(logits, size, 'bilinear',
    align_corners=True), mirrored back along the width when flip, softmax over the classes when softmax, times weight,
    added into pred[:, h0:h0+hc, w0:w0+wc]; with bump, count gains 1 inside that window.  pred: contiguous (C,H,W) or
    (1,C,H,W) float32; count: contiguous (H,W) float32, or None when bump is off; logits: any strided (C,h,w) or
    (1,C,h,w) view.  The interpolated logits are never written."""
    _chk_cuda(pred, count, logits)
    if logits.dim() == 4:
        if logits.shape[0] != 1:
            raise _lib.HipError("window_fuse: one view at a time")
        logits = logits[0]
    if pred.dim() == 4 and pred.shape[0] == 1:
        pred = pred[0]
    if pred.dim() != 3 or logits.dim() != 3 or pred.shape[0] != logits.shape[0] or not pred.is_contiguous():
        raise _lib.HipError("window_fuse: expected a contiguous (C,H,W) accumulator and (C,h,w) logits of the same C")
    C, Hh, Ww = pred.shape
    if bump and count is None:
        raise _lib.HipError("window_fuse: bump needs a count map")
    if count is not None and (tuple(count.shape) != (Hh, Ww) or not count.is_contiguous() or count.dtype != torch.float32):
        raise _lib.HipError("window_fuse: expected a contiguous (H,W) float32 count map")
    call("u2pl_window_fuse_f32", _f32c(pred), count, C, Hh, Ww, _f32c(logits), logits.stride(0), logits.stride(1),
         logits.stride(2), logits.shape[1], logits.shape[2], int(origin[0]), int(origin[1]), int(size[0]), int(size[1]),
         int(bool(flip)), int(bool(softmax)), float(weight), int(bool(bump)))


def predict_entropy(scores_low, size, prob=False):
    """label and softmax entropy of every pixel of F.interpolate(scores_low, size, 'bilinear', align_corners=True) in one
    launch -> (label uint8 (N,H,W) = predict_map's bits, entropy float32 (N,H,W)); the (N,C,H,W) scores are never written.
    prob=False: the scores are logits, the entropy is that of their softmax (entropy_map_up's bits); prob=True: they are
    non-negative class weights (what window_fuse(softmax=True) accumulates), normalised by their sum; a pixel whose weights
    sum to nothing gets log(C).  scores_low may be any strided (N,C,h,w) view."""
    _chk_cuda(scores_low)
    N, C, h, w = scores_low.shape
    H, W = int(size[0]), int(size[1])
    label = torch.empty((N, H, W), dtype=torch.uint8, device=scores_low.device)
    ent = torch.empty((N, H, W), dtype=torch.float32, device=scores_low.device)
    call("u2pl_predict_entropy_f32", _f32c(scores_low), *_strides_nchw(scores_low), N, C, h, w, H, W, int(bool(prob)), label, ent)
    return label, ent


def entropy_threshold(entropy, percent):
    """np.percentile(entropy.ravel(), percent) as a one-element float32 device tensor (a view of a fresh select workspace):
    every pixel is valid, the workspace's two counts are set on the device and the host waits for nothing."""
    _chk_cuda(entropy)
    ent = _f32c(entropy).contiguous()
    ws = new_select_ws(ent.device, ent.numel())
    ws[0:2].fill_(ent.numel())          # n_valid = n_total; the pass-0 histogram is the select's own (ws._hist0 stays False)
    return run_select(ent, ws, [("pct", float(percent))])


def reliable_map(label, entropy, thr=None, palette=None, heat_classes=None):
    """the reference's drop rule (loss_helper.py:41-43) on a uint8 label map, in place: label[entropy >= thr] = 255, then
    rgb = palette[label] and heat = the entropy as a byte, 255 = log(heat_classes).  thr: one-element float32 device tensor
    (entropy_threshold) or None: nothing is dropped.  -> (rgb uint8 label.shape + (3,) | None, heat uint8 | None,
    ndropped one-element int32 device tensor | None)."""
    _chk_cuda(label, entropy, thr, palette)
    if label.dtype != torch.uint8 or not label.is_contiguous():
        raise _lib.HipError("reliable_map: expected a contiguous uint8 label map (it is rewritten in place)")
    if entropy.shape != label.shape or not entropy.is_contiguous():
        raise _lib.HipError("reliable_map: expected a contiguous entropy map of the label map's shape")
    dev = label.device
    rgb = heat = ndropped = None
    scale = 0.0
    if heat_classes is not None:
        if int(heat_classes) < 2:
            raise _lib.HipError("reliable_map: the heat map needs at least two classes (255 = log(classes))")
        scale = float(np.float32(255 / math.log(int(heat_classes))))
        heat = torch.empty(label.shape, dtype=torch.uint8, device=dev)
    if thr is not None:
        if heat_classes is not None and int(heat_classes) > 255:
            raise _lib.HipError("reliable_map: 255 is the ignore value, a threshold needs C <= 255")
        if thr.dtype != torch.float32 or thr.numel() != 1:
            raise _lib.HipError("reliable_map: expected a one-element float32 threshold")
        ndropped = torch.zeros(1, dtype=torch.int32, device=dev)
    if palette is not None:
        if tuple(palette.shape) != (256, 3):
            raise _lib.HipError("palette: expected shape (256, 3)")
        palette = _u8c(palette, "palette")
        rgb = torch.empty(tuple(label.shape) + (3,), dtype=torch.uint8, device=dev)
    call("u2pl_reliable_map_u8", label, _f32c(entropy), thr, label.numel(), palette, rgb, heat, scale, ndropped)
    return rgb, heat, ndropped


def check_drop_percent(drop_percent):
    """trainer.unsupervised.drop_percent's meaning: the share of pixels kept, a percentile in [0, 100]"""
    if drop_percent is not None and not 0.0 <= float(drop_percent) <= 100.0:
        raise ValueError(f"drop_percent is a percentile in [0, 100], got {drop_percent!r}")


def predict_reliable(scores_low, size, prob=False, palette=None, drop_percent=None, heat=False):
    """the prediction epilogue with reliability: predict_entropy, then with drop_percent = P the per-image threshold
    np.percentile(entropy, P) (entropy_threshold; the 100 - P per cent highest-entropy pixels become 255), then reliable_map
    for the drop, the colours and the heat bytes.  One image at a time (the threshold is per image).
    -> (label (1,H,W), rgb (1,H,W,3) | None, dict(entropy (H,W), heat (H,W) | None, threshold | None, ndropped | None))."""
    check_drop_percent(drop_percent)
    N, C = scores_low.shape[:2]
    if N != 1:
        raise _lib.HipError("predict_reliable: one image at a time")
    if drop_percent is not None and C > 255:
        raise _lib.HipError("predict_reliable: 255 is the ignore value, a threshold needs C <= 255")
    label, ent = predict_entropy(scores_low, size, prob)
    thr = None if drop_percent is None else entropy_threshold(ent, drop_percent)
    rgb = hmap = ndropped = None
    if thr is not None or palette is not None or heat:
        rgb, hmap, ndropped = reliable_map(label, ent, thr, palette, C if heat else None)
    return label, rgb, dict(entropy=ent[0], heat=None if hmap is None else hmap[0], threshold=thr, ndropped=ndropped)


def infer_input(img_u8_hwc, lut, size):
    """decoded image (h,w,3) uint8 -> network input (1,3,H,W) float32 in channels_last memory: lut[c][byte]
    (infer.normalise_lut) then bilinear(align_corners=True) to `size`, in one kernel."""
    _chk_cuda(img_u8_hwc, lut)
    if img_u8_hwc.dim() != 3 or img_u8_hwc.shape[2] != 3:
        raise _lib.HipError("infer_input: expected an (h, w, 3) image")
    if tuple(lut.shape) != (3, 256):
        raise _lib.HipError("infer_input: expected a (3, 256) table")
    img = _u8c(img_u8_hwc, "infer_input")
    h, w = img.shape[:2]
    H, W = int(size[0]), int(size[1])
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=img.device, memory_format=torch.channels_last)
    call("u2pl_infer_input_u8_f32", img, h, w, _f32c(lut).contiguous(), out, H, W)
    return out


# --------------------------------------------------------------------------- pseudo label
def pseudo_label(logits_large):
    """softmax + max over classes (train_semi.py:323-324) -> (conf, label int64)."""
    _chk_cuda(logits_large)
    x = _f32c(logits_large).contiguous()
    N, C, H, W = x.shape
    conf = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    label = torch.empty((N, H, W), dtype=torch.int64, device=x.device)
    call("u2pl_pseudo_label_f32", x, N, C, H, W, conf, label)
    return conf, label


REPLAY = None   # when a dict: the last arguments of the HBM-bound group's stages (bench.py roofline replay)


def h2d(t, device):
    """small host table -> device through a PINNED staging buffer: a pageable `.to(device)` makes the host wait
    until the stream has drained (measured 17 ms per copy mid-step), a pinned one is a true async copy."""
    if torch.device(device).type != "cuda":   # host-logic tests run the collectives on CPU tensors
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


# --------------------------------------------------------------------------- selection
def new_select_ws(device, n_total):
    words = query("u2pl_select_workspace_bytes") // 4
    ws = torch.zeros(words, dtype=torch.int32, device=device)
    ws[1:2].fill_(int(n_total))   # device-side fill: `ws[1] = n` is a pageable H2D copy that stalls the host
    ws._hist0 = False   # set by producers that accumulate the pass-0 histogram themselves
    return ws


def percentile_q32(q):
    """numpy: q = np.true_divide(q, float32(100)) with a python-float q (weak scalar)."""
    return np.float32(q) / np.float32(100)


def run_select(values, ws, specs):
    """specs: list of ('pct', q) | ('kth', k, floor_thr).  Thresholds land in
    ws[SEL_WORD_THR + j] (float bits); returns a float32 view of them."""
    n = len(specs)
    kind = np.zeros(n, np.int32)
    q32 = np.zeros(n, np.float32)
    kp = np.zeros(n, np.int64)
    fp = np.zeros(n, np.float32)
    for j, s in enumerate(specs):
        if s[0] == "pct":
            q32[j] = percentile_q32(s[1])
        else:
            kind[j] = 1
            kp[j] = int(s[1])
            fp[j] = np.float32(s[2])
    dev = values.device
    # one H2D copy; the 8-byte field goes first so every array stays naturally aligned
    buf = torch.from_numpy(np.concatenate([kp.view(np.uint8), kind.view(np.uint8), q32.view(np.uint8),
                                           fp.view(np.uint8)]))
    buf = h2d(buf, dev)
    base = buf.data_ptr()
    call("u2pl_select_f32", values, values.numel(), n, base + 8 * n, base + 12 * n, base, base + 16 * n, ws,
         int(bool(getattr(ws, "_hist0", False))))
    return ws[SEL_WORD_THR:SEL_WORD_THR + n].view(torch.float32)


def entropy_map(logits_large, label, ws, ignore=255):
    """per-pixel entropy (NaN on ignored pixels); accumulates #valid into ws[0]."""
    x = _f32c(logits_large).contiguous()
    N, C, H, W = x.shape
    ent = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    call("u2pl_entropy_f32", x, label, ignore, N, C, H, W, ent, ws)
    ws._hist0 = True
    return ent


def entropy_map_up(logits_low, size, label, ws, ignore=255):
    """bilinear(align_corners=True) up-sampling fused with the entropy: never writes the
    (B,C,H,W) logits.  logits_low may be any strided (B,C,h,w) view."""
    N, C, h, w = logits_low.shape
    H, W = int(size[0]), int(size[1])
    ent = torch.empty((N, H, W), dtype=torch.float32, device=logits_low.device)
    call("u2pl_entropy_up_f32", _f32c(logits_low), *_strides_nchw(logits_low), N, C, h, w, H, W, label, ignore, ent, ws)
    ws._hist0 = True
    return ent


def reliability_apply(entropy, thr3, label_l, label_u_aug, out_hw, negative_high_entropy=True, ignore=255,
                      num_classes=None):
    """fused: unsup target (label_u_aug with entropy >= thr3[0] -> 255), low/high masks
    (thr3[1], thr3[2]) at out_hw and the Q0 class bits; returns (target_u, nkept, low, high, lbits).
    num_classes > 32: lbits are word planes (W, 2B, h, w).  WARNING: num_classes=None means AT MOST 32 CLASSES -- one
    32-bit word per pixel; a label >= 32 would then alias onto a lower bit.  Pass num_classes whenever the labels can reach
    32 or more (reliability_split always does)."""
    B, H, W = label_u_aug.shape
    h, w = out_hw
    dev = entropy.device
    target = torch.empty_like(label_u_aug)
    nk = torch.zeros(1, dtype=torch.int32, device=dev)
    low = torch.empty((2 * B, 1, h, w), dtype=torch.float32, device=dev)
    high = torch.empty((2 * B, 1, h, w), dtype=torch.float32, device=dev)
    lbits, sfx, nc = _class_bits(num_classes, (2 * B, h, w), dev)
    call("u2pl_reliability_apply" + sfx, entropy, thr3, label_l.contiguous(), label_u_aug.contiguous(), ignore, B, H, W, h, w,
         int(bool(negative_high_entropy)), *nc, target, nk, low, high, lbits)
    return target, nk, low, high, lbits


_RF_WS = {}


def _rf_workspace(device, n_px):
    """persistent (zeroed once, self re-arming) workspace + candidate scratch of the fused split, one per stream"""
    import torch.cuda as tc
    key = (str(device), tc.current_stream().cuda_stream)
    ent = _RF_WS.get(key)
    if ent is None or ent[4] < n_px:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        G = 256
        while G > cus:
            G //= 2
        ws = torch.zeros(query("u2pl_reliability_fused_workspace_bytes", G) // 4, dtype=torch.int32, device=device)
        cand = torch.empty(query("u2pl_reliability_fused_cand_floats", n_px, G), dtype=torch.float32, device=device)
        ent = _RF_WS[key] = [G, ws, cand, 0, n_px]
    return ent


RF_FLAGS = int(os.environ.get("U2PL_RF_FENCES", "0")) & 1     # bit 0: fence pair around the split's barrier (csrc/relfused.hip)


SPLIT_FALLBACKS = {"ledger": 0}     # persistent split skipped because the side-work ledger was not empty at launch


def split_route_stats():
    """(launches, launches that needed the second device-wide barrier) of the persistent split on every workspace of this
    process (device-to-host read: call it outside the timed region)"""
    tot = big = 0
    for slot in _RF_WS.values():
        w = slot[1][4:6].cpu()
        tot, big = tot + int(w[0]), big + int(w[1])
    return tot, big


def reliability_split(logits_low, size, label_l, label_u_aug, out_hw, percents, negative_high_entropy=True, ignore=255,
                      fused=None):
    """train_semi.py:371-465 + loss_helper.py:35-44 for the unlabeled half: entropy of the bilinearly up-sampled
    teacher logits, np.percentile thresholds at `percents` ([drop] or [drop, alpha_t, 100 - alpha_t]), unsup target,
    low / high masks and class bits.  One persistent launch (csrc/relfused.hip) when the shape allows, otherwise
    entropy_up + select + apply.  -> dict(entropy, thr (float32 view, valid until the next call), target_u,
    low_mask, high_mask, lbits)."""
    import os
    B, C, h, w = logits_low.shape
    H, W = int(size[0]), int(size[1])
    hm, wm = int(out_hw[0]), int(out_hw[1])
    dev = logits_low.device
    nspec = len(percents)
    if fused is None:
        # the persistent kernel owns the GPU for its two device-wide barriers: not when several ranks share one device
        fused = (os.environ.get("U2PL_NO_FUSED_SPLIT") is None and not _SPLIT_WATCH["disabled"]
                 and int(os.environ.get("LOCAL_WORLD_SIZE", "1")) <= torch.cuda.device_count())
    if _SPLIT_WATCH["pending"]:
        poll_split()
    ok = (fused and C in (19, 21) and nspec in (1, 3) and h >= 2 and w >= 2 and H - 1 == 4 * (h - 1) and W - 1 == 4 * (w - 1)
          and H <= 1024 and W <= 1024 and hm <= H and wm <= W and 0 <= ignore <= 255)
    if ok:
        slot = _rf_workspace(dev, B * H * W)
        G, ws, cand = slot[0], slot[1], slot[2]
        per = -(-(B * h * w) // G)
        ok = G >= 128 and per // 256 + (1 if per % 256 > 64 else 0) <= 2
    if not ok:
        ws = new_select_ws(dev, B * H * W)
        ent = entropy_map_up(logits_low, (H, W), label_u_aug, ws, ignore)
        thr = run_select(ent, ws, [("pct", float(p)) for p in percents])
        if nspec == 3:
            target, _, low, high, lbits = reliability_apply(ent, thr, label_l, label_u_aug, (hm, wm),
                                                            negative_high_entropy=negative_high_entropy, ignore=ignore,
                                                            num_classes=C)
        else:
            target = label_u_aug.clone()
            drop_high_entropy_(target, ent, thr[0:1], ignore)
            low = high = lbits = None
        return dict(entropy=ent, thr=thr, target_u=target, low_mask=low, high_mask=high, lbits=lbits)
    _chk_cuda(logits_low, label_l, label_u_aug)
    if _lib.SIDE_WORK:
        # the device-wide barrier needs all G blocks resident: every side stream of this process must have been joined
        # (stream order then guarantees that none of its kernels can still occupy a CU when this one starts).  A ledger entry
        # that is still here (e.g. left behind by an exception the caller caught between add and discard) is not fatal: the
        # five-launch path has no such requirement and gives the same thresholds / masks.  NOT silent: counted
        # (bench.py reports split_ledger_fallbacks) and warned about once -- a missing side-stream join would otherwise be an
        # invisible slowdown of every later step
        SPLIT_FALLBACKS["ledger"] += 1
        if SPLIT_FALLBACKS["ledger"] == 1:
            import warnings
            warnings.warn("u2pl_amd: reliability_split found un-joined side-stream work %s and took the multi-launch path"
                          % sorted(_lib.SIDE_WORK), RuntimeWarning)
        return reliability_split(logits_low, size, label_l, label_u_aug, out_hw, percents,
                                 negative_high_entropy=negative_high_entropy, ignore=ignore, fused=False)
    q32 = np.array([percentile_q32(p) for p in percents], dtype=np.float32)
    ent = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    target = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    low = high = lbits = None
    if nspec == 3:
        low = torch.empty((2 * B, 1, hm, wm), dtype=torch.float32, device=dev)
        high = torch.empty((2 * B, 1, hm, wm), dtype=torch.float32, device=dev)
        lbits = torch.empty((2 * B, hm, wm), dtype=torch.int32, device=dev)
    call("u2pl_reliability_fused", _f32c(logits_low), *_strides_nchw(logits_low), B, C, h, w, H, W, label_u_aug.contiguous(),
         label_l.contiguous(), int(ignore), nspec, q32.ctypes.data, int(bool(negative_high_entropy)), hm, wm, ent, target,
         low, high, lbits, ws, cand, G, slot[3] & 0x3FFFFFF, RF_FLAGS)
    slot[3] += 1
    return dict(entropy=ent, thr=ws[16:16 + nspec].view(torch.float32), target_u=target, low_mask=low, high_mask=high,
                lbits=lbits, nkept=ws[2:3], err=ws[3:4])


_SPLIT_WATCH = {"pending": [], "disabled": False}


def _split_failed(rs):
    """a device-wide barrier of the persistent split timed out: its outputs are undefined AND the grow-only barrier
    counters of the reused workspace are inconsistent (later launches could pass barriers early).  Drop every cached
    workspace (a fresh zeroed one is built on the next call), route this process to the multi-launch path from now on,
    and fail the step loudly."""
    _RF_WS.clear()
    _SPLIT_WATCH["disabled"] = True
    _SPLIT_WATCH["pending"] = []
    raise _lib.HipError("u2pl_reliability_fused: device-wide barrier timed out (GPU shared with another workload?): the "
                        "results of that step are undefined.  Later calls in this process use the multi-launch path "
                        "(same as U2PL_NO_FUSED_SPLIT=1).")


def check_split(rs):
    """the persistent split kernel gives up (error word set, results undefined) when its blocks could not all become
    resident within ~0.5 s -- e.g. another process occupying the GPU.  Blocking read: call it where the step
    synchronises with the host anyway (the contrastive branch); otherwise use watch_split()."""
    err = rs.get("err") if isinstance(rs, dict) else None
    if err is not None and int(err) != 0:
        _split_failed(rs)


def defer_check_split(rs):
    """check_split() for a step whose blocking read has been deferred (defer_host_read): the error word is copied to
    pinned memory behind the kernel now and examined when the deferred reads are settled -- a direct read then would
    wait for everything enqueued since"""
    err = rs.get("err") if isinstance(rs, dict) else None
    if err is None:
        return
    ring = _SPLIT_WATCH.get("deferred")
    if ring is None:
        ring = _SPLIT_WATCH["deferred"] = {"slots": [(torch.empty(1, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                                                     for _ in range(2)], "next": 0}
    host, ev = ring["slots"][ring["next"]]
    ring["next"] = (ring["next"] + 1) % len(ring["slots"])
    host.copy_(err, non_blocking=True)
    ev.record()

    def examine():
        ev.synchronize()
        if int(host[0]) != 0:
            _split_failed(rs)
    defer_host_read(examine)


def watch_split(rs):
    """check_split() for steps WITHOUT a host synchronisation (configs without trainer.contrastive are valid upstream):
    the error word is copied to pinned host memory behind the kernel (no stall) and examined by poll_split() at the
    next call / next step, when the copy has long completed."""
    err = rs.get("err") if isinstance(rs, dict) else None
    if err is None:
        return
    # a small ring of pre-pinned slots and events (a fresh pin_memory() per step is a hipHostMalloc: tens of us and, on some
    # ROCm versions, an implicit synchronisation -- the opposite of "no stall"); poll_split() keeps at most two copies
    # outstanding, so a slot that comes round again has long been read
    ring = _SPLIT_WATCH.get("ring")
    if ring is None:
        ring = _SPLIT_WATCH["ring"] = {"slots": [(torch.empty(1, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                                                 for _ in range(4)], "next": 0}
    host, ev = ring["slots"][ring["next"]]
    ring["next"] = (ring["next"] + 1) % len(ring["slots"])
    if any(h is host for h, _ in _SPLIT_WATCH["pending"]):      # (cannot happen with <= 2 outstanding; never overwrite an unread slot)
        poll_split(block=True)
    host.copy_(err, non_blocking=True)
    ev.record()
    _SPLIT_WATCH["pending"].append((host, ev))
    poll_split()


def poll_split(block=False):
    """examine the error words whose copies have completed (all of them when block=True; the oldest one is waited for
    once more than two steps are outstanding, so a failure is reported at most two steps late)"""
    pend = _SPLIT_WATCH["pending"]
    while pend:
        host, ev = pend[0]
        if not (block or len(pend) > 2 or ev.query()):
            break
        ev.synchronize()
        pend.pop(0)
        if int(host[0]) != 0:
            _split_failed(None)


# --------------------------------------------------------------------------- cross entropy
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore, unsup_weight, gmul, class_weight=None):
        _chk_cuda(logits, target)
        x = _f32c(logits).contiguous()
        N, C, H, W = x.shape
        work = torch.empty(query("u2pl_ce_workspace_bytes"), dtype=torch.uint8, device=x.device)
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        if class_weight is not None:
            call("u2pl_ce_fwd_weighted_f32", x, target, ignore, N, C, H, W, class_weight, work, out3)
        else:
            call("u2pl_ce_fwd_f32", x, target, ignore, N, C, H, W, int(unsup_weight), work, out3)
        ctx.save_for_backward(x, target, out3, class_weight)
        ctx.ignore, ctx.gmul = ignore, gmul
        return out3[0].clone() * gmul if gmul != 1.0 else out3[0].clone()

    @staticmethod
    def backward(ctx, g):
        x, target, out3, cw = ctx.saved_tensors
        N, C, H, W = x.shape
        grad = torch.empty_like(x)
        if cw is not None:
            call("u2pl_ce_bwd_weighted_f32", x, target, ctx.ignore, N, C, H, W, cw, out3, g.contiguous(), float(ctx.gmul), grad)
        else:
            call("u2pl_ce_bwd_f32", x, target, ctx.ignore, N, C, H, W, out3, g.contiguous(), float(ctx.gmul), grad)
        return grad, None, None, None, None, None


def cross_entropy(logits, target, ignore_index=255, unsup_weight=False, scale=1.0, class_weight=None):
    """F.cross_entropy(logits, target, ignore_index[, weight=class_weight]) [* B*H*W/n_valid if unsup_weight] * scale."""
    if target.dtype != torch.int64 or not target.is_contiguous():
        target = target.long().contiguous()
    if class_weight is not None:
        if unsup_weight or class_weight.numel() != logits.shape[1]:
            raise _lib.HipError("class_weight needs one weight per class and excludes unsup_weight")
        class_weight = class_weight.to(device=logits.device, dtype=torch.float32).contiguous()
    return _CrossEntropy.apply(logits, target, int(ignore_index), bool(unsup_weight), float(scale), class_weight)


# --------------------------------------------------------------------------- Lovasz-Softmax (csrc/lovasz.hip)
LOVASZ_CLASSES = ("present", "all")
LOVASZ_PLAN_FIELDS = ("chunks", "cap", "tile", "tiles", "err_blocks", "count_blocks", "passes", "grid_x", "sort_scan_blocks",
                      "grad_scan_blocks", "keys", "vals", "keys_alt", "vals_alt", "sort_ws", "tilefg", "part", "counts", "slabs",
                      "total")


def lovasz_plan(P, C, class_chunk=None):
    """u2pl_lovasz_plan as a dict (host arithmetic only, no GPU): chunk count, tiles and grids per stage, workspace offsets"""
    import ctypes
    chunk = int(query("u2pl_lovasz_default_chunk") if class_chunk is None else class_chunk)
    out = (ctypes.c_longlong * len(LOVASZ_PLAN_FIELDS))()
    rc = query("u2pl_lovasz_plan", int(P), int(C), chunk, out)
    if rc != 0:
        raise _lib.HipError(f"u2pl_lovasz_plan({P}, {C}, {chunk}) failed with code {rc}")
    return dict(zip(LOVASZ_PLAN_FIELDS, (int(v) for v in out)), class_chunk=chunk)


class _LovaszSoftmax(torch.autograd.Function):
    """owns the workspace and the [C][P] plane of Lovasz gradients; fixed sizes, no host read: capturable by graphs.py"""

    @staticmethod
    def forward(ctx, logits, target, ignore, present_only, gmul, class_chunk):
        _chk_cuda(logits, target)
        x = _f32c(logits).contiguous()
        N, C, H, W = x.shape
        P = N * H * W
        plan = lovasz_plan(P, C, class_chunk)
        chunk = plan["class_chunk"]
        work = torch.empty(plan["total"], dtype=torch.uint8, device=x.device)
        gplane = torch.empty((C, P), dtype=torch.float32, device=x.device)
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        for c0 in range(0, C, plan["cap"]):
            call("u2pl_lovasz_errors_f32", x, target, ignore, N, C, H, W, c0, work, chunk)
            call("u2pl_lovasz_sort", P, C, c0, work, chunk)
            call("u2pl_lovasz_grad_f32", P, C, c0, int(present_only), work, chunk, gplane)
        call("u2pl_lovasz_finish_f32", P, C, int(present_only), work, chunk, out3)
        ctx.save_for_backward(x, target, out3, gplane)
        ctx.ignore, ctx.gmul = ignore, gmul
        return out3[0].clone() * gmul if gmul != 1.0 else out3[0].clone()

    @staticmethod
    def backward(ctx, g):
        x, target, out3, gplane = ctx.saved_tensors
        N, C, H, W = x.shape
        grad = torch.empty_like(x)
        call("u2pl_lovasz_bwd_f32", x, target, ctx.ignore, N, C, H, W, gplane, out3, g.contiguous(), float(ctx.gmul), grad)
        return grad, None, None, None, None, None


def lovasz_softmax(logits, target, ignore_index=255, classes="present", scale=1.0, per_image=False, class_chunk=None):
    """Lovasz-Softmax loss of the flattened batch (Berman et al. 2018) * scale; classes: "present" (classes with a labelled
    pixel; 0 when there are none) or "all".  No per-image mode, no class list, no class weights.
    class_chunk: classes sorted at a time (default u2pl_lovasz_default_chunk() = 32); bounds the workspace, not the result."""
    if per_image:
        raise ValueError("lovasz_softmax: per_image=True is not supported (the batch is flattened)")
    if not isinstance(classes, str) or classes not in LOVASZ_CLASSES:
        raise ValueError(f"lovasz_softmax: classes must be 'present' or 'all', got {classes!r} (class lists are not supported)")
    if logits.dim() != 4 or not 2 <= logits.shape[1] <= WIDE_MAXC:
        raise ValueError(f"lovasz_softmax: logits [N, C, H, W] with 2 <= C <= {WIDE_MAXC} expected, got {tuple(logits.shape)}")
    if class_chunk is not None and int(class_chunk) < 1:
        raise ValueError(f"lovasz_softmax: class_chunk = {class_chunk}: expected a positive chunk size")
    if target.dtype != torch.int64 or not target.is_contiguous():
        target = target.long().contiguous()
    return _LovaszSoftmax.apply(logits, target, int(ignore_index), classes == "present", float(scale),
                                None if class_chunk is None else int(class_chunk))


def ohem_kept_target(pred, target, thresh, min_kept, ignore_index=255):
    """OhemCrossEntropy2dTensor target rewrite (loss_helper.py:502-529), no host sync."""
    x = _f32c(pred.detach()).contiguous()
    N, C, H, W = x.shape
    target = target.long().contiguous()
    ws = new_select_ws(x.device, N * H * W)
    mp = torch.empty((N, H, W), dtype=torch.float32, device=x.device)
    call("u2pl_ohem_prob_f32", x, target, ignore_index, N, C, H, W, mp, ws)
    ws._hist0 = True
    thr = run_select(mp, ws, [("kth", int(min_kept), float(thresh))])
    kept = torch.empty_like(target)
    call("u2pl_ohem_apply_i64", mp, thr, target, ignore_index, target.numel(), kept)
    return kept


# --------------------------------------------------------------------------- reliability split
def drop_high_entropy_(target, entropy, thr_bits, ignore=255):
    """target[entropy >= thr] = ignore, in place (loss_helper.py:41-43)."""
    nk = torch.zeros(1, dtype=torch.int32, device=target.device)
    call("u2pl_apply_drop_i64", entropy, thr_bits, target, ignore, target.numel(), nk)
    return nk


def reliability_masks(entropy, thr_lo, thr_hi, label_l, label_u_aug, out_hw, negative_high_entropy=True,
                      ignore=255, num_classes=None):
    """train_semi.py:408-465 -> low_mask_all, high_mask_all (2B,1,h,w) float and
    the (quirky) multi-hot labels as class bitmasks (2B,h,w) int32; num_classes > 32: word planes (W,2B,h,w).
    WARNING: num_classes=None means AT MOST 32 CLASSES (one word per pixel; a label >= 32 would alias onto a lower bit):
    pass num_classes whenever the labels can reach 32 or more."""
    B, H, W = label_u_aug.shape
    h, w = out_hw
    dev = entropy.device
    low = torch.empty((2 * B, 1, h, w), dtype=torch.float32, device=dev)
    high = torch.empty((2 * B, 1, h, w), dtype=torch.float32, device=dev)
    lbits, sfx, nc = _class_bits(num_classes, (2 * B, h, w), dev)
    call("u2pl_reliability_masks" + sfx, entropy, thr_lo, thr_hi, label_l.contiguous(), label_u_aug.contiguous(),
         ignore, B, H, W, h, w, int(bool(negative_high_entropy)), *nc, low, high, lbits)
    return low, high, lbits


def pack_class_bits(onehot, wide=None):
    """(N,C,h,w) multi-hot -> class bits (N,h,w) int32; C > 32 (or wide=True, for tests): word planes (W,N,h,w)"""
    N, C, h, w = onehot.shape
    bits, sfx, _ = _class_bits(C, (N, h, w), onehot.device, wide)
    call("u2pl_pack_class_bits" + sfx, onehot.long().contiguous(), N, C, h, w, bits)
    return bits


def unpack_class_bits(bits, C):
    if bits.dim() == 4:      # word planes (W,N,h,w)
        check_num_classes(C)
        if bits.shape[0] != wide_words(C):
            raise _lib.HipError(f"unpack_class_bits: {C} classes are {wide_words(C)} planes, got {bits.shape[0]}")
        _, N, h, w = bits.shape
        oh = torch.empty((N, C, h, w), dtype=torch.int64, device=bits.device)
        call("u2pl_unpack_class_bits_wide", bits.contiguous(), N, C, h, w, oh)
        return oh
    N, h, w = bits.shape
    oh = torch.empty((N, C, h, w), dtype=torch.int64, device=bits.device)
    call("u2pl_unpack_class_bits", bits, N, C, h, w, oh)
    return oh


# --------------------------------------------------------------------------- deferred host read
# With the contrastive sampling planned on the device (sampling_plan) the step's one device-to-host read -- the list
# lengths -- is no longer needed to ENQUEUE the step; it is taken at the end of train_step.  Until then the host copies
# that depend on it are stale: the memory bank's length / head / ptr, LAST_STATS and the global CPU generator (not yet
# advanced by the draws).  Whoever reads one of them calls settle_host_reads() first; it is a no-op when nothing is pending.
_SETTLE = []


def defer_host_read(fn):
    """fn runs at the next settle_host_reads(), after those deferred before it"""
    _SETTLE.append(fn)


def host_read_pending():
    return bool(_SETTLE)


def settle_host_reads():
    while _SETTLE:
        fns = list(_SETTLE)
        del _SETTLE[:]       # (cleared first: what fn reads -- the bank's bookkeeping -- settles too)
        for fn in fns:
            fn()


def _settled(name):
    def get(self):
        settle_host_reads()
        return getattr(self, name)

    def put(self, value):
        settle_host_reads()
        setattr(self, name, value)
    return property(get, put)


# --------------------------------------------------------------------------- memory bank
class DeviceMemoryBank:
    """Per-class FIFO of negative keys resident in HBM (replaces the reference's
    list of CPU tensors, train_semi.py:161-169 / utils.py:27-47).  Logical row j
    of class c lives at physical slot (head[c] + j) % cap[c]."""

    # host bookkeeping: reading it settles a deferred read of the list lengths first (settle_host_reads)
    head, length, ptr = _settled("_head"), _settled("_length"), _settled("_ptr")

    def __init__(self, num_classes, queue_size, feat_dim=256, device="cuda"):
        check_num_classes(num_classes, "DeviceMemoryBank: num_classes")
        self.C, self.D = num_classes, feat_dim
        self.cap = [int(q) for q in queue_size]
        # ONE storage buffer, the class rings are row ranges of it (u2pl_bank_* address it through the device state)
        self.storage = torch.zeros((sum(self.cap), feat_dim), dtype=torch.float32, device=device)
        offs = np.concatenate([[0], np.cumsum(self.cap)]).astype(np.int64)
        self.buf = [self.storage[int(offs[c]):int(offs[c + 1])] for c in range(num_classes)]
        self.head = [0] * num_classes
        self.length = [0] * num_classes
        self.ptr = [0] * num_classes  # reference's queue_ptr bookkeeping (utils.py:36-45)
        # device copy of the bookkeeping (int64 [C][5]: ring offset, cap, head, len, ptr) for u2pl_bank_enqueue_f32; the host
        # lists above mirror it (the reference draws torch.randint(len) on the CPU).  Host-driven appends mark it stale.
        self._offs = offs
        self.state = None
        self._state_stale = True

    def _sync_state(self):
        """upload the host bookkeeping when a host-driven append / load changed it"""
        if self.storage.device.type != "cuda":
            return False
        if self.state is None:
            self.state = torch.zeros((self.C, 5), dtype=torch.int64, device=self.storage.device)
        if self._state_stale:
            st = np.stack([self._offs[:-1], np.array(self.cap), np.array(self.head), np.array(self.length), np.array(self.ptr)], 1)
            self.state.copy_(h2d(torch.from_numpy(st.astype(np.int64)), self.storage.device))
            self._state_stale = False
        return True

    def enqueue_device(self, rows, ld, idx, idx_stride, counts_dev, list_off=None):
        """dequeue_and_enqueue for every class in ONE call with the list lengths still on the DEVICE (counts_dev: uint32
        [C]): can be issued before the step's host synchronisation.  Follow with mirror_counts() once the counts are on
        the host.  list_off (int64 [C] on the device): idx is a flat list buffer and class c's list starts at
        list_off[c] (the wide route; any C up to 255)."""
        self._sync_state()
        wide = list_off is not None or self.C > MAXC
        if wide and list_off is None:
            raise _lib.HipError("enqueue_device: more than 32 classes need the flat list layout (list_off)")
        call("u2pl_bank_enqueue_wide_f32" if wide else "u2pl_bank_enqueue_f32", self.state, self.storage, self.D, rows, ld, idx,
             list_off if wide else idx_stride, None, counts_dev, self.C)
        if REPLAY is not None and not wide:
            REPLAY["enqueue"] = (rows, ld, idx, idx_stride, counts_dev)
            REPLAY["bank"] = self

    def mirror_counts(self, counts):
        """the host copy of what u2pl_bank_enqueue_f32 did to the bookkeeping (same arithmetic, utils.py:36-45)"""
        for c in range(self.C):
            n_new = int(counts[c])
            cap = self.cap[c]
            tail = (self.head[c] + self.length[c]) % cap
            self.length[c] = min(self.length[c] + n_new, cap)
            self.head[c] = ((tail + n_new) % cap - self.length[c]) % cap
            self._book(c, n_new)

    def append_rows(self, c, rows, ld, n_new, idx_list=None):
        """append n_new rows (rows base pointer/tensor, leading dim ld, optional int32 index list)."""
        if n_new <= 0:
            self._book(c, 0)
            return
        cap = self.cap[c]
        tail = (self.head[c] + self.length[c]) % cap
        call("u2pl_bank_append_f32", self.buf[c], cap, tail, self.D, rows, ld, idx_list, n_new)
        self._state_stale = True
        tot = self.length[c] + n_new
        new_tail = (tail + n_new) % cap
        self.length[c] = min(tot, cap)
        self.head[c] = (new_tail - self.length[c]) % cap
        self._book(c, n_new)

    def append_multi(self, entries, ld):
        """entries: [(class, rows tensor/ptr, n_new, int32 index list or None)] in FIFO order -> ONE launch.
        Several entries may target the same class (rank-major blocks of an all-gather): each starts at the
        tail left by the previous one."""
        head, length = list(self.head), list(self.length)
        per_class = {}
        for c, _, n_new, _ in entries:
            per_class[c] = per_class.get(c, 0) + n_new
        if any(n > self.cap[c] for c, n in per_class.items()) and len(entries) > len(per_class):
            for c, rows, n_new, idx_list in entries:   # wrap-around inside one launch would race: go sequentially
                self.append_rows(c, rows, ld, n_new, idx_list)
            return
        desc = np.zeros((max(len(entries), 1), 6), dtype=np.int64)
        mx = 0
        for k, (c, rows, n_new, idx_list) in enumerate(entries):
            cap = self.cap[c]
            tail = (head[c] + length[c]) % cap
            desc[k] = (self.buf[c].data_ptr(), cap, tail, _lib._ptr(rows) or 0,
                       idx_list.data_ptr() if idx_list is not None else 0, n_new)
            mx = max(mx, min(n_new, cap))
            if n_new > 0:
                length[c] = min(length[c] + n_new, cap)
                head[c] = ((tail + n_new) % cap - length[c]) % cap
        if mx > 0:
            dd = h2d(torch.from_numpy(desc), self.buf[0].device)
            call("u2pl_bank_append_multi_f32", dd, len(entries), self.D, ld, mx)
            if REPLAY is not None:
                REPLAY["append"] = (dd, len(entries), self.D, ld, mx, [e[1] for e in entries], [e[3] for e in entries])
        self.head, self.length = head, length
        self._state_stale = True
        for c, n in per_class.items():
            self._book(c, n)

    def _book(self, c, bs):
        if self.length[c] >= self.cap[c]:
            self.ptr[c] = self.cap[c]
        else:
            self.ptr[c] = (self.ptr[c] + bs) % self.cap[c]

    def logical(self, c):
        n, h, cap = self.length[c], self.head[c], self.cap[c]
        if h + n <= cap:
            return self.buf[c][h:h + n]
        return torch.cat((self.buf[c][h:], self.buf[c][: (h + n) % cap]))

    def load_logical(self, c, rows):
        n = min(rows.shape[0], self.cap[c])
        self.buf[c][:n].copy_(rows[-n:])
        self.head[c], self.length[c] = 0, n
        self._state_stale = True

    def __len__(self):
        return self.C

    def __getitem__(self, c):  # memobank[c][0] compatibility
        return [self.logical(c)]


# --------------------------------------------------------------------------- contrastive core
class ContraPhase1:
    """Outputs of phase 1 (loss_helper.py:80-154) living on the device.
    Narrow route (C <= 32): idx int32 (3, 32, P), counts (3, 32).  Wide route: counts (3, C), offsets int64 (3, C) and,
    once finish() has run with the counts on the host, idx = ONE flat int32 buffer with the lists back to back in
    (kind, class) order.  list() / list_ptr() / lists() address a list the same way on both."""
    __slots__ = ("idx", "counts", "proto", "cap", "counts_host", "wide", "C", "offsets", "offsets_host", "bits", "_fin")

    def list_ptr(self, kind, c):
        """device address of the first element of list (kind, c)"""
        if self.wide:
            return self.idx.data_ptr() + int(self.offsets_host[kind][c]) * 4
        return self.idx.data_ptr() + (kind * MAXC + c) * self.cap * 4

    def list(self, kind, c):
        """the pixel list (kind, c) as an int32 view (needs counts_host)"""
        n = int(self.counts_host[kind][c])
        if self.wide:
            o = int(self.offsets_host[kind][c])
            return self.idx[o:o + n]
        return self.idx[kind, c, :n]

    def lists(self, kind):
        """what enqueue_all_classes indexes by class: the narrow (32, P) plane, or the wide route's per-class views"""
        if self.wide:
            return [self.list(kind, c) for c in range(self.C)]
        return self.idx[kind]

    def finish(self, counts_host):
        """wide route: with the list lengths on the host, size the flat list buffer, write the lists and the prototypes
        (the narrow route did all of it in contra_phase1)"""
        self.counts_host = counts_host
        if not self.wide or self._fin is None:
            return
        rows, ld, D, P, work = self._fin
        self._fin = None
        cnt = np.asarray(counts_host, dtype=np.int64)[:, :self.C]
        self.offsets_host = wide_list_offsets(cnt)
        total = int(cnt.sum())
        self.idx = torch.empty(max(total, 1), dtype=torch.int32, device=self.counts.device)
        abits, lowbits, nbits = self.bits
        call("u2pl_compact_lists_wide", abits, lowbits, nbits, P, self.C, work, self.offsets, self.idx, total)
        call("u2pl_class_prototypes_wide", rows, ld, D, self.idx, self.offsets, self.counts, self.C, self.proto)


def wide_list_offsets(counts):
    """counts [3][C] -> first element of every list in the flat buffer (lists back to back in (kind, class) order): the
    host's copy of what u2pl_contra_classify_wide writes to `offsets`"""
    cnt = np.asarray(counts, dtype=np.int64)
    flat = cnt.reshape(-1)
    return (np.cumsum(flat) - flat).reshape(cnt.shape)


def _contra_phase1_wide(rep_teacher_rows, ld, D, prob, prob_strides, lbits, low_mask, high_mask, num_labeled, C, h, w, cfg):
    """the wide route up to the list lengths: classify into word planes, scan, offsets.  ContraPhase1.finish() writes
    the lists and the prototypes once the lengths are on the host."""
    check_num_classes(C)
    dev = lbits.device
    W = wide_words(C)
    if lbits.dim() == 3:     # one 32-bit word per pixel (C <= 32 forced onto this route): it is plane 0
        lbits = lbits.unsqueeze(0)
    if lbits.shape[0] != W:
        raise _lib.HipError(f"contra_phase1: {C} classes need {W} planes of class bits, got {lbits.shape[0]}")
    lbits = lbits.contiguous()
    N2 = lbits.shape[1]
    P = N2 * h * w
    bits = torch.empty((3, W, P), dtype=torch.int32, device=dev)
    out = ContraPhase1()
    out.wide, out.C, out.cap = True, C, P
    out.counts = torch.empty((3, C), dtype=torch.int32, device=dev)
    out.offsets = torch.empty((3, C), dtype=torch.int64, device=dev)
    out.proto = torch.empty((C, D), dtype=torch.float32, device=dev)
    out.idx = out.offsets_host = out.counts_host = None
    work = torch.empty(query("u2pl_contra_wide_workspace_bytes", P, C), dtype=torch.uint8, device=dev)
    call("u2pl_contra_classify_wide", prob, *prob_strides, lbits, low_mask, high_mask, N2, num_labeled, C, h, w,
         float(cfg["current_class_threshold"]), float(cfg["current_class_negative_threshold"]), int(cfg["low_rank"]),
         int(cfg["high_rank"]), bits[0], bits[1], bits[2], work, out.counts, out.offsets)
    out.bits = (bits[0], bits[1], bits[2])
    out._fin = (rep_teacher_rows, ld, D, P, work)
    return out


def contra_phase1(rep_teacher_rows, ld, D, prob, prob_strides, lbits, low_mask, high_mask, num_labeled, C, h, w,
                  cfg, wide=None):
    """classify + compaction + prototypes.  prob_strides = (sn, sc, sp).
    C > 32 takes the wide route (csrc/contrast_wide.hip): the lists and prototypes are written by the returned object's
    finish(counts_host).  wide=True forces that route at C <= 32 -- for tests that compare the two; not a tuning knob."""
    if C > MAXC if wide is None else wide:
        return _contra_phase1_wide(rep_teacher_rows, ld, D, prob, prob_strides, lbits, low_mask, high_mask, num_labeled, C,
                                   h, w, cfg)
    if REPLAY is not None:
        REPLAY["phase1"] = (rep_teacher_rows, ld, D, prob, prob_strides, lbits, low_mask, high_mask, num_labeled, C, h, w, cfg)
    dev = lbits.device
    N2 = lbits.shape[0]
    P = N2 * h * w
    abits = torch.empty(P, dtype=torch.int32, device=dev)
    lowbits = torch.empty(P, dtype=torch.int32, device=dev)
    nbits = torch.empty(P, dtype=torch.int32, device=dev)
    out = ContraPhase1()
    out.cap = P
    out.wide, out.C, out.offsets, out.offsets_host, out.bits, out._fin = False, C, None, None, (abits, lowbits, nbits), None
    out.idx = torch.empty((3, MAXC, P), dtype=torch.int32, device=dev)
    out.counts = torch.empty((3, MAXC), dtype=torch.int32, device=dev)
    out.proto = torch.empty((C, D), dtype=torch.float32, device=dev)
    args = (float(cfg["current_class_threshold"]), float(cfg["current_class_negative_threshold"]), int(cfg["low_rank"]),
            int(cfg["high_rank"]))
    if PHASE1_FUSED and C in (19, 21, 32) and D % 4 == 0 and D <= 256:
        # three launches: classify, prototype streaming, merged tail (compaction write + list lengths || prototype finish)
        work = torch.empty(query("u2pl_contra_phase1_workspace_bytes", P, C, D), dtype=torch.uint8, device=dev)
        call("u2pl_contra_phase1", prob, *prob_strides, lbits, low_mask, high_mask, N2, num_labeled, C, h, w, *args,
             rep_teacher_rows, ld, D, abits, lowbits, nbits, out.idx, P, out.counts, out.proto, work)
    else:
        work = torch.empty(query("u2pl_compact_workspace_bytes", P), dtype=torch.uint8, device=dev)
        call("u2pl_contra_classify", prob, *prob_strides, lbits, low_mask, high_mask, N2, num_labeled, C, h, w, *args, abits,
             lowbits, nbits, work)
        call("u2pl_compact_lists", abits, lowbits, nbits, P, C, work, out.idx, P, out.counts, 1)
        pw = torch.empty(query("u2pl_proto_workspace_bytes", P, C, D), dtype=torch.uint8, device=dev)
        call("u2pl_class_prototypes", rep_teacher_rows, ld, D, out.idx, P, out.counts, C, P, pw, out.proto, lowbits)
    out.counts_host = None
    return out


PHASE1_FUSED = os.environ.get("U2PL_PHASE1_UNFUSED") is None     # False: the five-launch sequence (kept as the cross-check)
_NCE_STATE = {}


def _nce_state(device, P, D):
    """persistent buffers of the row-sparse InfoNCE gradient: an all-zero (P, D) gradient, the per-pixel chain heads
    (-1), and the pixel list whose rows the previous backward pass wrote (cleared lazily before the next write)"""
    key = (str(device), P, D)
    st = _NCE_STATE.get(key)
    if st is None:
        st = _NCE_STATE[key] = dict(grad=torch.zeros((P, D), dtype=torch.float32, device=device),
                                    head=torch.full((P,), -1, dtype=torch.int32, device=device), dirty=None, pending=None,
                                    ws=None)
    return st


NCE_FUSED = os.environ.get("U2PL_NCE_UNFUSED") is None     # loss reduce + stale-row clearing inside the InfoNCE launch


def _nce_forward(st, rep_rows, jobs_dev, njobs, Q, K, temp, valid_seg, groups, loss_q, ganchor, apix, nxt, loss):
    """the forward launches: ONE (u2pl_infonce_fused_f32: InfoNCE + loss reduction + clearing of the rows the previous
    backward wrote) when the shape allows it, else u2pl_infonce_f32 + u2pl_infonce_reduce_f32 (rows cleared in backward)"""
    P, D = rep_rows.shape
    # (the fused launch is exercised and sized for the narrow route's <= 32 jobs; more jobs take the separate entry points,
    # which are generic in njobs and reduce in the same order)
    if NCE_FUSED and Q % 4 == 0 and D <= 256 and njobs <= MAXC:
        need = query("u2pl_infonce_fused_workspace_bytes", njobs, Q)
        if st["ws"] is None or st["ws"].numel() < need:
            st["ws"] = torch.zeros(max(need, query("u2pl_infonce_fused_workspace_bytes", MAXC, Q)), dtype=torch.uint8,
                                   device=rep_rows.device)
        dirty = st["dirty"]
        call("u2pl_infonce_fused_f32", jobs_dev, njobs, rep_rows, D, D, Q, K, float(temp), loss_q, ganchor, apix, st["head"], nxt,
             groups[2], st["grad"] if dirty is not None else None, D, dirty, dirty.numel() if dirty is not None else 0,
             st["ws"], 1.0 / valid_seg, loss)
        st["dirty"] = None
    else:
        call("u2pl_infonce_f32", jobs_dev, njobs, rep_rows, D, D, Q, K, float(temp), loss_q, ganchor, apix, st["head"], nxt,
             groups[2])
        call("u2pl_infonce_reduce_f32", loss_q, njobs, Q, 1.0 / valid_seg, loss)


def _nce_rearm(st):
    """a forward pass whose backward never ran (loss evaluated without gradients) left its chain heads armed: clear them
    before new chains are built on top (rare path, plain torch)"""
    if st["pending"] is not None:
        # (entries of jobs a device-planned step did not have are -1: clamped onto pixel 0, whose head is either armed by
        # this same forward or -1 already)
        st["head"].index_fill_(0, st["pending"].reshape(-1).long().clamp_min_(0), -1)
        st["pending"] = None


def group_entries(ia_per_job, Q):
    """host-side grouping of the anchor draws (the host drew them: loss_helper.py:179-181): per job, the entries sorted
    by (candidate index, entry) and, for the first entry of every group of equal candidates, the group's position and
    length.  -> int32 [3][njobs*Q]: order, seg_pos, seg_len (0 for non-leaders)."""
    nj = len(ia_per_job)
    out = np.zeros((3, nj * Q), dtype=np.int32)
    for j, ia in enumerate(ia_per_job):
        ia = np.asarray(ia)
        o = np.argsort(ia, kind="stable")
        si = ia[o]
        starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]])
        lens = np.diff(np.r_[starts, Q])
        out[0, j * Q:(j + 1) * Q] = j * Q + o
        lead = j * Q + o[starts]
        out[1, lead] = j * Q + starts
        out[2, lead] = lens
    return out


class _InfoNCE(torch.autograd.Function):
    """rep_rows: (P, D) contiguous view of the student features (requires grad)."""

    @staticmethod
    def forward(ctx, rep_rows, jobs_dev, njobs, Q, K, temp, valid_seg, groups, keepalive):
        P, D = rep_rows.shape
        dev = rep_rows.device
        st = _nce_state(dev, P, D)
        loss_q = torch.empty((njobs, Q), dtype=torch.float32, device=dev)
        ganchor = torch.empty((njobs, Q, D), dtype=torch.float32, device=dev)
        apix = torch.empty((njobs, Q), dtype=torch.int32, device=dev)
        nxt = torch.empty((njobs, Q), dtype=torch.int32, device=dev)
        _nce_rearm(st)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _nce_forward(st, rep_rows, jobs_dev, njobs, Q, K, temp, valid_seg, groups, loss_q, ganchor, apix, nxt, loss)
        st["pending"] = apix
        ctx.save_for_backward(ganchor, apix, nxt, groups)
        ctx.meta = (P, D, njobs * Q, 1.0 / (Q * valid_seg))
        return loss

    @staticmethod
    def backward(ctx, g):
        ganchor, apix, nxt, groups = ctx.saved_tensors
        P, D, n, scale = ctx.meta
        st = _nce_state(g.device, P, D)
        if st["pending"] is not apix:
            raise _lib.HipError("InfoNCE backward must follow its own forward exactly once (the per-pixel chains are "
                                "consumed by the backward pass; retain_graph / interleaved forwards are not supported)")
        st["pending"] = None
        if st["dirty"] is not None:      # rows written by the previous step's backward (their consumer has long run)
            call("u2pl_zero_rows_f32", st["grad"], D, D, st["dirty"], st["dirty"].numel())
        call("u2pl_scatter_rows_ordered_f32", st["grad"], D, D, apix, nxt, st["head"], groups[0], groups[1], groups[2],
             ganchor, n, g.contiguous(), float(scale))
        st["dirty"] = apix
        return st["grad"], None, None, None, None, None, None, None, None


def infonce_kernels_once(rep_rows, jobs_dev, njobs, Q, K, temp, valid_seg, groups):
    """the exact launch sequence of _InfoNCE forward + backward (bench.py's roofline replay): InfoNCE (+ loss reduce + clearing
    of the previous rows in the same launch), ordered row-sparse scatter"""
    P, D = rep_rows.shape
    dev = rep_rows.device
    st = _nce_state(dev, P, D)
    loss_q = torch.empty((njobs, Q), dtype=torch.float32, device=dev)
    ganchor = torch.empty((njobs, Q, D), dtype=torch.float32, device=dev)
    apix = torch.empty((njobs, Q), dtype=torch.int32, device=dev)
    nxt = torch.empty((njobs, Q), dtype=torch.int32, device=dev)
    _nce_rearm(st)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    _nce_forward(st, rep_rows, jobs_dev, njobs, Q, K, temp, valid_seg, groups, loss_q, ganchor, apix, nxt, loss)
    if st["dirty"] is not None:
        call("u2pl_zero_rows_f32", st["grad"], D, D, st["dirty"], st["dirty"].numel())
    call("u2pl_scatter_rows_ordered_f32", st["grad"], D, D, apix, nxt, st["head"], groups[0], groups[1], groups[2], ganchor,
         njobs * Q, None, 1.0 / (Q * valid_seg))
    st["dirty"] = apix
    return loss


class _ZeroTimesSum(torch.autograd.Function):
    """`0 * rep.sum()` of the reference (loss_helper.py:160-162,187; Q13):
    a zero loss that still hands ZERO (not None) gradients to the rep head."""

    @staticmethod
    def forward(ctx, rep):
        ctx.meta = (rep.shape, None)
        return torch.zeros((), dtype=torch.float32, device=rep.device)

    @staticmethod
    def backward(ctx, g):
        shape, stride = ctx.meta
        return torch.zeros(shape, dtype=torch.float32, device=g.device)


def zero_times_sum(rep):
    return _ZeroTimesSum.apply(rep)


class _InfoNCEDev(torch.autograd.Function):
    """_InfoNCE with the job count, the valid-class count and both scales on the device (plan: the buffers of
    sampling_plan): worst-case grids, per-job buffers sized for max_jobs, no host value depends on the step's counts."""

    @staticmethod
    def forward(ctx, rep_rows, plan, Q, K, temp):
        P, D = rep_rows.shape
        dev = rep_rows.device
        mj = plan["max_jobs"]
        st = _nce_state(dev, P, D)
        loss_q = torch.empty((mj, Q), dtype=torch.float32, device=dev)
        ganchor = torch.empty((mj, Q, D), dtype=torch.float32, device=dev)
        nxt = torch.empty((mj, Q), dtype=torch.int32, device=dev)
        apix, groups = plan["apix"], plan["groups"]
        _nce_rearm(st)
        need = query("u2pl_infonce_fused_workspace_bytes", MAXC, Q)
        if st["ws"] is None or st["ws"].numel() < need:
            st["ws"] = torch.zeros(need, dtype=torch.uint8, device=dev)
        dirty = st["dirty"]
        call("u2pl_infonce_fused_dev_f32", plan["jobs"], plan["hdr"], mj, rep_rows, D, D, Q, K, float(temp), loss_q, ganchor,
             apix, st["head"], nxt, groups[2], st["grad"] if dirty is not None else None, D, dirty,
             dirty.numel() if dirty is not None else 0, st["ws"], plan["loss"])
        st["dirty"] = None
        st["pending"] = apix
        ctx.save_for_backward(ganchor, apix, nxt, groups, plan["hdr"])
        ctx.meta = (P, D, mj * Q)
        return plan["loss"]

    @staticmethod
    def backward(ctx, g):
        ganchor, apix, nxt, groups, hdr = ctx.saved_tensors
        P, D, n = ctx.meta
        st = _nce_state(g.device, P, D)
        if st["pending"] is not apix:
            raise _lib.HipError("InfoNCE backward must follow its own forward exactly once (the per-pixel chains are "
                                "consumed by the backward pass; retain_graph / interleaved forwards are not supported)")
        st["pending"] = None
        if st["dirty"] is not None:
            call("u2pl_zero_rows_f32", st["grad"], D, D, st["dirty"], st["dirty"].numel())
        call("u2pl_scatter_rows_ordered_dev_f32", st["grad"], D, D, apix, nxt, st["head"], groups[0], groups[1], groups[2],
             ganchor, n, g.contiguous(), hdr)
        st["dirty"] = apix
        return st["grad"], None, None, None, None


_PLAN_HOST = {}


def _plan_host_slot(n_words):
    """pinned staging for the raw words and the mirror words, with the event that says the mirror has arrived.  Two slots
    in turn: a slot's words are uploaded in one step and its mirror is read at the end of that step, before the slot
    comes round again."""
    ring = _PLAN_HOST.get(n_words)
    if ring is None:
        ring = _PLAN_HOST[n_words] = {"slots": [dict(words=torch.empty(n_words, dtype=torch.int32).pin_memory(),
                                                      mirror=torch.zeros(3 * MAXC + 2, dtype=torch.int32).pin_memory(),
                                                      event=torch.cuda.Event()) for _ in range(2)], "next": 0}
    slot = ring["slots"][ring["next"]]
    ring["next"] = (ring["next"] + 1) % len(ring["slots"])
    return slot


def sampling_device_ok(rep_rows, ph1, bank, cfg):
    """the shapes u2pl_infonce_plan + u2pl_infonce_fused_dev_f32 are built for; every bound a draw can have (a list holds
    at most P pixels, a ring at most its capacity) is below the generator's one-word limit"""
    from . import rng_words as RW
    Q, D = int(cfg["num_queries"]), rep_rows.shape[1]
    return (NCE_FUSED and not ph1.wide and Q % 4 == 0 and 0 < Q <= 1024 and int(cfg["num_negatives"]) > 0 and D <= 256
            and D in (64, 128, 256) and ph1.cap < RW.ONE_WORD_BOUND and max(bank.cap) < RW.ONE_WORD_BOUND)


def sampling_plan(ph1, bank, C, Q, K, D, words=None):
    """u2pl_infonce_plan on the current stream: raw words of the global CPU generator (not advanced), the plan's device
    buffers, and the asynchronous copy of the mirror words to pinned memory.  -> dict of buffers + the host slot.
    words (uint32 [C (Q + Q K)], tests): these instead of the generator's."""
    from . import rng_words as RW
    dev = ph1.counts.device
    per = Q + Q * K
    slot = _plan_host_slot(C * per)
    if words is None:
        words = RW.peek_words(C * per)
    slot["words"].numpy()[:] = np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)
    words = slot["words"].to(dev, non_blocking=True)
    bank._sync_state()
    plan = dict(max_jobs=C, per=per, slot=slot, words=words, ph1=ph1,
                jobs=torch.empty((C, 7), dtype=torch.int64, device=dev),
                idx=torch.empty((C, per), dtype=torch.int64, device=dev),
                groups=torch.empty((3, C * Q), dtype=torch.int32, device=dev),
                apix=torch.empty((C, Q), dtype=torch.int32, device=dev),
                hdr=torch.empty(query("u2pl_infonce_plan_hdr_bytes") // 4, dtype=torch.int32, device=dev),
                mirror=torch.empty(3 * MAXC + 2, dtype=torch.int32, device=dev),
                loss=torch.empty((), dtype=torch.float32, device=dev))
    assert query("u2pl_infonce_job_bytes") == 56
    call("u2pl_infonce_plan", ph1.counts, bank.state, words, C, Q, K, ph1.idx, ph1.cap, ph1.proto, D, bank.storage,
         plan["jobs"], plan["idx"], plan["groups"], plan["apix"], plan["hdr"], plan["mirror"], plan["loss"])
    slot["mirror"].copy_(plan["mirror"], non_blocking=True)
    slot["event"].record()
    return plan


def infonce_loss_device(rep_rows, ph1, bank, cfg, words=None):
    """Phase 2 (loss_helper.py:156-233) without the host knowing the list lengths: plan, InfoNCE forward at the worst-case
    grid.  -> (loss, plan); the loss is exactly 0 and its gradient all zeros when there is no job or at most one valid
    class (what zero_times_sum gives on the host path)."""
    Q, K = int(cfg["num_queries"]), int(cfg["num_negatives"])
    plan = sampling_plan(ph1, bank, ph1.C, Q, K, rep_rows.shape[1], words)
    loss = _InfoNCEDev.apply(rep_rows, plan, Q, K, float(cfg["temperature"]))
    infonce_loss_device.last_plan = plan     # (tests and bench.py's replay look at the tables of the last step)
    return loss, plan


def plan_mirror(plan):
    """wait for the plan's mirror words (they were copied right behind the planning kernel) -> counts uint32-valued
    int64 [3][32], njobs, valid_seg"""
    plan["slot"]["event"].synchronize()
    m = plan["slot"]["mirror"].numpy().view(np.uint32).astype(np.int64)
    return m[:3 * MAXC].reshape(3, MAXC), int(m[3 * MAXC]), int(m[3 * MAXC + 1])


def infonce_loss(rep_rows, ph1, bank, valid_classes, counts_host, cfg, randint=None):
    """Phase 2 (loss_helper.py:156-233) incl. the class-index mismatch (Q1).
    randint(high, n) defaults to torch.randint on the global CPU generator."""
    Q, K = int(cfg["num_queries"]), int(cfg["num_negatives"])
    valid_seg = len(valid_classes)
    if randint is None:
        def randint(high, n):
            return torch.randint(high, size=(n,))
    jobs, idx_chunks, ia_list = [], [], []
    for i in range(valid_seg):
        n_cand = int(counts_host[0][i])
        vc = valid_classes[i]
        if n_cand > 0 and bank.length[vc] > 0:
            ia = randint(n_cand, Q)
            inn = randint(bank.length[vc], Q * K)
            jobs.append((i, vc))
            idx_chunks += [ia.to(torch.int64), inn.to(torch.int64)]
            ia_list.append(ia.numpy())
    infonce_loss.last_njobs = len(jobs)
    if not jobs:
        return None
    dev = rep_rows.device
    idx_all = h2d(torch.cat(idx_chunks), dev)
    base = idx_all.data_ptr()
    D = rep_rows.shape[1]
    jb = np.zeros((len(jobs), 7), dtype=np.int64)
    off = 0
    for j, (i, vc) in enumerate(jobs):
        jb[j, 0] = ph1.list_ptr(0, i)         # Q1: the anchor list of class i = the POSITION in valid_classes, not of vc
        jb[j, 1] = base + off * 8
        jb[j, 2] = base + (off + Q) * 8
        jb[j, 3] = ph1.proto.data_ptr() + i * D * 4
        jb[j, 4] = bank.buf[vc].data_ptr()
        jb[j, 5] = bank.cap[vc]
        jb[j, 6] = bank.head[vc]
        off += Q + Q * K
    assert query("u2pl_infonce_job_bytes") == 56
    jobs_dev = h2d(torch.from_numpy(jb), dev)
    groups = h2d(torch.from_numpy(group_entries(ia_list, Q)), dev)
    if REPLAY is not None:
        REPLAY["infonce"] = (rep_rows.detach(), jobs_dev, len(jobs), Q, K, float(cfg["temperature"]), valid_seg, groups,
                             (idx_all, ph1, bank))
    return _InfoNCE.apply(rep_rows, jobs_dev, len(jobs), Q, K, float(cfg["temperature"]), valid_seg, groups,
                          (idx_all, ph1))
