"""numpy / torch (CPU) restatements of the prediction-side reliability maps (u2pl_predict_entropy_f32, u2pl_reliable_map_u8;
the reference's rule is compute_unsupervised_loss, loss_helper.py:30-48).  Shared by tests/test_reliability_cpu.py and
tests/test_gpu_reliability.py.

  entropy_ref64            the reference expression -sum(p * log(p + 1e-10)) of softmax(z), float64
  entropy_logits_f64/f32   the kernel's expression log(s) - t / s, in float64 / term for term in float32
  entropy_prob_f64/f32     class weights a_c -> q = a / sum(a), -sum(q log q), log(C) where the sum is not positive
  heat_bytes               the heat map byte as a numpy float32 expression
  reliable_map_np          drop, colours, heat and count of u2pl_reliable_map_u8
  predict_entropy_t, entropy_threshold_t, reliable_map_t, drop_high_entropy_t, confusion_hist_t
                           torch stand-ins with the signatures of u2pl_amd.hipops, for the host-logic tests
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def entropy_ref64(z):
    """z (..., C, H, W) logits -> (..., H, W) float64: loss_helper.py:35-36 / train_semi.py:402-403"""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(-3, keepdims=True))
    p = e / e.sum(-3, keepdims=True)
    return -(p * np.log(p + 1e-10)).sum(-3)


def _logits_entropy(z, dt):
    z = np.asarray(z, dtype=dt)
    C = z.shape[-3]
    m = z.max(-3)
    s = np.zeros(m.shape, dt)
    t = np.zeros(m.shape, dt)
    for c in range(C):                      # classes upward, every operation rounded to dt
        d = (z[..., c, :, :] - m).astype(dt)
        e = np.exp(d).astype(dt)
        s = (s + e).astype(dt)
        t = (t + (e * d).astype(dt)).astype(dt)
    return (np.log(s).astype(dt) - (t / s).astype(dt)).astype(dt)


def entropy_logits_f64(z):
    return _logits_entropy(z, np.float64)


def entropy_logits_f32(z):
    return _logits_entropy(z, np.float32)


def _prob_entropy(a, dt):
    a = np.asarray(a, dtype=dt)
    C = a.shape[-3]
    S = np.zeros(a.shape[:-3] + a.shape[-2:], dt)
    for c in range(C):
        S = (S + a[..., c, :, :]).astype(dt)
    acc = np.zeros(S.shape, dt)
    ok = S > 0
    safe = np.where(ok, S, dt(1))
    for c in range(C):
        p = (a[..., c, :, :] / safe).astype(dt)
        pos = p > 0
        term = (p * np.log(np.where(pos, p, dt(1))).astype(dt)).astype(dt)
        acc = (acc + np.where(pos, term, dt(0))).astype(dt)
    return np.where(ok, (dt(0) - acc).astype(dt), np.log(dt(C)).astype(dt)).astype(dt)


def entropy_prob_f64(a):
    """float64 -sum(q log q) of the float32 class weights as they are given"""
    return _prob_entropy(a, np.float64)


def entropy_prob_f32(a):
    return _prob_entropy(a, np.float32)


def heat_scale(C):
    return np.float32(255 / math.log(C))


def heat_bytes(ent, C):
    """clamp((int)(entropy * scale + 0.5), 0, 255) with the product and the sum each rounded to float32"""
    ent = np.asarray(ent, dtype=np.float32)
    x = (ent * heat_scale(C)).astype(np.float32) + np.float32(0.5)
    assert x.dtype == np.float32
    return np.clip(np.clip(x, -1.0, 256.0).astype(np.int32), 0, 255).astype(np.uint8)


def reliable_map_np(label, ent, thr, palette, heat_classes):
    """-> (label_out, rgb | None, heat | None, ndropped | None); thr: float32 scalar or None"""
    label = np.asarray(label, np.uint8)
    drop = np.zeros(label.shape, bool) if thr is None else np.asarray(ent, np.float32) >= np.float32(thr)
    out = np.where(drop, np.uint8(255), label).astype(np.uint8)
    rgb = None if palette is None else np.asarray(palette)[out]
    heat = None if heat_classes is None else heat_bytes(ent, heat_classes)
    return out, rgb, heat, None if thr is None else int(drop.sum())


# ------------------------------------------------------------------ torch stand-ins for u2pl_amd.hipops (CPU tensors)
def predict_entropy_t(scores_low, size, prob=False):
    up = F.interpolate(scores_low, size=tuple(int(v) for v in size), mode="bilinear", align_corners=True)
    label = up.argmax(1).to(torch.uint8)
    fn = entropy_prob_f32 if prob else entropy_logits_f32
    return label, torch.from_numpy(fn(up.numpy()))


def entropy_threshold_t(entropy, percent):
    return torch.from_numpy(np.percentile(entropy.numpy().ravel(), percent).astype(np.float32).reshape(1))


def reliable_map_t(label, entropy, thr=None, palette=None, heat_classes=None):
    out, rgb, heat, nd = reliable_map_np(label.numpy(), entropy.numpy(), None if thr is None else thr.numpy()[0],
                                         None if palette is None else palette.numpy(), heat_classes)
    label.copy_(torch.from_numpy(out))
    return (None if rgb is None else torch.from_numpy(rgb), None if heat is None else torch.from_numpy(heat),
            None if nd is None else torch.tensor([nd], dtype=torch.int32))


def drop_high_entropy_t(target, entropy, thr_bits, ignore=255):
    target[(entropy.reshape(target.shape) >= thr_bits[0]) & (target != ignore)] = ignore


def confusion_hist_t(logits, target, ignore, C, hist):
    """u2pl_confusion_hist_f32 on CPU tensors: hist (3*C,) int64 += intersection | output | target counts"""
    am = logits.reshape(C, -1).argmax(0)
    t = target.reshape(-1)
    live = t != ignore
    hist[C:2 * C] += torch.bincount(am[live], minlength=C)
    inside = live & (t >= 0) & (t < C)
    hist[2 * C:] += torch.bincount(t[inside], minlength=C)
    hist[:C] += torch.bincount(t[inside & (am == t)], minlength=C)


def hists_from_maps(gray, truth, C, ignore=255):
    """(3, C) integer counts of the kept pixels from a filtered gray map (255 = dropped) and the ground truth"""
    gray, truth = np.asarray(gray).astype(np.int64), np.asarray(truth).astype(np.int64)
    live = (truth != ignore) & (gray != 255)
    inside = live & (truth < C)
    return np.stack([np.bincount(truth[inside & (gray == truth)], minlength=C), np.bincount(gray[live], minlength=C),
                     np.bincount(truth[inside], minlength=C)])
