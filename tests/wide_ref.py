"""numpy side of the tests of the route for more than 32 classes: word planes, the flat list layout, and phase 1 restated
through oracle/restate.py (contra_phase1, class_rank, label_onehot_quirk -- all generic in the class count)."""
import numpy as np

from conftest import golden
from oracle import restate as R

CONTRA_TAGS = ["c33", "c40s", "c65", "c150s", "c255"]


def words(C):
    return (C + 31) // 32


def full_prob(prob_slot0, B):
    """the (2B,C,h,w) probabilities the reference was fed: images 0 and B from the fixture, the constant 1 / C elsewhere
    (no other image carries a label bit under the label_onehot slot-0 quirk; tools/gen_wide_golden.py)"""
    _, C, h, w = prob_slot0.shape
    out = np.full((2 * B, C, h, w), np.float32(1.0) / np.float32(C), dtype=np.float32)
    out[0], out[B] = prob_slot0[0], prob_slot0[1]
    return out


def planes_from_onehot(oh):
    """(N,C,h,w) multi-hot -> word planes (W,N,h,w) uint32: plane g, bit b = class 32 g + b"""
    N, C, h, w = oh.shape
    out = np.zeros((words(C), N, h, w), dtype=np.uint32)
    for c in range(C):
        out[c >> 5] |= (oh[:, c] != 0).astype(np.uint32) << np.uint32(c & 31)
    return out


def label_planes(label_l, label_u, C, s):
    """the label bits of the concatenated low-res batch as word planes (W,2B,s,s): label_onehot's slot-0 quirk on the
    full-size labels, then the legacy-nearest down-sampling (oracle/restate.py)"""
    oh = [R.nearest_down(R.label_onehot_quirk(lab, C), s, s) for lab in (label_l, label_u)]
    return planes_from_onehot(np.concatenate(oh))


def onehot_from_planes(planes, C):
    return np.stack([(planes[c >> 5] >> np.uint32(c & 31)) & np.uint32(1) for c in range(C)], 1).astype(np.int64)


def list_offsets(counts):
    """counts [3][C] -> first element of list (kind, class) in the flat buffer: lists back to back in (kind, class) order"""
    flat = np.asarray(counts, dtype=np.int64).reshape(-1)
    return (np.cumsum(flat) - flat).reshape(np.asarray(counts).shape)


def phase1_ref(rep_teacher, label_l, label_u, prob_l, prob_u, low_mask, high_mask, cfg):
    """-> dict(per = oracle.restate.contra_phase1's per-class dicts, bits uint32 [3][W][P] (anchor, low-valid, negative),
    counts int64 [3][C], flat = the flat list buffer, offsets)"""
    per = R.contra_phase1(rep_teacher, label_l, label_u, prob_l, prob_u, low_mask, high_mask, cfg)
    C = label_l.shape[1]
    P = (label_l.shape[0] + label_u.shape[0]) * label_l.shape[2] * label_l.shape[3]
    bits = np.zeros((3, words(C), P), dtype=np.uint32)
    counts = np.zeros((3, C), dtype=np.int64)
    keys = ("anchor_idx", "low_idx", "neg_idx")
    for c, o in enumerate(per):
        for kind, key in enumerate(keys):
            bits[kind, c >> 5, o[key]] |= np.uint32(1) << np.uint32(c & 31)
            counts[kind, c] = o[key].size
    flat = np.concatenate([per[c][keys[kind]] for kind in range(3) for c in range(C)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(per=per, bits=bits, counts=counts, flat=flat, offsets=list_offsets(counts))


def job_table(valid_classes, counts, bank_len):
    """loss_helper.py:173-196: job i (the POSITION in valid_classes) reads the anchor list of class i (quirk Q1) and the
    bank of valid_classes[i] -> [(i, vc)]"""
    return [(i, vc) for i, vc in enumerate(valid_classes) if counts[0][i] > 0 and bank_len[vc] > 0]


def load_contra(tag):
    """-> (meta, [step dicts]) of a contra_65_<tag> fixture"""
    meta = golden("contra_65_" + tag)
    return meta, [golden(f"contra_65_{tag}_s{st}") for st in range(int(meta["num_steps"]))]


def bank_ends(b, D):
    """first / last two rows as tools/gen_wide_golden.py stores them (zero padded below two rows)"""
    p = np.concatenate([b, np.zeros((max(0, 2 - b.shape[0]), D), b.dtype)])
    return p[:2], (p[-2:] if b.shape[0] >= 2 else p[:2])
