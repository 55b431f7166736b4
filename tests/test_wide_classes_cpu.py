"""CPU half of the tests of training with more than 32 classes: the numpy restatement that the GPU stage test compares
against equals the reference-generated fixtures, the flat-list / job-table arithmetic, the class-count limits, and the
header declarations of the new entry points."""
import numpy as np
import pytest
import torch

import wide_ref as WR
from conftest import golden
from oracle import restate as R
from oracle.gen_golden import CONTRA_CFG


@pytest.mark.parametrize("tag", WR.CONTRA_TAGS)
def test_restatement_equals_the_reference_fixtures(tag):
    """per step: the restated negative-key lists have the reference's new_keys lengths, the valid classes and the job count
    (Q1: position i's anchor list, valid_classes[i]'s bank) are the reference's, and the bank lengths follow"""
    meta, steps = WR.load_contra(tag)
    C, B = int(meta["num_classes"]), int(meta["B"])
    qs = [int(x) for x in meta["queue_size"]]
    lens = [int(x) for x in meta["fill"]]
    for g in steps:
        prob = WR.full_prob(g["prob_slot0"], B)
        ref = WR.phase1_ref(g["rep_teacher"], g["label_l_small"].astype(np.int64), g["label_u_small"].astype(np.int64),
                            prob[:B], prob[B:], g["low_mask_all"].astype(np.float32), g["high_mask_all"].astype(np.float32),
                            CONTRA_CFG)
        assert list(ref["counts"][2]) == list(g["new_keys"])
        lens = [min(lens[c] + int(ref["counts"][2][c]), qs[c]) for c in range(C)]
        assert lens == list(g["bank_len"])
        valid = [c for c in range(C) if ref["counts"][1][c] > 0]
        assert len(WR.job_table(valid, ref["counts"], lens)) == int(g["njobs"])
        # the planes hold exactly the lists
        oh = WR.onehot_from_planes(ref["bits"][0].reshape(WR.words(C), 2 * B, *prob.shape[2:]), C)
        assert [int(oh[:, c].sum()) for c in range(C)] == list(ref["counts"][0])


def test_fixtures_cover_what_they_are_for():
    meta, steps = WR.load_contra("c33")
    assert any(g["new_keys"][32] > 0 for g in steps)
    meta, steps = WR.load_contra("c40s")
    assert max(int(g["njobs"]) for g in steps) > 32
    assert any(int(meta["fill"][c]) + int(steps[0]["new_keys"][c]) > int(meta["queue_size"][c]) for c in range(40))     # a ring wraps
    meta, steps = WR.load_contra("c150s")
    assert all(int(g["njobs"]) > 32 for g in steps)


@pytest.mark.parametrize("tag,B", [("c150", 2), ("c150_b3", 3)])
def test_label_bits_restatement_equals_the_reference_label_onehot(tag, B):
    g = golden("relsplit_65_" + tag)
    C, s = int(g["num_classes"]), g["label_l_small"].shape[-1]
    for lab, want in ((g["label_l"], g["label_l_small"]), (g["label_u_aug"], g["label_u_small"])):
        oh = R.nearest_down(R.label_onehot_quirk(lab.astype(np.int64), C), s, s)
        assert np.array_equal(oh.astype(np.uint8), want)
        planes = WR.planes_from_onehot(oh)
        assert planes.shape[0] == 5 and np.array_equal(WR.onehot_from_planes(planes, C), oh.astype(np.int64))
    if B == 3:
        assert int(g["label_l_small"].sum(1).max()) == 3 or int(g["label_u_small"].sum(1).max()) == 3     # three labels on one pixel (Q0)


def test_flat_list_offsets_and_job_table_arithmetic():
    """hipops.wide_list_offsets = the running sum in (kind, class) order; ContraPhase1.list_ptr / list address list
    (kind, c) by it; the job of position i reads list (0, i), not (0, valid_classes[i]) (Q1)"""
    from u2pl_amd import hipops as H
    rng = np.random.default_rng(3)
    C = 150
    counts = rng.integers(0, 5, size=(3, C))
    counts[:, 7] = 0
    off = H.wide_list_offsets(counts)
    assert np.array_equal(off, WR.list_offsets(counts))
    assert off[0, 0] == 0 and off[1, 0] == counts[0].sum() and off[2, C - 1] == counts.sum() - counts[2, C - 1]
    ph = H.ContraPhase1()
    ph.wide, ph.C, ph.cap = True, C, 10 ** 6
    ph.idx = torch.arange(int(counts.sum()), dtype=torch.int32)
    ph.offsets_host, ph.counts_host = off, counts
    for kind, c in ((0, 0), (0, 33), (1, 149), (2, 128), (2, 7)):
        lst = ph.list(kind, c)
        assert lst.numel() == counts[kind, c]
        assert ph.list_ptr(kind, c) == ph.idx.data_ptr() + 4 * int(off[kind, c])
        if lst.numel():
            assert int(lst[0]) == off[kind, c]
    assert [v.numel() for v in ph.lists(2)] == list(counts[2])
    # the narrow layout's address, unchanged: idx[kind][c] of an int32 (3, 32, P) array
    nr = H.ContraPhase1()
    nr.wide, nr.C, nr.cap = False, 19, 1156
    nr.idx = torch.zeros((3, H.MAXC, 1156), dtype=torch.int32)
    assert nr.list_ptr(0, 5) == nr.idx.data_ptr() + (0 * 32 + 5) * 1156 * 4 == nr.idx[0, 5].data_ptr()
    valid = [c for c in range(C) if counts[1][c] > 0]
    jobs = WR.job_table(valid, counts, [1] * C)
    assert 7 not in valid and any(i != vc for i, vc in jobs)
    assert H.wide_words(32) == 1 and H.wide_words(33) == 2 and H.wide_words(255) == 8 and H.MAXC == 32 and H.WIDE_MAXC == 255


def test_more_than_255_classes_is_a_value_error():
    from u2pl_amd import _lib, configs, hipops as H
    from u2pl_amd.trainer import SemiTrainer, SupTrainer
    from u2pl_amd.utils.loss_helper import compute_contra_memobank_loss
    H.check_num_classes(255)
    with pytest.raises(ValueError, match="too many classes"):
        H.check_num_classes(256)
    cfg = configs.cityscapes_semi(arch="resnet50", crop=65, batch_size=2, sync_bn=False, num_classes=256)
    with pytest.raises(ValueError, match="256.*too many classes"):
        SemiTrainer(cfg, None, None, None, steps_per_epoch=2)
    with pytest.raises(ValueError, match="too many classes"):
        SupTrainer(cfg, None, None, steps_per_epoch=2)
    z = torch.zeros(2, 256, 3, 3)
    with pytest.raises(ValueError, match="too many classes"):
        compute_contra_memobank_loss(torch.zeros(4, 8, 3, 3), z.long(), z.long(), z, z, None, None, CONTRA_CFG, None, None, None, None)
    with pytest.raises(ValueError, match="too many classes"):
        H.DeviceMemoryBank(256, [4] * 256, 8, "cpu")
    with pytest.raises(ValueError, match="too many classes"):
        H.unpack_class_bits(torch.zeros(8, 1, 2, 2, dtype=torch.int32), 256)
    with pytest.raises(_lib.HipError, match="planes"):
        H.unpack_class_bits(torch.zeros(2, 1, 2, 2, dtype=torch.int32), 150)


def test_wide_entry_points_are_declared_and_sized():
    from u2pl_amd import _lib
    decls = _lib.parse_header()
    names = ["u2pl_wide_words", "u2pl_reliability_masks_wide", "u2pl_reliability_apply_wide", "u2pl_pack_class_bits_wide",
             "u2pl_unpack_class_bits_wide", "u2pl_contra_wide_workspace_bytes", "u2pl_contra_wide_block_pixels",
             "u2pl_contra_wide_staged", "u2pl_contra_classify_wide", "u2pl_compact_lists_wide", "u2pl_class_prototypes_wide", "u2pl_bank_init_wide",
             "u2pl_bank_enqueue_wide_f32"]
    L = _lib.lib()
    for n in names:
        assert n in decls and hasattr(L.cdll, n), n
    assert [L.u2pl_wide_words(c) for c in (1, 32, 33, 255, 256)] == [1, 1, 2, 8, 0]
    for C in (19, 33, 64, 97, 186, 187, 255):
        pix = L.u2pl_contra_wide_block_pixels(C)
        assert pix in (64, 128, 256)
        assert L.u2pl_contra_wide_workspace_bytes(1000, C) == -(-1000 // pix) * 3 * C * 4
    # the staging edges: (pixels + 3) * C * 4 <= 48 KB -- 256 pixels up to C = 47, 128 up to 93, 64 (staged) up to 183
    assert [L.u2pl_contra_wide_block_pixels(c) for c in (47, 48, 93, 94, 183, 184, 255)] == [256, 128, 128, 64, 64, 64, 64]
    assert [L.u2pl_contra_wide_staged(c) for c in (1, 47, 48, 183, 184, 255, 256)] == [1, 1, 1, 1, 0, 0, 0]
    for c in range(1, 256):
        pix, st = L.u2pl_contra_wide_block_pixels(c), L.u2pl_contra_wide_staged(c)
        assert ((pix + 3) * c * 4 <= 48 * 1024) == bool(st) and (pix == 256 or (2 * pix + 3) * c * 4 > 48 * 1024)
    assert L.u2pl_contra_wide_block_pixels(256) == 0 and L.u2pl_contra_wide_workspace_bytes(1000, 256) == 0
