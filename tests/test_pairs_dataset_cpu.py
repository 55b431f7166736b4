"""Paired-list datasets (dataset.type pairs / pairs_semi) and dataset.label_map on the host: the validated 256-entry
label table, the `other: error` check of both dataset classes, label file modes, the host chain (table at load, before any
transform), list handling and resampling, colour and inverse tables, and that the two reference dataset types make the
calls they made before."""
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
ADE = dict(ignore_label=255, label_map=dict(offset=-1))
# Cityscapes labelIds -> trainIds (cityscapesScripts' label table): 34 raw ids, 19 classes, the rest void
CITY_TABLE = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14,
              28: 15, 31: 16, 32: 17, 33: 18}
CITY = dict(ignore_label=255, label_map=dict(table={v: CITY_TABLE.get(v, 255) for v in range(34)}))
MAPS = [(dict(ignore_label=255), 21), (ADE, 150), (CITY, 19)]


def invariant(lut, C, ignore=255):
    return lut.dtype == np.uint8 and lut.shape == (256,) and bool(((lut < C) | (lut == ignore)).all())


def test_build_label_lut_identity_offset_and_table():
    from u2pl_amd.dataset.builder import build_label_lut, label_tables

    lut = build_label_lut(dict(ignore_label=255), 21)
    assert invariant(lut, 21)
    assert np.array_equal(lut[:21], np.arange(21)) and (lut[21:] == 255).all()
    lut = build_label_lut(ADE, 150)
    assert invariant(lut, 150)
    assert lut[0] == 255 and np.array_equal(lut[1:151], np.arange(150)) and (lut[151:] == 255).all()
    lut = build_label_lut(CITY, 19)
    assert invariant(lut, 19)
    for v in range(256):
        assert lut[v] == CITY_TABLE.get(v, 255)
    # `table` wins over `offset`; the raw ignore value stays the ignore value unless the table lists it
    lut = build_label_lut(dict(ignore_label=255, label_map=dict(offset=-1, table={7: 0, 8: 1, 255: 1})), 2)
    assert invariant(lut, 2) and lut[7] == 0 and lut[8] == 1 and lut[255] == 1 and lut[1] == 255 and lut[2] == 255
    # a lower ignore value: its own entry maps to itself, 255 is then an ordinary out-of-range value
    lut = build_label_lut(dict(ignore_label=200), 19)
    assert invariant(lut, 19, 200) and lut[200] == 200 and lut[255] == 200 and lut[18] == 18
    # which raw values `other: error` refuses: everything without a class that is not the ignore value / listed
    _, bad = label_tables(ADE, 150)
    assert bad[0] and not bad[1:151].any() and bad[151:255].all() and not bad[255]
    _, bad = label_tables(CITY, 19)
    assert not bad[:34].any() and bad[34:255].all() and not bad[255]
    assert label_tables(dict(ADE, label_map=dict(offset=-1, other="ignore")), 150)[1] is None


def test_build_label_lut_refuses_bad_class_counts_and_ignore_values():
    from u2pl_amd.dataset.builder import build_label_lut

    with pytest.raises(ValueError, match="ignore_label"):
        build_label_lut(dict(ignore_label=100), 150)
    with pytest.raises(ValueError, match="256"):
        build_label_lut(dict(ignore_label=255), 256)
    with pytest.raises(ValueError, match="other"):
        build_label_lut(dict(ignore_label=255, label_map=dict(other="drop")), 19)
    with pytest.raises(ValueError, match="unknown keys"):
        build_label_lut(dict(ignore_label=255, label_map=dict(ofset=-1)), 19)


def _palette_png(path, arr):
    """mode P file whose palette luminances differ from the indices"""
    im = Image.fromarray(arr)
    im.putpalette((np.arange(256)[:, None] * np.array([151, 37, 91]) % 256).astype(np.uint8).reshape(-1).tolist())
    im.save(path)
    assert Image.open(path).mode == "P"


def _files(tmp_path, raw, h=40, w=56, seed=0, name="a"):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(img).save(os.path.join(tmp_path, name + ".png"))
    _palette_png(os.path.join(tmp_path, name + "_lab.png"), raw)
    return img


def _datasets(tmp_path, cfg_dataset, C, lines, pipe_cfg=None):
    from u2pl_amd.dataset.builder import Pipeline, SegDataset, label_tables
    from u2pl_amd.dataset.device_aug import AugmentPlan, RawSegDataset

    lst = os.path.join(tmp_path, "list.txt")
    open(lst, "w").write("\n".join(lines) + "\n")
    pc = pipe_cfg or dict(mean=MEAN, std=STD, crop=dict(type="center", size=[32, 32]))
    tables = label_tables(cfg_dataset, C)
    base = SegDataset(str(tmp_path), lst, Pipeline(pc), 0, None, "train", kind_hint="pairs", label_map=tables,
                      ignore_label=cfg_dataset["ignore_label"])
    return base, RawSegDataset(base, AugmentPlan(pc, lut=tables[0]))


def test_other_error_names_the_file_for_both_dataset_classes(tmp_path):
    raw = np.random.default_rng(1).integers(1, 151, (40, 56), dtype=np.uint8)
    raw[3, 4], raw[9, 9] = 200, 0          # 200 has no class; neither has 0 ("unlabeled") under offset -1
    _files(tmp_path, raw)
    host, dev = _datasets(tmp_path, ADE, 150, ["a.png a_lab.png"])
    for ds in (host, dev):
        with pytest.raises(ValueError, match=r"a_lab\.png.*\[0, 200\]"):
            ds[0]
    host, dev = _datasets(tmp_path, dict(ADE, label_map=dict(offset=-1, other="ignore")), 150, ["a.png a_lab.png"])
    lab = host[0][1]
    assert lab.shape == (32, 32)
    assert np.array_equal(dev[0][1].numpy(), raw)          # the device pipeline gets the RAW bytes: the GPU maps them


def test_palette_labels_are_indices_and_16_bit_labels_are_refused(tmp_path):
    from u2pl_amd.dataset.builder import read_label

    raw = np.random.default_rng(2).integers(0, 151, (40, 56), dtype=np.uint8)
    _files(tmp_path, raw)
    p = os.path.join(tmp_path, "a_lab.png")
    assert not np.array_equal(np.asarray(Image.open(p).convert("L")), raw)     # what convert("L") would have given
    assert np.array_equal(read_label(p), raw)
    Image.fromarray(raw).save(os.path.join(tmp_path, "l.png"))                 # mode L
    assert np.array_equal(read_label(os.path.join(tmp_path, "l.png")), raw)
    for mode, arr in (("I;16", raw.astype(np.uint16) * 3), ("I", raw.astype(np.int32) * 1000)):
        q = os.path.join(tmp_path, "wide.png" if mode == "I;16" else "wide.tif")
        Image.fromarray(arr).save(q)
        assert Image.open(q).mode == mode
        with pytest.raises(ValueError, match=os.path.basename(q).replace(".", r"\.") + ".*16-bit"):
            read_label(q)
    host, dev = _datasets(tmp_path, dict(ADE, label_map=dict(offset=-1, other="ignore")), 150, ["a.png wide.png"])
    for ds in (host, dev):
        with pytest.raises(ValueError, match=r"wide\.png"):
            ds[0]


@pytest.mark.parametrize("seed", range(4))
def test_host_chain_maps_at_load_before_any_transform(tmp_path, seed):
    """SegDataset + Pipeline with a table == mapping the array first and running today's Pipeline, bit for bit, with
    rotation, blur, flip and a crop larger than the image; the padded border is class 0 although lut[0] == 255"""
    from u2pl_amd.dataset.builder import Pipeline, build_label_lut

    pc = dict(mean=MEAN, std=STD, ignore_label=255, rand_resize=[0.5, 1.2], rand_rotation=[-10.0, 10.0], GaussianBlur=True,
              flip=True, crop=dict(type="center", size=[80, 96]))
    raw = np.random.default_rng(10 + seed).integers(0, 256, (40, 56), dtype=np.uint8)
    raw[5:9, 5:9] = 1                       # raw 1 -> class 0 exists inside the frame too
    img = _files(tmp_path, raw, seed=seed)
    host, _ = _datasets(tmp_path, dict(ADE, label_map=dict(offset=-1, other="ignore")), 150, ["a.png a_lab.png"], pc)
    lut = build_label_lut(ADE, 150)
    assert lut[0] == 255
    random.seed(50 + seed)
    oi, ol = host[0]
    after = random.random()
    random.seed(50 + seed)
    ri, rl = Pipeline(pc)(Image.fromarray(img), Image.fromarray(lut[raw]))
    assert random.random() == after
    assert torch.equal(oi.view(torch.int32), ri.view(torch.int32)) and torch.equal(ol, rl)
    assert ol.shape == (80, 96)
    assert (ol[:16] == 0).all() and (ol[-16:] == 0).all() and (ol[:, :14] == 0).all()     # at least (80 - 48) // 2 rows, (96 - 67) // 2 columns of padding
    assert bool(((ol < 150) | (ol == 255)).all())


def test_pairs_semi_lists_resampling_and_unlabeled_lines(tmp_path):
    import make_synth_dataset as M
    import yaml

    from u2pl_amd.dataset.builder import SegDataset, get_loader, parse_list, parse_pairs

    d, s = M.make_pairs(str(tmp_path), n_l=2, n_u=5, n_val=3, H=40, W=56, C=40, mixed_sizes=True)
    cfg = yaml.safe_load(open(M.write_pairs_config(str(tmp_path), d, s, C=40, crop=33)))
    cfg["dataset"]["batch_size"] = 1
    with pytest.raises(ValueError, match="unknown dataset list"):
        parse_list(os.path.join(s, "labeled.txt"))            # the path-driven parser is as it was
    sup, unsup, val = get_loader(cfg, seed=3)
    assert len(sup.dataset) == len(unsup.dataset) == 5 and len(val.dataset) == 3
    # the labeled list (2 lines) is tiled, then sampled, in SegDataset's random.seed(seed) order
    pairs = parse_pairs(os.path.join(s, "labeled.txt"))
    random.seed(3)
    assert sup.dataset.samples == random.sample(pairs * 3, 5)
    assert sorted(unsup.dataset.samples) == sorted(parse_pairs(os.path.join(s, "unlabeled.txt")))
    assert all(lp is None for _, lp in unsup.dataset.samples)
    for i in range(5):
        assert (unsup.dataset.raw_label(None, 40, 56) == 255).all()
        assert set(unsup.dataset[i][1].unique().tolist()) <= {0, 255}       # 0: the crop's padding of a shrunken sample
        lab = sup.dataset[i][1]
        assert bool(((lab < 40) | (lab == 255)).all()) and (lab < 40).any()
    # dataset.train.unlabeled_list names another list: both loaders take ITS length
    other = os.path.join(str(tmp_path), "more.txt")
    open(other, "w").write("".join(ip + "\n" for ip, _ in parse_pairs(os.path.join(s, "val.txt"))))
    cfg["dataset"]["train"]["unlabeled_list"] = other
    sup, unsup, _ = get_loader(cfg, seed=3)
    assert len(sup.dataset) == len(unsup.dataset) == 3
    # `pairs` (supervised): resampled only when n_sup is given
    cfg["dataset"]["type"] = "pairs"
    sup, _ = get_loader(cfg, seed=3)
    assert sup.dataset.samples == pairs
    cfg["dataset"]["n_sup"] = 7
    assert len(get_loader(cfg, seed=3)[0].dataset) == 7
    # the device pipeline carries the table, the identity one included
    cfg["dataset"]["device_aug"] = True
    assert np.array_equal(get_loader(cfg, seed=3)[0].device_plan.lut, sup.dataset.lut)
    cfg["dataset"].pop("label_map")
    plan = get_loader(cfg, seed=3)[0].device_plan
    assert np.array_equal(plan.lut[:40], np.arange(40)) and (plan.lut[40:] == 255).all()
    assert isinstance(sup.dataset, SegDataset)


def test_head_lr_times():
    from u2pl_amd.trainer import head_lr_times

    assert head_lr_times(dict(type="pairs_semi")) == 1 and head_lr_times(dict(type="pairs", head_lr_times=10)) == 10
    assert head_lr_times(dict(type="pascal_semi", head_lr_times=3)) == 10
    assert head_lr_times(dict(type="cityscapes_semi", head_lr_times=3)) == 1


def test_generic_colormap_and_inverse_tables():
    from u2pl_amd.dataset.builder import build_label_lut, raw_id_lut
    from u2pl_amd.infer import colormap, dataset_colormap

    g = colormap("generic")
    assert g.shape == (256, 3) and g.dtype == np.uint8
    assert len({tuple(r) for r in g.tolist()}) == 256
    assert np.array_equal(g[:21], colormap("pascal")[:21])
    assert np.array_equal(dataset_colormap(dict(type="pairs_semi"), "pascal"), g)
    assert np.array_equal(dataset_colormap(dict(type="pairs", colormap="cityscapes"), "pascal"), colormap("cityscapes"))
    assert np.array_equal(dataset_colormap(dict(type="cityscapes_semi"), "pascal"), colormap("pascal"))
    for cfg, C in MAPS:
        lut = build_label_lut(cfg, C)
        inv = raw_id_lut(lut, 255)
        assert inv.dtype == np.uint8 and inv.shape == (256,)
        assert np.array_equal(lut[inv[:C]], np.arange(C))            # class -> raw -> class
        for c in range(C):
            assert inv[c] == np.flatnonzero(lut == c).min()           # the SMALLEST raw value of the class
        assert inv[255] == 255
    assert np.array_equal(raw_id_lut(build_label_lut(ADE, 150))[:150], np.arange(1, 151))
    assert raw_id_lut(build_label_lut(CITY, 19))[18] == 33


def test_raw_ids_is_refused_for_the_reference_dataset_types():
    sys.path.insert(0, ROOT)
    import importlib

    ev = importlib.import_module("eval")
    with pytest.raises(SystemExit, match="raw_ids"):
        ev.raw_id_table(dict(dataset=dict(type="cityscapes_semi"), net=dict(num_classes=19)), True)
    assert ev.raw_id_table(dict(dataset=dict(type="cityscapes_semi"), net=dict(num_classes=19)), False) is None
    t = ev.raw_id_table(dict(dataset=dict(ADE, type="pairs"), net=dict(num_classes=150)), True)
    assert t[0] == 1 and t[149] == 150 and t[255] == 255


@pytest.mark.parametrize("kind", ["cityscapes", "cityscapes_blur", "pascal_packed", "pairs", "pairs_rot_blur", "pairs_packed"])
def test_entry_points_of_augment_batch(kind, monkeypatch):
    """the reference dataset types issue the entry points they issued before the table existed; a plan with a table
    issues u2pl_augment_lut_u8_f32 for every batch layout (recorded at device_aug.call: nothing runs)"""
    from u2pl_amd.dataset import device_aug as D

    names = []
    monkeypatch.setattr(D, "call", lambda name, *a: names.append((name, len(a))))
    monkeypatch.setattr(D, "query", lambda name, B, Sh, Sw, mode: B * 3 * (Sh + 4) * (Sw + 4) * 4)
    cfg = dict(mean=MEAN, std=STD, ignore_label=255, rand_resize=[0.5, 2.0], flip=True, crop=dict(type="rand", size=[33, 33]))
    if kind.endswith("blur"):
        cfg.update(GaussianBlur=True, rand_rotation=[-10.0, 10.0])
    lut = np.arange(256, dtype=np.uint8) if kind.startswith("pairs") else None
    plan = D.AugmentPlan(cfg) if lut is None else D.AugmentPlan(cfg, lut=lut)
    sizes = [(40, 56), (44, 50)] if kind.endswith("packed") else [(40, 56)] * 2
    items = [(torch.zeros((h, w, 3), dtype=torch.uint8), torch.zeros((h, w), dtype=torch.uint8),
              torch.from_numpy(plan.draw(h, w))) for h, w in sizes]
    D.augment_batch(plan, *D.RawSegDataset.collate_fn(items), device="cpu")
    want = {"cityscapes": ("u2pl_augment_u8_f32", 12), "cityscapes_blur": ("u2pl_augment_ex_u8_f32", 17),
            "pascal_packed": ("u2pl_augment_ex_u8_f32", 17)}.get(kind, ("u2pl_augment_lut_u8_f32", 18))
    assert names == [want]


def test_reference_dataset_types_carry_no_table(tmp_path):
    import make_synth_dataset as M
    import yaml

    from u2pl_amd.dataset.builder import get_loader

    d, s = M.make_cityscapes(str(tmp_path), H=40, W=56)
    cfg = yaml.safe_load(open(M.write_city_config(str(tmp_path), d, s, crop=33)))
    cfg["dataset"]["device_aug"] = True
    cfg["dataset"]["label_map"] = dict(offset=-1)           # not a key of this dataset type: ignored
    sup, unsup, val = get_loader(cfg, seed=2)
    assert sup.device_plan.lut is None and sup.dataset.base.lut is None and val.dataset.lut is None
    img, lab, rec = sup.dataset[0]
    assert lab.dtype == torch.uint8 and rec.shape == (8,)


def test_the_example_config_builds_the_ade20k_table():
    import yaml

    from u2pl_amd.dataset.builder import label_tables

    cfg = yaml.safe_load(open(os.path.join(ROOT, "tools", "ade20k_pairs_example.yaml")))
    assert cfg["dataset"]["type"] == "pairs_semi" and cfg["net"]["num_classes"] == 150
    lut, bad = label_tables(cfg["dataset"], cfg["net"]["num_classes"])
    assert bad is None and lut[0] == 255 and np.array_equal(lut[1:151], np.arange(150)) and (lut[151:] == 255).all()
