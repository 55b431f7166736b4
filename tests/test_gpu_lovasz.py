"""-m gpu: the Lovasz-Softmax route (u2pl_amd/csrc/lovasz.hip) against tests/lovasz_bounds.py -- stage by stage through the C
ABI (keys, the segmented sort, the gradient plane, the backward), end to end through H.lovasz_softmax, the criterion and both
trainers.  The sort is held to numpy's stable sort of the kernel's OWN keys bit for bit; the backward to float64 evaluated with
the kernel's own permutation, which the sort check has shown to be the stable one: no element is left out of a comparison."""
import copy
import math

import numpy as np
import pytest
import torch

import loss_bounds as LB
import lovasz_bounds as V
from decoder_harness import DEV, S_NET, assert_replay_equals_eager, train_steps

pytestmark = pytest.mark.gpu
TILE = V.TILE
SENT = 0x5EA7BEEF                   # sentinel word framing the buffers
GUARD = 64


def _call(name, *args):
    from u2pl_amd import _lib
    _lib.call(name, *args)


def _framed(n, dtype, fill):
    """a buffer of n elements between two guards of GUARD sentinel words (4-byte dtypes)"""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + n].view(dtype)
    view.fill_(fill)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- stage 2 on its own: the general sort ------------------------------------------------------------------------------------------
def _sort_case(kind, nseg, n, rng):
    if kind == "random":
        return rng.integers(0, 2 ** 32, (nseg, n), dtype=np.uint64).astype(np.uint32)
    if kind.startswith("digit"):                       # keys that differ in one 8-bit digit only
        d = int(kind[-1])
        return (np.uint32(0x12345678) & ~np.uint32(0xFF << (8 * d))) | (rng.integers(0, 256, (nseg, n)).astype(np.uint32) << np.uint32(8 * d))
    if kind == "equal":
        return np.full((nseg, n), 0x3F800000, dtype=np.uint32)
    base = np.sort(rng.integers(0, 2 ** 30, (nseg, n), dtype=np.uint64).astype(np.uint32), axis=1)
    return base if kind == "sorted" else np.ascontiguousarray(base[:, ::-1])


def _run_segsort(keys, lens, bits):
    from u2pl_amd import _lib
    L = _lib.lib()
    nseg, n = keys.shape
    vals = np.arange(nseg * n, dtype=np.uint32).reshape(nseg, n) * np.uint32(2654435761)
    bufs = []
    for src in (keys, vals, None, None):
        b, v = _framed(nseg * n, torch.int32, -1)
        if src is not None:
            v.copy_(torch.from_numpy(src.view(np.int32).reshape(-1)))
        bufs.append((b, v))
    ws = torch.full((L.u2pl_segsort_ws_bytes(nseg, n),), 255, dtype=torch.uint8, device=DEV)      # NaN-filled
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    _call("u2pl_segsort_u32", bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], ws, nseg, n, ld, bits)
    torch.cuda.synchronize()
    assert all(_guards_intact(b) for b, _ in bufs)
    odd = L.u2pl_segsort_passes(bits) % 2
    got_k, got_v = _u32(bufs[2 * odd][1]).reshape(nseg, n), _u32(bufs[1 + 2 * odd][1]).reshape(nseg, n)
    for s in range(nseg):
        ln = n if lens is None else max(0, min(int(lens[s]), n))
        rk, rv = V.stable_sort_ref(keys[s, :ln], vals[s, :ln], bits)
        assert np.array_equal(got_k[s, :ln], rk) and np.array_equal(got_v[s, :ln], rv), (s, ln)
        if not odd:         # past the length nothing is written: the input pair keeps its tail, the other pair its fill
            assert np.array_equal(got_k[s, ln:], keys[s, ln:]) and np.array_equal(got_v[s, ln:], vals[s, ln:])
        else:
            assert (got_k[s, ln:] == 0xFFFFFFFF).all() and (got_v[s, ln:] == 0xFFFFFFFF).all()


# lengths: 1, the wave edges, the tile edges, two tiles + 5, and the first lengths of a second block (a block orders 4 tiles;
# the grids have no cap, so there is no grid-stride trip to reach)
SORT_LENGTHS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 4 * TILE, 4 * TILE + 1)


@pytest.mark.parametrize("n", SORT_LENGTHS)
def test_segsort_is_the_stable_sort_at_every_length(n):
    rng = np.random.default_rng(n)
    for kind, bits in (("random", 32), ("random", 30), ("digit0", 32), ("digit1", 32), ("digit2", 32), ("digit3", 32), ("equal", 30),
                       ("sorted", 30), ("reverse", 30), ("random", 8), ("random", 17)):
        _run_segsort(_sort_case(kind, 1, n, rng), None, bits)


@pytest.mark.parametrize("nseg", (1, 2, 19))
def test_segsort_segments_of_unequal_fill(nseg):
    rng = np.random.default_rng(100 + nseg)
    n = 2 * TILE + 5
    pool = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, n - 1, n, n + 7, -3]
    lens = [pool[(3 * s + nseg) % len(pool)] for s in range(nseg)]
    for kind, bits in (("random", 30), ("digit2", 32), ("equal", 30), ("random", 12)):
        _run_segsort(_sort_case(kind, nseg, n, rng), lens, bits)
    few = rng.integers(0, 4, (nseg, n)).astype(np.uint32)          # four distinct keys: long runs of ties in every tile
    _run_segsort(few, lens, 30)


# ---- stages 1 .. 5 through the C ABI -------------------------------------------------------------------------------------------
def run_stages(z, t, classes="present", chunk=V.DEFAULT_CHUNK, gout=1.0, gmul=1.0):
    """every stage through its entry point, chunk by chunk, in NaN-prefilled and sentinel-framed buffers -> the dict
    lovasz_excess takes plus tilefg (the scanned tile counts of every class) and frames_ok"""
    from u2pl_amd import hipops as H
    N, C, Hh, W = z.shape
    P = N * Hh * W
    plan = H.lovasz_plan(P, C, chunk)
    zt, tt = torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV)
    wbuf = torch.full((plan["total"] + 8 * GUARD,), 255, dtype=torch.uint8, device=DEV)
    wbuf.view(torch.int32)[:GUARD] = SENT
    wbuf.view(torch.int32)[-GUARD:] = SENT
    work = wbuf[4 * GUARD:4 * GUARD + plan["total"]]
    gbuf, gplane = _framed(C * P, torch.float32, math.nan)
    obuf, out3 = _framed(3, torch.float32, math.nan)
    dbuf, grad = _framed(C * P, torch.float32, math.nan)
    present = int(classes == "present")
    keys, vals, skeys, svals, tilefg = [], [], [], [], []

    def words(off, rows, cols):
        return _u32(work[off:off + rows * cols * 4].view(torch.int32)).reshape(rows, cols).copy()

    for c0 in range(0, C, plan["cap"]):
        cc = min(plan["cap"], C - c0)
        _call("u2pl_lovasz_errors_f32", zt, tt, 255, N, C, Hh, W, c0, work, chunk)
        keys.append(words(plan["keys"], cc, P))
        vals.append(words(plan["vals"], cc, P))
        _call("u2pl_lovasz_sort", P, C, c0, work, chunk)
        skeys.append(words(plan["keys"], cc, P))
        svals.append(words(plan["vals"], cc, P))
        _call("u2pl_lovasz_grad_f32", P, C, c0, present, work, chunk, gplane)
        tilefg.append(words(plan["tilefg"], cc, plan["tiles"]))
    _call("u2pl_lovasz_finish_f32", P, C, present, work, chunk, out3)
    counts = words(plan["counts"], 1, C + 1)[0].astype(np.int64)
    go = torch.tensor(gout, dtype=torch.float32, device=DEV)
    _call("u2pl_lovasz_bwd_f32", zt, tt, 255, N, C, Hh, W, gplane, out3, go, float(gmul), grad)
    torch.cuda.synchronize()
    o3 = out3.cpu().numpy()
    frames_ok = (_guards_intact(gbuf) and _guards_intact(obuf) and _guards_intact(dbuf)
                 and _guards_intact(wbuf.view(torch.int32)))
    return dict(keys=np.concatenate(keys), vals=np.concatenate(vals), skeys=np.concatenate(skeys), svals=np.concatenate(svals),
                counts=counts, gplane=gplane.cpu().numpy().reshape(C, P), out3=o3,
                loss=np.float32(o3[0] * np.float32(gmul)) if gmul != 1.0 else o3[0],
                grad=grad.cpu().numpy().reshape(N, C, Hh, W), tilefg=np.concatenate(tilefg), frames_ok=frames_ok)


def _check_scans(got):
    """the scanned tile counts the gradient kernel starts from: the exclusive prefix of the foreground bits of the sorted payloads"""
    fg = (got["svals"] >> np.uint32(31)).astype(np.int64)
    C, P = fg.shape
    tiles = -(-P // TILE)
    per = np.pad(fg, ((0, 0), (0, tiles * TILE - P))).reshape(C, tiles, TILE).sum(2)
    assert np.array_equal(got["tilefg"], np.cumsum(per, 1) - per)


STAGE_CASES = [("trained", 19, (2, 65, 65), "some", "present", 19), ("saturated", 19, (2, 65, 65), "some", "all", 7),
               ("ties", 21, (3, 23, 31), "image", "present", 20), ("uniform", 2, (1, 7, 9), "none", "present", 1),
               ("wrong", 33, (3, 23, 31), "one", "all", 32), ("offset", 150, (1, 7, 9), "some", "present", 149),
               ("trained", 255, (1, 7, 9), "none", "present", 256), ("ties", 19, (1, 1, 1), "none", "present", 19),
               ("trained", 19, (3, 23, 31), "all", "present", 5), ("saturated", 5, (2, 64, 64), "none", "present", 2)]


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: "-".join(str(v) for v in c).replace(" ", ""))
def test_stages_through_the_c_abi(case):
    """keys within E_prob, fg / G / valid count exact, ignored behind valid; the sort is numpy's stable sort of the kernel's keys;
    scans exact, g within its bound, the plane fully written (NaN-prefilled: a missed slot is a NaN); loss and dz in bound"""
    fam, C, shape, pat, mode, chunk = case
    z, t = V.make_case(fam, C, shape)
    t = V.apply_ignore(t, pat)
    got = run_stages(z, t, mode, chunk, gout=1.7, gmul=0.4)
    assert got["frames_ok"]
    assert np.isfinite(got["gplane"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["out3"]).all()
    _check_scans(got)
    ex = V.lovasz_excess(got, z, t, mode, gout=1.7, gmul=0.4)
    print(case, {k: round(v, 3) for k, v in ex.items()})
    assert max(ex.values()) <= 1.0, ex


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _e2e_shapes(C):
    return V.SHAPES if C <= 33 else V.SHAPES[:3]           # small pixel counts at the wide class counts


E2E = [(C, shape, fam) for C in V.CLASSES for shape in _e2e_shapes(C) for fam in V.FAMILIES]


@pytest.mark.parametrize("C,shape,family", E2E, ids=lambda v: str(v).replace(" ", ""))
def test_lovasz_softmax_end_to_end(C, shape, family):
    """H.lovasz_softmax against float64 over the five ignore patterns; class mode, chunk size (1, C - 1, C, C + 1), scale and the
    upstream gradient rotate with the pattern and the family so that every pairing occurs over the grid; two runs, equal bits"""
    from u2pl_amd import hipops as H
    z, t0 = V.make_case(family, C, shape)
    zt = torch.from_numpy(z).to(DEV)
    fi = V.FAMILIES.index(family)
    for k, pat in enumerate(V.IGNORES):
        t = V.apply_ignore(t0, pat)
        tt = torch.from_numpy(t).to(DEV)
        mode = V.MODES[(k + fi) % 2]
        chunk = (1, C - 1, C, C + 1)[(k + 2 * fi + len(shape) * shape[1]) % 4]
        scale, gout = ((1.0, 1.0), (0.4, 1.7))[(k + fi // 2) % 2]
        runs = []
        for _ in range(2):
            x = zt.clone().requires_grad_(True)
            loss = H.lovasz_softmax(x, tt, 255, classes=mode, scale=scale, class_chunk=chunk)
            loss.backward(torch.tensor(gout, device=DEV))
            runs.append((loss.detach().cpu().numpy(), x.grad.cpu().numpy()))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        ref = V.lovasz_ref(z, t, mode, gout=gout, gmul=scale)
        b = V.E_lv_loss(C, t.size, ref["out3"][0]) * abs(scale) + V.EPS * abs(ref["loss"])
        assert abs(float(runs[0][0]) - ref["loss"]) <= b, (pat, mode, chunk, float(runs[0][0]), ref["loss"], b)
        grad = runs[0][1].astype(np.float64)
        # (the gradient is held element by element in test_stages_through_the_c_abi, under the kernel's own permutation)
        assert np.isfinite(grad).all() and (grad.transpose(0, 2, 3, 1)[t == 255] == 0).all()
        if ref["out3"][2] == 0:
            assert not grad.any() and float(runs[0][0]) == 0.0


# ---- criterion ---------------------------------------------------------------------------------------------------------------------
def _criterion_ref(main, aux, t, aux_weight, ce_w, lv_w, mode):
    total, bound = 0.0, 0.0
    C = main.shape[1]
    if ce_w:
        ce = LB.ce_ref(main, t, gmul=ce_w)
        total += ce["loss"]
        bound += LB.E_loss(C, float(np.abs(main).max()), 1.0, ce["out3"][0]) * abs(ce_w)
    if lv_w:
        lv = V.lovasz_ref(main, t, mode, gmul=lv_w)
        total += lv["loss"]
        bound += V.E_lv_loss(C, t.size, lv["out3"][0]) * abs(lv_w)
    if aux is not None:
        ce = LB.ce_ref(aux, t, gmul=aux_weight)
        total += ce["loss"]
        bound += LB.E_loss(C, float(np.abs(aux).max()), 1.0, ce["out3"][0]) * abs(aux_weight)
    return total, bound + 4 * V.EPS * abs(total)


@pytest.mark.parametrize("aux_weight", (0.0, 0.4))
@pytest.mark.parametrize("ce_w,lv_w,mode", ((1.0, 1.0, "present"), (0.0, 1.0, "all"), (1.0, 0.0, "present"), (0.5, 2.0, "present")))
def test_criterion_lovasz_against_float64(aux_weight, ce_w, lv_w, mode):
    from u2pl_amd.utils.loss_helper import CriterionLovasz
    from split_bounds import recorded_calls
    from u2pl_amd import hipops as H
    main, t = V.make_case("trained", 19, (2, 23, 31))
    aux, _ = V.make_case("wrong", 19, (2, 23, 31), seed=1)
    t = V.apply_ignore(t, "some")
    crit = CriterionLovasz(aux_weight, 255, ce_weight=ce_w, lovasz_weight=lv_w, classes=mode)
    xm = torch.from_numpy(main).to(DEV).requires_grad_(True)
    xa = torch.from_numpy(aux).to(DEV).requires_grad_(True)
    tt = torch.from_numpy(t).to(DEV)
    with recorded_calls(H) as seen:
        loss = crit([xm, xa], tt) if aux_weight > 0 else crit(xm, tt)
        loss.backward()
    torch.cuda.synchronize()
    ref, bound = _criterion_ref(main, aux if aux_weight > 0 else None, t, aux_weight, ce_w, lv_w, mode)
    assert abs(float(loss.detach()) - ref) <= bound, (float(loss.detach()), ref, bound)
    assert ("u2pl_lovasz_finish_f32" in seen) == (lv_w != 0) and ("u2pl_lovasz_bwd_f32" in seen) == (lv_w != 0)
    assert len(seen.get("u2pl_ce_fwd_f32", ())) == (ce_w != 0) + (aux_weight > 0)
    # the main head's gradient is the sum of the two terms' own gradients (each held to float64 by its own stage test): one fp32 add
    parts = []
    for on, fn in ((ce_w, lambda x: H.cross_entropy(x, tt, 255, scale=ce_w)),
                   (lv_w, lambda x: H.lovasz_softmax(x, tt, 255, classes=mode, scale=lv_w))):
        if on:
            x = torch.from_numpy(main).to(DEV).requires_grad_(True)
            fn(x).backward()
            parts.append(x.grad.double())
    want = sum(parts)
    assert bool(((xm.grad.double() - want).abs() <= V.EPS * sum(p.abs() for p in parts)).all())
    assert (xa.grad is not None) == (aux_weight > 0)


# ---- trainers ------------------------------------------------------------------------------------------------------------------------
def _use_lovasz(cfg):
    cfg["criterion"] = dict(type="lovasz", kwargs=dict(ce_weight=1.0, lovasz_weight=1.0, classes="present"))


def _lovasz_cfg():
    from u2pl_amd import configs
    cfg = configs.cityscapes_semi(arch="resnet50", crop=S_NET, batch_size=2, sync_bn=False, epochs=20)
    _use_lovasz(cfg)
    cfg["trainer"]["contrastive"]["current_class_threshold"] = 0.055
    return cfg


def test_semi_step_with_lovasz_eager_and_replayed(monkeypatch):
    """the eager run's criterion is wrapped: what it was handed at each step is recomputed in float64 below"""
    from u2pl_amd.utils import loss_helper
    rec = []

    def recording(cfg, real=loss_helper.get_criterion):
        crit = real(cfg)

        def fn(preds, target):
            rec.append(([p.detach().cpu().numpy().copy() for p in preds], target.cpu().numpy().copy()))
            return crit(preds, target)
        return fn
    with monkeypatch.context() as m:
        m.setattr(loss_helper, "get_criterion", recording)
        b = train_steps(m, False, _use_lovasz)
    a = train_steps(monkeypatch, True, _use_lovasz)
    print("graph stats", a["stats"], "meters", a["meters"])
    assert_replay_equals_eager(a, b)
    assert len(rec) == len(b["meters"])
    for (preds, target), m in zip(rec, b["meters"]):
        ref, _ = _criterion_ref(preds[0], preds[1], target, 0.4, 1.0, 1.0, "present")
        assert abs(float(m[0]) - ref) <= 1e-4 * max(1.0, abs(ref)), (float(m[0]), ref)


def test_sup_step_with_the_example_config():
    """tools/city_semi_lovasz_example.yaml's criterion and net (ResNet-50 in place of 101, no SyncBN) train a train_sup step"""
    import os
    import yaml
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SupTrainer
    from u2pl_amd.utils.loss_helper import CriterionLovasz, get_criterion
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "tools", "city_semi_lovasz_example.yaml")))
    cfg["net"]["sync_bn"] = False
    cfg["net"]["encoder"]["type"] = "u2pl.models.resnet.resnet50"
    cfg["net"]["encoder"]["kwargs"]["pretrained"] = False
    torch.manual_seed(0)
    model = ModelBuilder(copy.deepcopy(cfg["net"])).to(DEV)
    crit = get_criterion(cfg)
    assert type(crit) is CriterionLovasz
    tr = SupTrainer(cfg, model, crit, steps_per_epoch=4)
    g = torch.Generator().manual_seed(7)
    w0 = tr.arena.flat.clone()
    losses = []
    for _ in range(2):
        img = torch.randn(2, 3, S_NET, S_NET, generator=g).to(DEV)
        lab = torch.randint(0, 19, (2, S_NET, S_NET), generator=g)
        lab[:, :5] = 255
        losses.append(float(tr.train_step(img, lab.to(DEV))[0]))
    torch.cuda.synchronize()
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
    assert not torch.equal(w0, tr.arena.flat)


def test_default_config_makes_no_lovasz_or_sort_call(monkeypatch):
    """the default (ohem) step issues none of the new entry points; the same step under criterion.type lovasz does, which shows
    that the recorder sees them"""
    from u2pl_amd import _lib, configs, hipops as H, nn as K
    from u2pl_amd.models.model_helper import ModelBuilder
    from u2pl_amd.trainer import SemiTrainer
    from u2pl_amd.utils.loss_helper import get_criterion
    monkeypatch.setenv("U2PL_GRAPHS", "0")
    names = {}
    for crit_type in ("ohem", "lovasz"):
        cfg = _lovasz_cfg() if crit_type == "lovasz" else configs.cityscapes_semi(arch="resnet50", crop=S_NET, batch_size=2, sync_bn=False)
        if crit_type == "ohem":
            cfg["criterion"]["kwargs"]["min_kept"] = 1500
        torch.manual_seed(0)
        model, teacher = ModelBuilder(copy.deepcopy(cfg["net"])).to(DEV), ModelBuilder(copy.deepcopy(cfg["net"])).to(DEV)
        tr = SemiTrainer(cfg, model, teacher, get_criterion(cfg), steps_per_epoch=4)
        seen = []
        real = _lib.call

        def rec(name, *args):
            seen.append(name)
            return real(name, *args)
        for mod in (H, K, _lib):
            monkeypatch.setattr(mod, "call", rec)
        g = torch.Generator().manual_seed(5)
        il, iu = torch.randn(2, 3, S_NET, S_NET, generator=g).to(DEV), torch.randn(2, 3, S_NET, S_NET, generator=g).to(DEV)
        ll = torch.randint(0, 19, (2, S_NET, S_NET), generator=g).to(DEV)
        np.random.seed(3)
        tr.train_step(il, ll, iu, epoch=0)
        torch.cuda.synchronize()
        for mod in (H, K, _lib):
            monkeypatch.setattr(mod, "call", real)
        names[crit_type] = seen
    new = [n for n in names["ohem"] if "lovasz" in n or "segsort" in n]
    assert not new and len(names["ohem"]) > 100
    assert "u2pl_ohem_prob_f32" in names["ohem"] and "u2pl_ohem_prob_f32" not in names["lovasz"]
    assert {"u2pl_lovasz_errors_f32", "u2pl_lovasz_sort", "u2pl_lovasz_grad_f32", "u2pl_lovasz_finish_f32",
            "u2pl_lovasz_bwd_f32"} <= set(names["lovasz"])
