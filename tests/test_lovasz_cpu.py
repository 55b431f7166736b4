"""CPU side of the Lovasz-Softmax route (tests/lovasz_bounds.py): the float64 definition against its published-way twin, the
faithful fp32 emulation inside every bound and every faulty emulation outside one, the calibrated constants as ceilings of what
is measured here, and the host-side half of u2pl_amd/csrc/lovasz.hip (workspace, plan, refusals) and of the Python seams
(criterion routing, the ValueErrors) without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import lovasz_bounds as V
from u2pl_amd import _lib

# (family, C, shape, ignore pattern, class mode, class chunk): small shapes for the wide class counts, 2 x 65 x 65 (five tiles,
# the last one partial) where a tile edge matters; chunk sizes 1, C - 1, C, C + 1 and a middle one
GRID = [(f, C, (1, 7, 9), pat, mode, chunk)
        for C, chunk in ((2, 1), (19, 18), (21, 22), (33, 32), (150, 64), (255, 254))
        for f in V.FAMILIES for pat, mode in (("none", "present"), ("some", "all"), ("one", "present"), ("all", "present"))]
GRID += [(f, 19, (2, 65, 65), pat, mode, chunk) for f, pat, mode, chunk in
         (("trained", "some", "present", 19), ("saturated", "some", "all", 7), ("ties", "image", "present", 20),
          ("uniform", "none", "present", 1))]
GRID += [("trained", 5, (1, 1, 1), "none", "present", 5), ("saturated", 19, (3, 23, 31), "some", "present", 6),
         ("ties", 21, (3, 23, 31), "image", "all", 21)]


def _case(f, C, shape, pat):
    z, t = V.make_case(f, C, shape)
    return z, V.apply_ignore(t, pat)


@pytest.mark.parametrize("family", ("trained", "wrong", "offset"))
@pytest.mark.parametrize("C", (2, 19))
@pytest.mark.parametrize("pat", ("none", "some", "one", "all"))
@pytest.mark.parametrize("mode", V.MODES)
def test_definition_equals_published_form_in_float64(family, C, pat, mode):
    """no ties in these families: the closed-form g equals the Jaccard differences, the analytic gradient equals autograd's"""
    z, t = _case(family, C, (2, 7, 9), pat)
    ref = V.lovasz_ref(z, t, mode)
    loss, grad, parts = V.lovasz_torch64(z, t, mode)
    assert abs(ref["loss"] - loss) <= 1e-13
    assert np.abs(ref["grad"] - grad).max() <= 1e-13
    for c, perm, jac in parts:
        assert np.array_equal(perm, ref["perm"][c])
        assert np.abs(ref["g"][c][perm] - jac).max() <= 1e-12
    assert len(parts) == (ref["out3"][2] if ref["nv"] else 0)      # (no valid pixel: the twin has no list to sort; the loss is 0)


def test_closed_form_keeps_the_tail_that_fp32_differences_lose():
    """10^6 background pixels in front of 1000 foreground ones: the fp32 difference of two Jaccard values is a multiple of their
    ulp (2^-24 near 1), the closed form 1000 / ((U - 1) U) ~ 1e-9 is not"""
    n, G = 10 ** 6, 1000
    fgs = np.zeros((1, n), dtype=bool)
    fgs[0, n - G:] = True
    g, Fc, I, U = V.closed_form_g(fgs, np.array([G]))
    J = 1.0 - I / U
    assert np.abs(np.diff(J[0]) - g[0, 1:]).max() <= 1e-15
    J32 = (np.float32(1) - (I.astype(np.float32) / U.astype(np.float32))).astype(np.float32)
    d32 = np.diff(J32[0]).astype(np.float64)
    tail = slice(n // 2, n - G - 1)          # background positions of the second half
    assert (np.abs(d32[tail] - g[0, 1:][tail]) / g[0, 1:][tail]).max() > 0.5
    assert abs(g.sum() - J[0, -1]) <= 1e-12


_FAITHFUL = {}


def _faithful(i):
    if i not in _FAITHFUL:
        f, C, shape, pat, mode, chunk = GRID[i]
        z, t = _case(f, C, shape, pat)
        kw = dict(gout=1.7, gmul=0.4) if i % 2 else {}
        _FAITHFUL[i] = V.lovasz_excess(V.emu_lovasz(z, t, mode, chunk, **kw), z, t, mode, **kw)
    return _FAITHFUL[i]


@pytest.mark.parametrize("i", range(len(GRID)), ids=lambda i: "-".join(str(v) for v in GRID[i]).replace(" ", ""))
def test_faithful_emulation_is_inside_every_bound(i):
    ex = _faithful(i)
    assert max(ex.values()) <= 1.0, ex


@pytest.mark.parametrize("fault", V.FAULTS)
def test_every_fault_leaves_a_bound(fault):
    """each wrong emulation is rejected on at least one case of the grid on which the faithful one passes"""
    order = sorted(range(len(GRID)), key=lambda i: -np.prod(GRID[i][2]))          # tile faults need the large shapes
    for i in order:
        f, C, shape, pat, mode, chunk = GRID[i]
        z, t = _case(f, C, shape, pat)
        kw = dict(gout=1.7, gmul=0.4) if i % 2 else {}
        ex = V.lovasz_excess(V.emu_lovasz(z, t, mode, chunk, fault=fault, **kw), z, t, mode, **kw)
        if max(ex.values()) > 1.0:
            assert max(_faithful(i).values()) <= 1.0
            return
    pytest.fail(f"{fault}: inside every bound on the whole grid")


def test_calibrated_constants_are_ceilings(capsys):
    """re-measures the table of lovasz_bounds' docstring (run with -s to see it) from the emulation and the torch-fp32 form"""
    rows = {k: [] for k in ("g", "sum", "dz")}
    for C in V.CLASSES:
        worst = {k: [0.0, 0.0] for k in rows}
        for fam in V.FAMILIES:
            for n, form in enumerate(("emu", "torch")):
                got = V.measure_case(fam, C, form=form)
                for k in rows:
                    worst[k][n] = max(worst[k][n], got[k])
        for k in rows:
            rows[k].append(worst[k])
        assert max(worst["g"]) <= V.CAL_LV_G * (1 + 1e-6), (C, worst)
        assert max(worst["sum"]) <= V.CAL_LV_SUM, (C, worst)
        assert max(worst["dz"]) <= V.cal_dz(C), (C, worst)
    with capsys.disabled():
        print("\n" + " " * 8 + "".join(f"C = {C:<12d}" for C in V.CLASSES))
        for k, r in rows.items():
            print(f"{k:8s}" + "".join(f"{a:5.2f} / {b:5.2f}   " for a, b in r))


# ---- the host side of csrc/lovasz.hip --------------------------------------------------------------------------------------------
def _plan(P, C, chunk):
    from u2pl_amd import hipops as H
    out = (ctypes.c_longlong * len(H.LOVASZ_PLAN_FIELDS))()
    rc = _lib.lib().u2pl_lovasz_plan(P, C, chunk, out)
    return rc, dict(zip(H.LOVASZ_PLAN_FIELDS, (int(v) for v in out)))


@pytest.mark.parametrize("P", (1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4 * 2048, 4 * 2048 + 1, 2 * 769 * 769, 2 ** 31 - 1))
@pytest.mark.parametrize("C,chunk", ((2, 1), (2, 2), (19, 1), (19, 18), (19, 19), (19, 20), (19, 32), (150, 32), (255, 64), (255, 255)))
def test_workspace_and_plan_match_the_restatement(P, C, chunk):
    L = _lib.lib()
    rc, got = _plan(P, C, chunk)
    ref = V.plan_ref(P, C, chunk)
    assert rc == 0 and got == ref
    assert L.u2pl_lovasz_workspace_bytes(P, C, chunk) == ref["total"]
    assert L.u2pl_segsort_ws_bytes(ref["cap"], P) == V.segsort_ws_bytes(ref["cap"], P)
    assert got["chunks"] * got["cap"] >= C > (got["chunks"] - 1) * got["cap"]


def test_constants_of_the_restatement():
    L = _lib.lib()
    assert L.u2pl_segsort_tile() == V.TILE and L.u2pl_lovasz_default_chunk() == V.DEFAULT_CHUNK
    assert [L.u2pl_segsort_passes(b) for b in (0, 1, 8, 9, 30, 32, 33)] == [0, 1, 1, 2, 4, 4, 0]


def test_refusals_need_no_gpu():
    """1001 before any HIP call: the pointers below are never dereferenced"""
    L = _lib.lib()
    p = 4096          # any non-null value
    out = (ctypes.c_longlong * 20)()
    for P, C, chunk in ((0, 19, 4), (-5, 19, 4), (2 ** 31, 19, 4), (100, 1, 4), (100, 256, 4), (100, 19, 0), (100, 19, -1)):
        assert L.u2pl_lovasz_plan(P, C, chunk, out) == 1001
        assert L.u2pl_lovasz_workspace_bytes(P, C, chunk) == 0
        assert L.u2pl_lovasz_sort(P, C, 0, p, chunk, None) == 1001
        assert L.u2pl_lovasz_grad_f32(P, C, 0, 1, p, chunk, p, None) == 1001
        assert L.u2pl_lovasz_finish_f32(P, C, 1, p, chunk, p, None) == 1001
    assert L.u2pl_lovasz_plan(100, 19, 4, None) == 1001
    for N, C, H, W, c0, chunk in ((0, 19, 5, 5, 0, 4), (1, 19, 0, 5, 0, 4), (1, 1, 5, 5, 0, 4), (1, 256, 5, 5, 0, 4), (1, 19, 5, 5, 0, 0),
                                  (1, 19, 5, 5, 19, 4), (1, 19, 5, 5, -4, 4), (1, 19, 5, 5, 3, 4), (32768, 19, 256, 256, 0, 4)):
        assert L.u2pl_lovasz_errors_f32(p, p, 255, N, C, H, W, c0, p, chunk, None) == 1001
        if c0 == 0 and chunk > 0:
            assert L.u2pl_lovasz_bwd_f32(p, p, 255, N, C, H, W, p, p, None, 1.0, p, None) == 1001
    for args in ((None, p, 255, 1, 19, 5, 5, 0, p, 4), (p, None, 255, 1, 19, 5, 5, 0, p, 4), (p, p, 255, 1, 19, 5, 5, 0, None, 4)):
        assert L.u2pl_lovasz_errors_f32(*args, None) == 1001
    assert L.u2pl_lovasz_sort(25, 19, 0, None, 4, None) == 1001
    assert L.u2pl_lovasz_grad_f32(25, 19, 0, 1, None, 4, p, None) == 1001 and L.u2pl_lovasz_grad_f32(25, 19, 0, 1, p, 4, None, None) == 1001
    assert L.u2pl_lovasz_finish_f32(25, 19, 1, None, 4, p, None) == 1001 and L.u2pl_lovasz_finish_f32(25, 19, 1, p, 4, None, None) == 1001
    for k in range(5):
        args = [p, p, 255, 1, 19, 5, 5, p, p, None, 1.0, p]
        args[(0, 1, 7, 8, 11)[k]] = None
        assert L.u2pl_lovasz_bwd_f32(*args, None) == 1001
    for k in range(5):
        args = [p, p, p, p, p, 3, 100, None, 30]
        args[k] = None
        assert L.u2pl_segsort_u32(*args, None) == 1001
    for nseg, n, bits in ((0, 100, 30), (65536, 100, 30), (3, 0, 30), (3, 2 ** 31, 30), (3, 100, 0), (3, 100, 33)):
        assert L.u2pl_segsort_u32(p, p, p, p, p, nseg, n, None, bits, None) == 1001
    assert L.u2pl_segsort_ws_bytes(0, 100) == 0 and L.u2pl_segsort_ws_bytes(3, 2 ** 31) == 0


# ---- the Python seams ------------------------------------------------------------------------------------------------------------
def _cfg(ctype, kwargs=None, aux=True):
    from u2pl_amd import configs
    cfg = configs.cityscapes_semi(arch="resnet50", crop=65, batch_size=2, sync_bn=False)
    cfg["criterion"] = dict(type=ctype, kwargs=kwargs or {})
    if not aux:
        cfg["net"].pop("aux_loss", None)
    return cfg


def test_get_criterion_routing():
    from u2pl_amd.utils import loss_helper as LH
    from u2pl_amd import configs
    c = LH.get_criterion(_cfg("lovasz", dict(ce_weight=0.5, lovasz_weight=2.0, classes="all")))
    assert type(c) is LH.CriterionLovasz and (c.ce_weight, c.lovasz_weight, c.classes) == (0.5, 2.0, "all")
    assert c._aux_weight == 0.4 and c._ignore_index == 255
    assert LH.get_criterion(_cfg("lovasz", aux=False))._aux_weight == 0
    d = LH.get_criterion(_cfg("lovasz"))
    assert (d.ce_weight, d.lovasz_weight, d.classes) == (1.0, 1.0, "present")
    # every other type builds what it built before
    assert type(LH.get_criterion(configs.cityscapes_semi(arch="resnet50", crop=65, batch_size=2, sync_bn=False))) is LH.CriterionOhem
    assert type(LH.get_criterion(_cfg("CELoss", dict(use_weight=False)))) is LH.Criterion
    assert type(LH.get_criterion(_cfg("anything_else"))) is LH.Criterion


def test_unsupported_modes_are_refused_by_name():
    from u2pl_amd import hipops as H
    from u2pl_amd.utils import loss_helper as LH
    z, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="per_image"):
        H.lovasz_softmax(z, t, per_image=True)
    for bad in ("each", [0, 1], None, ("present",)):
        with pytest.raises(ValueError, match="classes"):
            H.lovasz_softmax(z, t, classes=bad)
    with pytest.raises(ValueError, match="2 <= C"):
        H.lovasz_softmax(torch.zeros(1, 1, 4, 4), t)
    with pytest.raises(ValueError, match="class_chunk"):
        H.lovasz_softmax(z, t, class_chunk=0)
    with pytest.raises(_lib.HipError):                       # no CPU fallback
        H.lovasz_softmax(z, t)
    with pytest.raises(ValueError, match="per_image"):
        LH.get_criterion(_cfg("lovasz", dict(per_image=True)))
    with pytest.raises(ValueError, match="classes"):
        LH.get_criterion(_cfg("lovasz", dict(classes=[1, 2])))
    with pytest.raises(ValueError, match="use_weight"):
        LH.get_criterion(_cfg("lovasz", dict(use_weight=True)))
    with pytest.raises(ValueError, match="both 0"):
        LH.get_criterion(_cfg("lovasz", dict(ce_weight=0, lovasz_weight=0)))
    with pytest.raises(TypeError):                           # no OHEM combination: its arguments do not exist here
        LH.get_criterion(_cfg("lovasz", dict(thresh=0.7, min_kept=1000)))


def test_example_config_parses_and_routes():
    import os
    import yaml
    from u2pl_amd.utils import loss_helper as LH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "tools", "city_semi_lovasz_example.yaml")))
    assert cfg["criterion"] == dict(type="lovasz", kwargs=dict(ce_weight=1.0, lovasz_weight=1.0, classes="present"))
    assert type(LH.get_criterion(cfg)) is LH.CriterionLovasz
    base = yaml.safe_load(open(os.path.join(root, "tools", "city_semi_template.yaml")))
    cfg["criterion"] = base["criterion"]
    assert cfg == base                          # the template with the criterion swapped, nothing else
