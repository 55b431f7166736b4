"""The batched rebuild of the split-fp16 weight operands (operands.presplit -> u2pl_weight_rebuild2h_f32: Winograd planes recomputed
from the nine taps, max |w| once per weight) against the per-weight lazy path (u2pl_wino_weight_f32 / u2pl_weight_transpose_f32 +
u2pl_weight_split2h_f32): every byte of every derived buffer -- planes, padding rows, the maxima and the 16-byte-rounded tail --
with torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


@pytest.fixture
def Kn():
    from u2pl_amd import nn as K
    saved = (dict(K.CONV_ALGO), dict(K.CONV_WS), dict(K.CONV_H), K.PRESPLIT["on"])
    K.CONV_H["on"] = True
    K.CONV_WS["on"] = True
    K.CONV_ALGO.update(wino=4, min_gain=0.0)
    yield K
    K.CONV_ALGO.update(saved[0])
    K.CONV_WS.update(saved[1])
    K.CONV_H.update(saved[2])
    K.PRESPLIT["on"] = saved[3]


def _operand(K, w, op):
    if op == "f":
        return K.ws_forward(w, True)
    if op == "d":
        return K.ws_dgrad(w, True)
    how, mt = op[:2], int(op[2])
    return K.ws_wino(w, how == "wd", mt, True)


def _kind(op):
    return op + "h"


def _lazy_vs_rebuild(K, convs, ops, mutate):
    """ops: [(conv index, "f" | "d" | "wf4" | "wd4" | "wf2" | "wd2")] in registration order.  Registers the operands lazily, changes the
    weights with mutate(convs), rebuilds each operand by the lazy path, then all of them by presplit -> (arena, launches, lazy
    buffers, rebuilt buffers)"""
    from u2pl_amd._lib import query
    arena = K.ParamArena([[p for c in convs for p in c.parameters()]])
    K.PRESPLIT["on"] = False
    for i, op in ops:
        _operand(K, convs[i].weight, op)
    with torch.no_grad():
        mutate(convs)
    K.invalidate_weights(arena)
    lazy = {(i, op): _operand(K, convs[i].weight, op).clone() for i, op in ops}
    torch.cuda.synchronize()
    for i, op in ops:
        convs[i].weight._u2pl_derived[_kind(op)]["buf"].fill_(0xA5)         # (every byte must be rewritten)
    K.PRESPLIT["on"] = True
    K.invalidate_weights(arena)
    k0 = query("u2pl_kernel_launches")
    n = K.presplit(arena.params, arena)
    launches = query("u2pl_kernel_launches") - k0
    torch.cuda.synchronize()
    assert n == len(ops)
    new = {(i, op): convs[i].weight._u2pl_derived[_kind(op)]["buf"] for i, op in ops}
    return arena, launches, lazy, new


def _convs(K, shapes):
    return [K.Conv2d(ci, co, k, padding=d * (k // 2), dilation=d, bias=False).to(DEV) for co, ci, k, d in shapes]


def _sgd_like(convs):
    g = torch.Generator(device=DEV).manual_seed(5)
    for c in convs:
        c.weight.add_(torch.randn(c.weight.shape, device=DEV, generator=g).contiguous(memory_format=CL) * 0.05)


# O, C, k, dilation: rows / K below, at and above the pad granularity of the planes (<= 128 -> 128, else multiples of 256)
SHAPES = [(96, 32, 3, 1), (160, 64, 3, 1), (128, 128, 3, 2), (288, 96, 3, 1), (512, 256, 1, 1), (96, 32, 1, 1), (128, 64, 1, 1)]
ALL_OPS = {0: ["f", "d", "wf4", "wd4", "wf2"], 1: ["f", "d", "wf4", "wd4"], 2: ["f", "d", "wf2", "wd2", "wf4"], 3: ["f", "d", "wf4", "wd4"],
           4: ["f", "d"], 5: ["f", "d"], 6: ["f", "d"]}


@pytest.mark.parametrize("order", ["wino_last", "wino_first", "interleaved"])
def test_rebuild_writes_the_lazy_paths_bytes(Kn, order):
    """forward / transposed / Winograd (mt = 4 and 2, both orientations, one dilated layer) operands of seven weights in one table:
    jobs of 512 segments that share a block span with their neighbours (the 1x1 96 <- 32 and 128 <- 64 layers), jobs of many spans
    (288 <- 96: 55296 segments, 6144 Winograd units), rows of 32 .. 512 (padded to 128 / 256 / 512), K of one chunk (32) and more"""
    torch.manual_seed(3)
    convs = _convs(Kn, SHAPES)
    ops = [(i, op) for i in range(len(SHAPES)) for op in ALL_OPS[i]]
    if order == "wino_first":
        ops.sort(key=lambda t: not t[1].startswith("w"))
    elif order == "wino_last":
        ops.sort(key=lambda t: t[1].startswith("w"))
    arena, launches, lazy, new = _lazy_vs_rebuild(Kn, convs, ops, _sgd_like)
    # clear, maxima of every kind, pieces of the plain / transposed operands, pieces of the Winograd operands
    assert launches == 4
    for key, b in lazy.items():
        assert torch.equal(new[key], b), key
    assert "scratch" not in Kn.PRESPLIT["tables"][id(arena)]         # no fp32 Winograd-domain filters in memory


def test_rebuild_without_winograd_operands_is_three_launches(Kn):
    torch.manual_seed(4)
    convs = _convs(Kn, [SHAPES[4], SHAPES[5], SHAPES[0]])
    ops = [(0, "f"), (0, "d"), (1, "d"), (1, "f"), (2, "d")]          # (a weight whose only operand is the transposed one, too)
    arena, launches, lazy, new = _lazy_vs_rebuild(Kn, convs, ops, _sgd_like)
    assert launches <= 3
    for key, b in lazy.items():
        assert torch.equal(new[key], b), key
    tab = Kn.PRESPLIT["tables"][id(arena)]
    assert "scratch" not in tab and tab["n_wino"] == 0


def _tail_words(K, w, op):
    from u2pl_amd._lib import query
    e = w._u2pl_derived[_kind(op)]
    sp = e["spec"]
    nb = query("u2pl_weight_split2h_bytes", sp["rows"], sp["K"], sp["batch"])
    planes = nb - ((sp["batch"] * 4 + 15) & ~15)
    return e["buf"][planes:planes + 4 * sp["batch"]].view(torch.int32)


def _set_first(convs):
    for c in convs:
        c.weight.mul_(0.1)
        c.weight[0, 0, 0, 0] = 7.5


def _set_last(convs):
    for c in convs:
        c.weight.mul_(0.1)
        c.weight[-1, -1, 2, 2] = 9.25


def _set_zero(convs):
    for c in convs:
        c.weight.zero_()


def _set_negative(convs):
    for c in convs:
        c.weight.copy_(-c.weight.abs() - 0.01)
        c.weight[c.weight.shape[0] // 2, 3, 1, 1] = -11.0


def _set_nonfinite(convs):
    # (separate filters: the components of a filter then see ONE non-finite source and no NaN meets another NaN's payload)
    for c in convs:
        c.weight[1, 2, 0, 1] = float("nan")
        c.weight[c.weight.shape[0] - 2, 5, 2, 0] = float("inf")


@pytest.mark.parametrize("mutate", [_set_first, _set_last, _set_zero, _set_negative, _set_nonfinite], ids=lambda f: f.__name__[5:])
def test_maxima_edge_cases(Kn, mutate):
    """per component and per weight: the largest value in the first / the last filter, an all-zero weight, a negative maximum, one
    NaN and one Inf tap (NaN sorts above everything: bit patterns of |w|) -- buffers and maxima equal the lazy path's, and the
    forward and transposed planes of one weight carry the same maximum word"""
    torch.manual_seed(6)
    convs = _convs(Kn, [(160, 64, 3, 1), (96, 32, 3, 1)])
    ops = [(i, op) for i in range(2) for op in ("f", "d", "wf4", "wd4", "wf2", "wd2")]
    arena, launches, lazy, new = _lazy_vs_rebuild(Kn, convs, ops, mutate)
    assert launches == 4
    for key, b in lazy.items():
        assert torch.equal(new[key], b), key
    for i, c in enumerate(convs):
        f, d = _tail_words(Kn, c.weight, "f"), _tail_words(Kn, c.weight, "d")
        assert torch.equal(f, d)
        want = c.weight.detach().abs().reshape(-1).view(torch.int32).max()          # (bit patterns: NaN above Inf above finite)
        assert int(f[0]) == int(want), (i, int(f[0]), int(want))
        if mutate is _set_zero:
            assert int(_tail_words(Kn, c.weight, "wf4").abs().max()) == 0


def test_step_equal_with_presplit_on_and_off(Kn):
    """forward + backward through a four-layer stack (1x1, dilated 3x3 on the Winograd route, strided 3x3, 1x1 with bias): the same
    outputs and input gradients from operands rebuilt lazily and from operands rebuilt by presplit behind the optimizer step.
    (No graph-replay variant here: capturing and instantiating a graph of this stack costs more than the second such a variant may
    take; tests/test_gpu_graphs.py::test_graph_replay_steps_are_bit_identical_to_eager_steps replays the captured segments of whole
    training steps, each behind the presplit() of its optimizer and EMA updates, and compares them with eager steps.)"""
    torch.manual_seed(21)
    convs = [Kn.Conv2d(128, 256, 1, bias=False).to(DEV), Kn.Conv2d(256, 128, 3, padding=2, dilation=2, bias=False).to(DEV),
             Kn.Conv2d(128, 160, 3, stride=2, padding=1, bias=False).to(DEV), Kn.Conv2d(160, 96, 1, bias=True).to(DEV)]
    arena = Kn.ParamArena([[p for c in convs for p in c.parameters()]])
    x = torch.randn(2, 128, 21, 19, device=DEV).contiguous(memory_format=CL)

    def step():
        h = x.clone().requires_grad_(True)
        y = h
        for c in convs:
            y = c(y)
        y.square().mean().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), h.grad.clone()

    Kn.PRESPLIT["on"] = False
    step()
    w0, g0 = arena.flat.clone(), None
    out = {}
    for on in (False, True):
        Kn.PRESPLIT["on"] = on
        arena.flat.copy_(w0)
        arena.momentum_buf = None
        arena.grad.copy_(g0) if g0 is not None else arena.grad.normal_(0, 1.0)
        g0 = arena.grad.clone() if g0 is None else g0
        Kn.invalidate_weights(arena)
        arena.sgd_step([0.05], 0.9, 1e-4)
        out[on] = step()
    assert any("wf4h" in c.weight._u2pl_derived for c in convs)
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert "scratch" not in Kn.PRESPLIT["tables"][id(arena)]


def test_one_weight_call_back_to_back(Kn):
    """u2pl_weight_split2h_f32 passes its job record in the kernel arguments: two calls in a row (no
    synchronisation, other host work in between) write what each call writes alone"""
    from u2pl_amd._lib import call, query
    torch.manual_seed(8)
    wa, wb = torch.randn(96, 64, device=DEV), torch.randn(3, 160, 32, device=DEV) * 3.0
    na, nb = query("u2pl_weight_split2h_bytes", 96, 64, 1), query("u2pl_weight_split2h_bytes", 160, 32, 3)

    def run(sync):
        a = torch.full((na,), 0xA5, dtype=torch.uint8, device=DEV)
        b = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        call("u2pl_weight_split2h_f32", wa, 96 * 64, 96, 64, 1, a)
        if sync:
            torch.cuda.synchronize()
        sorted(range(1000), key=lambda v: -v)          # (host work: whatever lay on the stack during the first call is gone)
        call("u2pl_weight_split2h_f32", wb, 160 * 32, 160, 32, 3, b)
        torch.cuda.synchronize()
        return a, b

    a0, b0 = run(True)
    a1, b1 = run(False)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    assert int(a0[na - 16:na - 12].view(torch.int32)) == int(wa.abs().view(torch.int32).max())
    for z in range(3):
        assert int(b0[nb - 16 + 4 * z:nb - 12 + 4 * z].view(torch.int32)) == int(wb[z].abs().view(torch.int32).max())
    assert int(b0[nb - 4:].view(torch.int32)) == 0
