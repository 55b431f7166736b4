"""Every Winograd transform kernel of u2pl_amd/csrc/wino.hip on its own, through the C ABI, against the float64 reference and the
per-stage bound of tests/wino_stage_ref.py (the bound's derivation and the shape lists live there; tests/test_wino_stages_cpu.py
shows that the bound rejects a transform that is merely sloppy).  Every output buffer is pre-filled with 0xA5 bytes, so "every
element written" and "nothing else written" are both asserted; sources are pitched with NaN in the gap and behind the last pixel.
The batched GEMMs between the stages are held by test_gpu_split_bounds.py / test_gpu_igemm_ws.py, the plane formats by
test_gpu_weight_planes.py / test_gpu_presplit_taps.py.  Each test prints its largest excess (pytest -s)."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_bounds as BB  # noqa: E402
import wino_stage_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
MARGIN = 64             # sentinel floats behind every output buffer
EINVAL = "code 1001"


def _call(name, *args):
    from u2pl_amd._lib import call
    call(name, *args)


def _query(name, *args):
    from u2pl_amd._lib import query
    return query(name, *args)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def _sentinel(n):
    """n + MARGIN floats of 0xA5 bytes"""
    return torch.full(((n + MARGIN) * 4,), R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV).view(torch.float32)


def _take(buf, shape):
    """the first prod(shape) floats of a _sentinel buffer as numpy; the margin behind them must be untouched"""
    torch.cuda.synchronize()
    n = int(np.prod(shape))
    tail = buf[n:].cpu().numpy().view(np.uint32)
    assert (tail == 0xA5A5A5A5).all(), "wrote behind the buffer"
    return buf[:n].cpu().numpy().reshape(shape)


def _pitched(a, ld, behind=3):
    """a [M][C] -> device [M + behind][ld]: NaN in the gap and in the rows of the `neighbouring tensor` behind the last row"""
    M, C = a.shape
    b = np.full((M + behind, ld), np.nan, dtype=F32)
    b[:M, :C] = a
    return _dev(b)


def _amax_obj(fill=0.0):
    return torch.full((_query("u2pl_amax_words"),), fill, dtype=torch.float32, device=DEV)


def _amax_value(obj):
    torch.cuda.synchronize()
    return obj.view(torch.int32).max().view(torch.float32).cpu().numpy()[()]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _report(stage, e):
    print("excess %s %.3f" % (stage, e))
    assert e <= 1.0, (stage, e)


# ---- input and gy transforms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["input", "gy"])
@pytest.mark.parametrize("mt", R.MTS)
@pytest.mark.parametrize("case", R.GEOMS, ids=lambda c: "x".join(map(str, c)))
def test_input_and_gy_transform(case, mt, stage):
    N, H, W, C, dil = case
    a2 = (mt + 2) ** 2
    tiles = _query("u2pl_wino_tiles", N, H, W, dil, mt)
    assert tiles == R.geom(N, H, W, dil, mt)[2]
    ref_fn = R.ref_input if stage == "input" else R.ref_gy
    worst = 0.0
    for ki, kind in enumerate(R.KINDS):
        src = R.rows(kind, N * H * W, C, 17 * ki + mt)
        ref, bound = ref_fn(src, N, H, W, C, dil, mt)
        if dil > H:         # phases without a real pixel: their tiles are zero, and so is their bound
            assert (bound.reshape(a2, N, dil, dil, -1)[:, :, H:] == 0).all()
        for ld in (C, C + 4, C + 12):
            x = _pitched(src, ld)
            V = _sentinel(a2 * tiles * C)
            _call("u2pl_wino_%s_f32" % stage, x, ld, N, H, W, C, dil, mt, V)
            got = _take(V, (a2, tiles, C))
            worst = max(worst, R.stage_excess(got, ref, bound))
            for run in range(2):            # the fused maximum: the plain form's bits, the exact maximum, twice the same
                V2, obj = _sentinel(a2 * tiles * C), _amax_obj()
                _call("u2pl_wino_%s_amax_f32" % stage, x, ld, N, H, W, C, dil, mt, V2, obj)
                assert _same_bits(_take(V2, (a2, tiles, C)), got), (kind, ld, run)
                assert _amax_value(obj) == np.abs(got).max(), (kind, ld, run)
    _report("%s F(%dx%d)" % (stage, mt, mt), worst)
    # one NaN inside the slice (the last pixel's last channel: the element the surplus lanes redo) makes the maximum NaN
    src = R.rows(R.KINDS[0], N * H * W, C, 3)
    src[-1, -1] = np.nan
    V2, obj = _sentinel(a2 * tiles * C), _amax_obj()
    _call("u2pl_wino_%s_amax_f32" % stage, _pitched(src, C + 4), C + 4, N, H, W, C, dil, mt, V2, obj)
    assert np.isnan(_amax_value(obj))


# ---- filter transform ---------------------------------------------------------------------------------------------------------------
def _weight_call(w, O, C, transposed, mt):
    a2 = (mt + 2) ** 2
    U = _sentinel(a2 * O * C)
    _call("u2pl_wino_weight_f32", w, O, C, transposed, mt, U)
    return _take(U, (a2, C, O) if transposed else (a2, O, C))


@pytest.mark.parametrize("mt", R.MTS)
@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("O,C", R.WEIGHT_SHAPES)
def test_filter_transform(O, C, transposed, mt):
    w = R.weights((O, 3, 3, C), 5 + O)
    ref, bound = R.ref_weight(w, transposed, mt)
    got = _weight_call(_dev(w), O, C, transposed, mt)
    _report("filter F(%dx%d)" % (mt, mt), R.stage_excess(got, ref, bound))
    assert _same_bits(got, R.emu_weight(w, transposed, mt))      # no contraction: the emulation's operations ARE the kernel's


def _multi(jobs, ws):
    """jobs: (O, C, transposed, mt); ws: device weights -> the U buffers u2pl_wino_weight_multi_f32 writes (sentinel-filled).
    Record layout of include/u2pl_hip.h: { const float* w; float* U; long begin; int O, C, transposed, mt; }, 40 bytes"""
    Us, recs, begin = [], b"", 0
    for (O, C, tr, mt), w in zip(jobs, ws):
        Us.append(_sentinel((mt + 2) ** 2 * O * C))
        recs += struct.pack("<QQqiiii", w.data_ptr(), Us[-1].data_ptr(), begin, O, C, tr, mt)
        begin += O * C
    assert len(recs) == 40 * len(jobs)
    table = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(DEV)
    _call("u2pl_wino_weight_multi_f32", table, len(jobs), begin)
    torch.cuda.synchronize()
    return Us, begin


def test_filter_transform_multi_writes_the_per_weight_bytes():
    jobs = [(96, 32, 0, 4), (12, 20, 1, 2), (1, 1, 0, 4), (5, 300, 1, 4), (4, 4, 0, 2), (12, 20, 1, 4)]      # a one-pair job in the middle
    ws = [_dev(R.weights((O, 3, 3, C), 31 + i)) for i, (O, C, _, _) in enumerate(jobs)]
    Us, _ = _multi(jobs, ws)
    for (O, C, tr, mt), w, U in zip(jobs, ws, Us):
        shape = ((mt + 2) ** 2, C, O) if tr else ((mt + 2) ** 2, O, C)
        assert _same_bits(_take(U, shape), _weight_call(w, O, C, tr, mt)), (O, C, tr, mt)


def test_filter_transform_multi_across_the_first_grid_stride():
    """total just above 4096 * 256 pairs: the pairs behind the grid take the second trip of the grid-stride loop"""
    jobs = [(1024, 1024, 0, 2), (1, 1, 1, 2), (12, 20, 0, 2)]
    g = torch.Generator().manual_seed(7)
    ws = [torch.randn(O, 3, 3, C, generator=g).to(DEV) for O, C, _, _ in jobs]
    Us, total = _multi(jobs, ws)
    assert total > 4096 * 256
    for (O, C, tr, mt), w, U in zip(jobs, ws, Us):
        one = _sentinel(16 * O * C)
        _call("u2pl_wino_weight_f32", w, O, C, tr, mt, one)
        torch.cuda.synchronize()
        assert torch.equal(U.view(torch.int32), one.view(torch.int32)), (O, C)          # (margins included)
        del one


# ---- output transform -------------------------------------------------------------------------------------------------------------
def _y_buffer(N, H, W, O, ldy):
    """-> sentinel buffer of N H W + 2 rows, and the mask of what the kernel may write"""
    rows_ = N * H * W + 2
    written = np.zeros((rows_, ldy), dtype=bool)
    written[:N * H * W, :O] = True
    return _sentinel(rows_ * ldy), written


def _pad_ref(ref, bound, written):
    r, b = np.zeros(written.shape), np.zeros(written.shape)
    r[written], b[written] = ref.reshape(-1), bound.reshape(-1)
    return r, b


@pytest.mark.parametrize("mt", R.MTS)
@pytest.mark.parametrize("case", R.GEOMS, ids=lambda c: "x".join(map(str, c)))
def test_output_transform(case, mt):
    N, H, W, O, dil = case
    a2, tiles, M = (mt + 2) ** 2, R.geom(N, H, W, dil, mt)[2], N * H * W
    rng = np.random.default_rng(11)
    bias = rng.standard_normal(O).astype(F32)
    bn = [v.astype(F32) for v in (rng.standard_normal(O), 0.5 + rng.random(O), rng.standard_normal(O), 50.0 * rng.standard_normal(O))]
    res = rng.standard_normal((M, O)).astype(F32)
    d_bias, d_bn, d_res = _dev(bias), [_dev(v) for v in bn], _pitched(res, O + 4)
    worst = {"plain": 0.0, "bias": 0.0, "bn": 0.0}
    for ki, kind in enumerate(R.KINDS):
        Mb = R.rows(kind, a2 * tiles, O, 23 * ki + mt).reshape(a2, tiles, O)
        d_Mb = _dev(Mb)
        # plain and with a bias; dense and pitched y: the sentinel survives in the gap and behind the last pixel
        for mode, b_np, b_dev, ldy in (("plain", None, None, O), ("bias", bias, d_bias, O + 8)):
            y, written = _y_buffer(N, H, W, O, ldy)
            _call("u2pl_wino_output_f32", d_Mb, N, H, W, O, dil, mt, b_dev, y, ldy, None, None)
            ref, bound = _pad_ref(*R.ref_output(Mb, N, H, W, O, dil, mt, bias=b_np), written)
            worst[mode] = max(worst[mode], R.stage_excess(_take(y, written.shape), ref, bound, written))
        # eval BatchNorm epilogue, pitched residual (NaN in its gap), ReLU off and on; the _amax form: same bits, exact maximum
        for relu in (0, 1):
            for with_res in (False, True):
                ldy = O + 8
                y, written = _y_buffer(N, H, W, O, ldy)
                r_dev, r_np = (d_res, res) if with_res else (None, None)
                _call("u2pl_wino_output_bnact_f32", d_Mb, N, H, W, O, dil, mt, d_bias, y, ldy, *d_bn, r_dev, O + 4, relu)
                got = _take(y, written.shape)
                ref, bound = _pad_ref(*R.ref_output(Mb, N, H, W, O, dil, mt, bias=bias, bn=bn, res=r_np, relu=relu), written)
                worst["bn"] = max(worst["bn"], R.stage_excess(got, ref, bound, written))
                for run in range(2):
                    y2, obj = _y_buffer(N, H, W, O, ldy)[0], _amax_obj()
                    _call("u2pl_wino_output_bnact_amax_f32", d_Mb, N, H, W, O, dil, mt, d_bias, y2, ldy, *d_bn, r_dev, O + 4, relu, obj)
                    assert _same_bits(_take(y2, written.shape), got), (kind, relu, with_res, run)
                    assert _amax_value(obj) == np.abs(got[written]).max(), (kind, relu, with_res, run)
    for mode, e in worst.items():
        _report("output F(%dx%d) %s" % (mt, mt, mode), e)


@pytest.mark.parametrize("pivot_on", [False, True])
@pytest.mark.parametrize("case", R.STAT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_output_transform_statistics(case, pivot_on):
    N, H, W, O, dil, mt = case
    a2, tiles, M = (mt + 2) ** 2, R.geom(N, H, W, dil, mt)[2], N * H * W
    Mb = R.rows("relu_heavy_tail", a2 * tiles, O, 41 + O).reshape(a2, tiles, O)
    rng = np.random.default_rng(12)
    bias, pivot = rng.standard_normal(O).astype(F32), (rng.standard_normal(O).astype(F32) if pivot_on else None)
    d_Mb, d_bias, d_pivot = _dev(Mb), _dev(bias), (_dev(pivot) if pivot_on else None)
    nblk = _query("u2pl_wino_stat_blocks", tiles, O)
    assert nblk == -(-tiles // BB.wino_tpb(O))
    y0, written = _y_buffer(N, H, W, O, O)
    _call("u2pl_wino_output_f32", d_Mb, N, H, W, O, dil, mt, d_bias, y0, O, None, None)
    y0 = _take(y0, written.shape)
    y1, part = _y_buffer(N, H, W, O, O)[0], _sentinel(nblk * 2 * O)
    _call("u2pl_wino_output_f32", d_Mb, N, H, W, O, dil, mt, d_bias, y1, O, part, d_pivot)
    assert _same_bits(_take(y1, written.shape), y0)                 # the statistics change nothing in y
    ref, bound = R.ref_stats(y0[:M], pivot, N, H, W, O, dil, mt, BB.L_wino(mt, O))
    _report("statistics", R.stage_excess(_take(part, (nblk, 2, O)), ref, bound))


# ---- weight-gradient finish -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", R.MTS)
@pytest.mark.parametrize("nsplit", R.NSPLITS)
@pytest.mark.parametrize("O,C", R.FINISH_SHAPES)
def test_wgrad_finish(O, C, nsplit, mt):
    a2, n = (mt + 2) ** 2, O * 9 * C
    part = R.rows("relu_heavy_tail", nsplit * O * a2, C, 5 + nsplit).reshape(nsplit, O, a2, C)
    part = part * np.where(np.random.default_rng(8).random(part.shape) < 0.5, F32(-1), F32(1))
    dw0 = R.weights((O, 3, 3, C), 9) * F32(100)
    d_part = _dev(part)
    worst = 0.0
    for accumulate in (0, 1):
        ref, bound = R.ref_finish(part, mt, dw0 if accumulate else None)
        for lead in (4, 5):             # dw inside a larger arena: 16-byte aligned, and 4 bytes past it (the scalar branch)
            arena = _sentinel(lead + n)
            dw = arena[lead:lead + n]
            assert dw.data_ptr() % 16 == (0 if lead == 4 else 4)
            if accumulate:
                dw.copy_(_dev(dw0).reshape(-1))
            _call("u2pl_wino_wgrad_finish_f32", d_part, nsplit, O, C, mt, accumulate, dw)
            got = _take(arena, (lead + n,))
            assert (got[:lead].view(np.uint32) == 0xA5A5A5A5).all(), "wrote in front of dw"
            worst = max(worst, R.stage_excess(got[lead:].reshape(O, 3, 3, C), ref, bound))
    _report("finish F(%dx%d)" % (mt, mt), worst)


# ---- the stand-alone maximum ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,ld", [(3, 8, 8), (4099, 1024, 1024), (37, 20, 24)],
                         ids=["below-one-wave", "first-grid-stride", "pitched-nan-gap"])
def test_absmax_is_exact(M, C, ld):
    assert (M * C // 4 < 64) if M == 3 else (M * C // 4 > 2048 * 512) if M == 4099 else ld > C
    a = np.random.default_rng(M).standard_normal((M, C)).astype(F32)
    a[-1, -1] = -7.5                    # the largest magnitude: negative, in the last element (the grid-stride loop's last trip)
    x = _pitched(a, ld, behind=1)
    obj = _amax_obj(fill=123.0)         # clear = 1 zeroes a dirty object first
    _call("u2pl_absmax_f32", x, ld, M, C, obj, 1)
    assert _amax_value(obj) == 7.5
    obj = _amax_obj()                   # clear = 0: the caller's zeroed object
    _call("u2pl_absmax_f32", x, ld, M, C, obj, 0)
    assert _amax_value(obj) == 7.5
    obj = _amax_obj(fill=9.0)           # clear = 0 leaves what the object holds: the maximum of both
    _call("u2pl_absmax_f32", x, ld, M, C, obj, 0)
    assert _amax_value(obj) == 9.0
    a[M // 2, C - 1] = np.nan
    obj = _amax_obj()
    _call("u2pl_absmax_f32", _pitched(a, ld, behind=1), ld, M, C, obj, 1)
    assert np.isnan(_amax_value(obj))


# ---- refusals: U2PL_EINVAL before any launch (the buffers would hold the largest reading of each call all the same) ---------------
def test_refusals():
    from u2pl_amd._lib import HipError
    N, H, W, C = 1, 4, 4, 8
    x, V, obj = _dev(np.zeros((N * H * W, 16))), _sentinel(36 * 4 * 16), _amax_obj()
    y, part, vec = _sentinel(N * H * W * 16), _sentinel(4 * 2 * 2048), _dev(np.ones(2048))
    Mb = _dev(np.zeros(36 * 4 * 1028))

    def refused(name, *args):
        with pytest.raises(HipError, match=EINVAL):
            _call(name, *args)

    for stage in ("input", "gy"):
        refused("u2pl_wino_%s_f32" % stage, x, 8, N, H, W, C, 1, 3, V)                  # mt = 3
        refused("u2pl_wino_%s_f32" % stage, x, 8, N, H, W, 6, 1, 4, V)                  # C % 4 != 0
        refused("u2pl_wino_%s_f32" % stage, x, 8, N, H, W, C, 0, 4, V)                  # dil = 0
        refused("u2pl_wino_%s_f32" % stage, x, 10, N, H, W, C, 1, 4, V)                 # pitch % 4 != 0
        refused("u2pl_wino_%s_amax_f32" % stage, x, 9, N, H, W, C, 1, 2, V, obj)
    refused("u2pl_wino_weight_f32", x, 4, 4, 0, 3, V)
    refused("u2pl_wino_wgrad_finish_f32", x, 1, 1, 4, 3, 0, V)
    refused("u2pl_wino_wgrad_finish_f32", x, 1, 1, 6, 4, 0, V)
    refused("u2pl_wino_output_f32", Mb, N, H, W, C, 1, 3, None, y, 8, None, None)
    refused("u2pl_wino_output_f32", Mb, N, H, W, 6, 1, 4, None, y, 8, None, None)
    refused("u2pl_wino_output_f32", Mb, N, H, W, C, 0, 4, None, y, 8, None, None)
    refused("u2pl_wino_output_f32", Mb, N, H, W, C, 1, 4, None, y, 10, None, None)      # ldy % 4 != 0
    refused("u2pl_wino_output_f32", Mb, 1, 2, 2, 1028, 1, 4, None, y, 1028, part, None)  # statistics with O > 1024
    refused("u2pl_wino_output_bnact_f32", Mb, N, H, W, C, 1, 4, None, y, 8, None, vec, vec, vec, None, 8, 0)     # NULL mean
    refused("u2pl_wino_output_bnact_amax_f32", Mb, N, H, W, C, 1, 4, None, y, 8, None, vec, vec, vec, None, 8, 0, obj)
    refused("u2pl_wino_output_bnact_f32", Mb, N, H, W, C, 1, 4, None, y, 8, vec, vec, vec, vec, x, 10, 0)        # ldr % 4 != 0
    refused("u2pl_absmax_f32", x, 10, 4, 8, obj, 1)
    torch.cuda.synchronize()
    for buf in (V, y, part):
        assert (buf.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
