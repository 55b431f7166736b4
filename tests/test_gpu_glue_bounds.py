"""The glue kernels of u2pl_amd/csrc/nn.hip against float64 at every shape, pitch and edge of tests/glue_bounds.py: max pool,
feature bilinear, row copies / broadcast / concat, global average pool, softmax_rows, dense_small, SGD / Adam / EMA, the box and
class mixes, label presence and the sliding-window accumulator -- through _lib.call AND through their wrappers
(nn.MaxPool3x3s2Ceil, nn.global_avg_pool, nn.upsample_bilinear, nn.cat_channels, ParamArena, trainer.cutmix / cutout / classmix /
classmix_select).  Exact operations are compared bit for bit with the numpy fp32 emulation and with the float64 reference rounded
to fp32; everything else is inside min(derived count, CAL_MARGIN x what torch's own fp32 reaches) on EVERY element.  Every pitched
output is pre-filled with a sentinel bit pattern that must survive outside the M x C region, and each kernel runs once more at
the first size that takes a second grid-stride trip.  Figures are printed before they are asserted (-s).
tests/test_glue_bounds_cpu.py pins the references and shows that the bounds reject faulty arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_bounds as GB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
f32, f64 = np.float32, np.float64
SENT = np.array([GB.SENTINEL_BITS], dtype=np.uint32).view(f32)[0]


def call(*a):
    from u2pl_amd._lib import call as c
    return c(*a)


def K():
    from u2pl_amd import nn as Kn
    return Kn


def D(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def H(t):
    return t.detach().cpu().numpy()


def report(name, **figs):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in figs.items()), end="")


class Pitched:
    """rows [M, C] inside a sentinel-filled buffer of M + 2 rows of ld floats, starting at column `off` (a multiple of 4)"""

    def __init__(self, M, C, ld, off=0, rows=None):
        assert off % 4 == 0 and off + C <= ld
        self.M, self.C, self.ld, self.off = M, C, ld, off
        host = np.full((M + 2, ld), SENT, dtype=f32)
        if rows is not None:
            host[:M, off:off + C] = rows
        self.buf = D(host)
        self.ptr = self.buf[:, off:]            # the kernel's base pointer: row r, column c at ptr + r ld + c

    def rows(self):
        return H(self.buf)[:self.M, self.off:self.off + self.C].copy()

    def assert_padding_untouched(self, what=""):
        bits = H(self.buf).view(np.uint32).copy()
        bits[:self.M, self.off:self.off + self.C] = GB.SENTINEL_BITS
        assert (bits == GB.SENTINEL_BITS).all(), f"{what}: wrote outside the {self.M} x {self.C} region (ld {self.ld}, offset {self.off})"


def layouts(C):
    """(ld, offset) of a dense tensor and of the channel slice [:, 8:8 + C] of a wider buffer"""
    return ((C, 0), (C + 12, 8))


def to_rows(x):
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1).reshape(-1, x.shape[1]))


def from_rows(r, N, Hh, W):
    return np.ascontiguousarray(r.reshape(N, Hh, W, -1).transpose(0, 3, 1, 2))


def wide_slice(x, requires_grad=False):
    """x [N, C, H, W] as the slice [:, 8:8 + C] of a sentinel-filled channels_last tensor of C + 12 channels"""
    N, C, Hh, W = x.shape
    w = torch.full((N, C + 12, Hh, W), float(SENT), dtype=torch.float32, device=DEV).contiguous(memory_format=CL)
    w[:, 8:8 + C] = D(x)
    return w[:, 8:8 + C].detach().requires_grad_(requires_grad)


def dense_cl(x, requires_grad=False):
    return D(x).contiguous(memory_format=CL).requires_grad_(requires_grad)


# ------------------------------------------------------------------ max pool
def pool_raw(x, g, ldx_off, ldy_off):
    N, C, Hh, W = x.shape
    Ho, Wo = GB.pool_out(Hh), GB.pool_out(W)
    xi = Pitched(N * Hh * W, C, *ldx_off, rows=to_rows(x))
    yo = Pitched(N * Ho * Wo, C, *ldy_off)
    tap = torch.full((N * Ho * Wo + 2, C), 0xEE, dtype=torch.uint8, device=DEV)
    call("u2pl_maxpool3s2_fwd_f32", xi.ptr, xi.ld, N, Hh, W, C, Ho, Wo, yo.ptr, yo.ld, tap)
    yo.assert_padding_untouched("pool fwd")
    assert bool((tap[-2:] == 0xEE).all())
    gi = Pitched(N * Ho * Wo, C, *ldy_off, rows=to_rows(g))
    dx = Pitched(N * Hh * W, C, *ldx_off)
    call("u2pl_maxpool3s2_bwd_f32", gi.ptr, gi.ld, tap, N, Hh, W, C, Ho, Wo, dx.ptr, dx.ld)
    dx.assert_padding_untouched("pool bwd")
    return (from_rows(yo.rows(), N, Ho, Wo), from_rows(H(tap[:-2]), N, Ho, Wo), from_rows(dx.rows(), N, Hh, W))


def pool_wrapper(x, g, sliced):
    xt = wide_slice(x, True) if sliced else dense_cl(x, True)
    y = K().MaxPool3x3s2Ceil()(xt)
    y.backward(wide_slice(g) if sliced else dense_cl(g))
    return H(y), H(xt.grad)


@pytest.mark.parametrize("shape", GB.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_forward_taps_backward(shape):
    """output and taps bit-equal to F.max_pool2d(3, 2, 1, ceil_mode=True) (first maximum), the backward inside the float64
    bound and bit-equal to the emulation, dense and as channel slices, raw and through nn.MaxPool3x3s2Ceil"""
    worst, same = 0.0, True
    for fam in GB.POOL_FAMILIES:
        x, g = GB.pool_case(fam, shape)
        y64, tap64, dx64, unit = GB.pool_ref64(x, g)
        ye, te = GB.emu_pool_fwd(x)
        dxe = GB.emu_pool_bwd(g, te, shape[2], shape[3])
        for lay in layouts(shape[1]):
            y, tap, dx = pool_raw(x, g, lay, (lay[0] + (4 if lay[1] else 0), lay[1]))
            ex = GB.rel_excess(dx, dx64, GB.E_pool_bwd() * unit)
            worst, same = max(worst, ex), same and GB.bits_equal(dx, dxe)
            report(f"pool {fam} ld {lay[0]}", bwd_excess=ex, bwd_bits_equal_emulation=GB.bits_equal(dx, dxe))
            assert GB.bits_equal(y, y64.astype(f32)) and GB.bits_equal(y, ye), (fam, lay)
            assert np.array_equal(tap, tap64) and np.array_equal(tap, te), (fam, lay)
            assert ex <= 1.0 and GB.bits_equal(dx, dxe), (fam, lay, ex)
        for sliced in (False, True):
            y, dx = pool_wrapper(x, g, sliced)
            assert GB.bits_equal(y, y64.astype(f32)) and GB.bits_equal(dx, dxe), (fam, sliced)


def test_maxpool_second_grid_stride_trip():
    shape = GB.POOL_STRIDE_SHAPE
    assert shape[0] * GB.pool_out(shape[2]) * GB.pool_out(shape[3]) * shape[1] // 4 > GB.GRID_CAP
    x, g = GB.pool_case("normal", shape)
    y64, tap64, dx64, unit = GB.pool_ref64(x, g)
    y, dx = pool_wrapper(x, g, False)
    ex = GB.rel_excess(dx, dx64, GB.E_pool_bwd() * unit)
    report("pool 2x128x257x257", bwd_excess=ex)
    assert GB.bits_equal(y, y64.astype(f32)) and ex <= 1.0


# ------------------------------------------------------------------ feature bilinear
def bilr_raw(x, g, hi, lay_lo, lay_hi):
    N, C, h, w = x.shape
    xi = Pitched(N * h * w, C, *lay_lo, rows=to_rows(x))
    yo = Pitched(N * hi[0] * hi[1], C, *lay_hi)
    call("u2pl_bilinear_rows_fwd_f32", xi.ptr, xi.ld, N, h, w, C, hi[0], hi[1], yo.ptr, yo.ld)
    yo.assert_padding_untouched("bilinear fwd")
    gi = Pitched(N * hi[0] * hi[1], C, *lay_hi, rows=to_rows(g))
    dx = Pitched(N * h * w, C, *lay_lo)
    call("u2pl_bilinear_rows_bwd_f32", gi.ptr, gi.ld, N, h, w, C, hi[0], hi[1], dx.ptr, dx.ld)
    dx.assert_padding_untouched("bilinear bwd")
    return from_rows(yo.rows(), N, *hi), from_rows(dx.rows(), N, h, w)


@pytest.mark.parametrize("lo,hi", GB.BILR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bilinear_rows_forward_backward(lo, hi):
    """up-sampling, identity and down-sampling sizes, C in 4, 20, 256, N in 1, 3, pitched and dense: the forward bit-equal to
    oracle.restate.bilinear_ac and inside the float64 bound, the backward inside the bound of its own order"""
    wf = wb = 0.0
    same = True
    for C in GB.BILR_C:
        for N in GB.BILR_N:
            x, g = GB.bilr_case(lo, hi, N, C)
            emu = GB.emu_bilr_fwd(x, *hi)
            ref, unit, ru = GB.bilr_fwd64(x, *hi), GB.bilr_fwd_unit(x, *hi), GB.bilr_bwd64(g, *lo)
            emub = GB.emu_bilr_bwd(g, *lo) if C <= 20 else None
            for lay in layouts(C):
                y, dx = bilr_raw(x, g, hi, lay, (lay[0] + (4 if lay[1] else 0), lay[1]))
                ef, eb = GB.rel_excess(y, ref, GB.E_bilr_fwd() * unit), GB.bilr_bwd_excess(dx, g, *lo, ref_unit=ru)
                wf, wb = max(wf, ef), max(wb, eb)
                same = same and (emub is None or GB.bits_equal(dx, emub))
                assert GB.bits_equal(y, emu), (C, N, lay)
                assert ef <= 1.0 and eb <= 1.0, (C, N, lay, ef, eb)
    report(f"bilinear {lo}->{hi}", fwd_excess=wf, bwd_excess=wb, bwd_bits_equal_emulation=same)
    # the wrapper, on a channel slice, with the gradient a channel slice
    x, g = GB.bilr_case(lo, hi, 3, 20)
    if lo != (1, 1):
        xt = wide_slice(x, True)
        y = K().upsample_bilinear(xt, hi)
        y.backward(wide_slice(g))
        assert GB.bits_equal(H(y), GB.emu_bilr_fwd(x, *hi)) and GB.bilr_bwd_excess(H(xt.grad), g, *lo) <= 1.0


def test_bilinear_rows_second_grid_stride_trip():
    (N, C), lo, hi = GB.BILR_STRIDE_FWD
    assert N * hi[0] * hi[1] * C // 4 > GB.GRID_CAP
    x, _ = GB.bilr_case(lo, hi, N, C)
    y = H(K().upsample_bilinear(dense_cl(x), hi))
    ef = GB.rel_excess(y, GB.bilr_fwd64(x, *hi), GB.E_bilr_fwd() * GB.bilr_fwd_unit(x, *hi))
    (N, C), lo, hi = GB.BILR_STRIDE_BWD
    assert N * lo[0] * lo[1] * C // 4 > GB.GRID_CAP
    x2, g = GB.bilr_case(lo, hi, N, C)
    xt = dense_cl(x2, True)
    K().upsample_bilinear(xt, hi).backward(dense_cl(g))
    eb = GB.bilr_bwd_excess(H(xt.grad), g, *lo)
    report("bilinear second trip", fwd_excess=ef, bwd_excess=eb)
    assert GB.bits_equal(y, GB.emu_bilr_fwd(x, 257, 257)) and ef <= 1.0 and eb <= 1.0


def test_upsample_from_a_1x1_map_is_a_broadcast_and_its_backward_the_column_sums():
    wc = 0.0
    for shape in GB.GAP_SHAPES:
        N, C, Hh, W = shape
        g, v = GB.gap_case(shape)            # g: the upstream gradient [N, C, H, W], v: the 1x1 map [N, C]
        for sliced in (False, True):
            vt = D(v.reshape(N, C, 1, 1)).requires_grad_(True)
            y = K().upsample_bilinear(vt, (Hh, W))
            y.backward(wide_slice(g) if sliced else dense_cl(g))
            assert GB.bits_equal(H(y), np.ascontiguousarray(np.broadcast_to(v[:, :, None, None], shape)))
            g64 = g.astype(f64)
            ex = GB.rel_excess(H(vt.grad)[:, :, 0, 0], g64.sum((2, 3)), GB.E_colsum(Hh * W) * np.abs(g64).sum((2, 3)))
            wc = max(wc, ex)
            assert ex <= 1.0, (shape, sliced, ex)
    report("1x1 upsample backward (column sums)", excess=wc)


# ------------------------------------------------------------------ row copies, broadcast, concat
@pytest.mark.parametrize("M", GB.ROW_M)
def test_copy_rows_copy_cols_broadcast_rows(M):
    for C in GB.ROW_C:
        src, old = GB.rows_case(M, C), GB.rows_case(M, C, tag=1)
        for acc in (0, 1):
            s = Pitched(M, C, C + 8, 4, rows=src)
            d = Pitched(M, C, C + 20, 8, rows=old)
            call("u2pl_copy_rows_f32", s.ptr, s.ld, d.ptr, d.ld, M, C, acc)
            d.assert_padding_untouched("copy_rows")
            assert GB.bits_equal(d.rows(), GB.copy_rows_ref(src, old, acc)) and GB.bits_equal(d.rows(), GB.emu_copy_rows(src, old, acc))
        for scale in GB.BCAST_SCALES:
            for rpi in GB.BCAST_RPI:
                v = GB.rows_case(-(-M // rpi), C, tag=2)
                vi = Pitched(v.shape[0], C, C + 4, 0, rows=v)
                d = Pitched(M, C, C + 12, 4)
                call("u2pl_broadcast_rows_f32", vi.ptr, vi.ld, float(scale), d.ptr, d.ld, rpi, M, C)
                d.assert_padding_untouched("broadcast_rows")
                assert GB.bits_equal(d.rows(), GB.broadcast_ref(v, scale, rpi, M)), (C, scale, rpi)
                assert GB.bits_equal(d.rows(), GB.emu_broadcast(v, scale, rpi, M))
    for C in GB.COL_C:
        src = GB.rows_case(M, C, tag=3)
        s = Pitched(M, C, C + 3, 0, rows=src)
        d = Pitched(M, C, C + 5, 4)
        call("u2pl_copy_cols_f32", s.ptr, s.ld, d.ptr, d.ld, M, C)
        d.assert_padding_untouched("copy_cols")
        assert GB.bits_equal(d.rows(), src)


def test_cat_channels_of_4_256_20_and_its_backward_slices():
    N, Hh, W = 2, 5, 7
    xs = [np.random.default_rng([21, c]).standard_normal((N, c, Hh, W), dtype=f32) for c in GB.CAT_CHANNELS]
    ts = [dense_cl(xs[0], True), wide_slice(xs[1], True), dense_cl(xs[2], True)]
    out = K().cat_channels(ts)
    g = np.random.default_rng(22).standard_normal(out.shape, dtype=f32)
    out.backward(dense_cl(g))
    assert GB.bits_equal(H(out), np.concatenate(xs, 1))
    rs = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    torch.cat(rs, 1).backward(torch.from_numpy(g))
    for t, r in zip(ts, rs):
        assert GB.bits_equal(H(t.grad), r.grad.numpy())


def test_row_kernels_second_grid_stride_trip():
    C, M = 4, GB.ROW_STRIDE_ITEMS
    src = np.arange(M * C, dtype=f32).reshape(M, C)
    s, d = Pitched(M, C, C, 0, rows=src), Pitched(M, C, C + 4, 4, rows=np.ones((M, C), dtype=f32))
    call("u2pl_copy_rows_f32", s.ptr, s.ld, d.ptr, d.ld, M, C, 1)
    d.assert_padding_untouched("copy_rows")
    assert GB.bits_equal(d.rows(), (src + f32(1)).astype(f32))
    v = GB.rows_case(-(-M // 17), C, tag=4)
    d = Pitched(M, C, C + 4, 0)
    call("u2pl_broadcast_rows_f32", D(v), C, float(1.0 / 323), d.ptr, d.ld, 17, M, C)
    d.assert_padding_untouched("broadcast_rows")
    assert GB.bits_equal(d.rows(), GB.broadcast_ref(v, 1.0 / 323, 17, M))
    col = np.arange(M, dtype=f32).reshape(M, 1)
    d = Pitched(M, 1, 4, 0)
    call("u2pl_copy_cols_f32", D(col), 1, d.ptr, d.ld, M, 1)
    d.assert_padding_untouched("copy_cols")
    assert GB.bits_equal(d.rows(), col)


# ------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("shape", GB.GAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_global_avg_pool_forward_backward(shape):
    N, C, Hh, W = shape
    HW = Hh * W
    x, g = GB.gap_case(shape)
    x64 = x.astype(f64)
    for sliced in (False, True):
        xt = wide_slice(x, True) if sliced else dense_cl(x, True)
        y = K().global_avg_pool(xt)
        y.backward(D(g.reshape(N, C, 1, 1)))
        ef = GB.rel_excess(H(y)[:, :, 0, 0], x64.mean((2, 3)), GB.E_gap_fwd(HW) * np.abs(x64).mean((2, 3)))
        gb = np.broadcast_to((g.astype(f64) / HW)[:, :, None, None], shape)
        eb = GB.rel_excess(H(xt.grad), gb, GB.E_gap_bwd() * np.abs(gb))
        same = GB.bits_equal(H(y)[:, :, 0, 0], GB.emu_colsum(x, 1.0 / HW))
        report(f"gap {shape} sliced {sliced}", fwd_excess=ef, bwd_excess=eb, fwd_bits_equal_emulation=same)
        assert ef <= 1.0 and eb <= 1.0
        assert GB.bits_equal(H(xt.grad), np.ascontiguousarray(np.broadcast_to(GB.emu_broadcast(g, 1.0 / HW, 1, N)[:, :, None, None], shape)))


# ------------------------------------------------------------------ softmax_rows
def softmax_raw(z, ldx, ldy):
    M, C = z.shape
    xi, yo = Pitched(M, C, ldx, 0, rows=z), Pitched(M, C, ldy, 0)
    call("u2pl_softmax_rows_f32", xi.ptr, xi.ld, yo.ptr, yo.ld, M, C)
    yo.assert_padding_untouched("softmax_rows")
    return yo.rows()


@pytest.mark.parametrize("C", GB.SOFTMAX_C)
def test_softmax_rows(C):
    we = ws = 0.0
    for fam in GB.SOFTMAX_FAMILIES:
        for M in GB.SOFTMAX_M:
            z = GB.softmax_case(fam, C, M)
            e, s = GB.softmax_excess(softmax_raw(z, C + 3, C + 1), z)
            we, ws = max(we, e), max(ws, s)
            assert e <= 1.0 and s <= 1.0, (fam, M, e, s)
    report(f"softmax_rows C={C}", element_excess=we, rowsum_excess=ws)


def test_softmax_rows_second_grid_stride_trip():
    M, C = GB.SOFTMAX_STRIDE
    z = np.random.default_rng(23).standard_normal((M, C), dtype=f32) * f32(3)
    e, s = GB.softmax_excess(softmax_raw(z, C + 1, C), z)
    report("softmax_rows second trip", element_excess=e, rowsum_excess=s)
    assert e <= 1.0 and s <= 1.0


# ------------------------------------------------------------------ dense_small
@pytest.mark.parametrize("K_", GB.DENSE_K)
def test_dense_small_is_the_correctly_rounded_dot_product(K_):
    worst = 0.0
    for fam in GB.DENSE_FAMILIES:
        for M in GB.DENSE_M:
            for Cout in GB.DENSE_COUT:
                x, w, b = GB.dense_case(fam, M, K_, Cout)
                for bias in (b, None):
                    xi, yo = Pitched(M, K_, K_ + 8, 4, rows=x), Pitched(M, Cout, Cout + 3, 0)
                    call("u2pl_dense_small_f32", xi.ptr, xi.ld, D(w), None if bias is None else D(bias), yo.ptr, yo.ld, M, K_, Cout)
                    yo.assert_padding_untouched("dense_small")
                    ex = GB.dense_excess(yo.rows(), x, w, bias)
                    worst = max(worst, ex)
                    assert ex <= 1.0, (fam, M, Cout, bias is None, ex)
    report(f"dense_small K={K_}", excess=worst)


# ------------------------------------------------------------------ SGD, Adam, EMA
def tail_ok(*ts):
    return all(bool((t[-8:].view(torch.int32) == GB.SENTINEL_BITS).all()) for t in ts)


def flat(a):
    """a flat device buffer with eight sentinel floats behind it"""
    return D(np.concatenate([a, np.full(8, SENT, dtype=f32)]))


def sgd_raw(p, grads, b1, b2, lrs, mom, wd, gs):
    n = p.size
    pt, bt = flat(p), flat(np.zeros(n, dtype=f32))
    out = []
    for k, g in enumerate(grads):
        call("u2pl_sgd_step_f32", pt, D(g), bt, n, b1, b2, float(lrs[0]), float(lrs[1]), float(lrs[2]), float(mom), float(wd), int(k == 0), float(gs))
        out.append((H(pt)[:n].copy(), H(bt)[:n].copy()))
    assert tail_ok(pt, bt)
    return out


@pytest.mark.parametrize("n", GB.OPT_N)
def test_sgd_step_segments_scales_and_decay(n):
    worst = 0.0
    p, grads = GB.opt_case(n, GB.SGD_STEPS)
    for b1, b2 in GB.seg_table(n):
        for gs in GB.SGD_SCALES:
            for wd in GB.SGD_DECAYS:
                a = (p, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, wd, gs)
                got, emu = sgd_raw(*a), GB.emu_sgd(*a)
                ex = GB.sgd_excess(got, GB.sgd_ref64(*a))
                worst = max(worst, ex)
                assert all(GB.bits_equal(u[0], v[0]) and GB.bits_equal(u[1], v[1]) for u, v in zip(got, emu)), (b1, b2, gs, wd)
                assert ex <= 1.0, (b1, b2, gs, wd, ex)
    report(f"sgd n={n}", excess=worst)


def adam_raw(p, grads, b1, b2, lrs, betas, eps):
    n = p.size
    pt, mt, vt = flat(p), flat(np.zeros(n, dtype=f32)), flat(np.zeros(n, dtype=f32))
    out = []
    for k, g in enumerate(grads):
        be1, om1, be2, om2, bc1, bc2s = GB.adam_host_args(betas, k + 1)
        call("u2pl_adam_step_f32", pt, D(g), mt, vt, n, b1, b2, float(lrs[0]), float(lrs[1]), float(lrs[2]), be1, om1, be2, om2, float(eps), 0.0,
             bc1, bc2s, 1.0)
        out.append(dict(p=H(pt)[:n].copy(), m=H(mt)[:n].copy(), v=H(vt)[:n].copy()))
    assert tail_ok(pt, mt, vt)
    return out


@pytest.mark.parametrize("betas", GB.ADAM_BETAS, ids=lambda b: f"beta2_{b[1]}")
def test_adam_step_against_float64_adam(betas):
    """five steps against torch.optim.Adam in float64 (Python-double betas): exp_avg_sq relative to itself, exp_avg relative to
    max |g|, the update relative to lr (FINDING 2 of glue_bounds); names the quantity that leaves its bound"""
    worst = dict(exp_avg_sq=0.0, exp_avg=0.0, update=0.0)
    same = dict(p=True, m=True, v=True)
    for n in GB.OPT_N:
        p, grads = GB.opt_case(n, GB.ADAM_STEPS)
        for b1, b2 in GB.seg_table(n):
            a = (p, grads, b1, b2, GB.ADAM_LRS, betas, GB.ADAM_EPS)
            got = adam_raw(*a)
            ex = GB.adam_excess(got, GB.adam_ref64(*a), p, grads, GB.seg_lr(n, b1, b2, GB.ADAM_LRS).astype(f64), betas)
            same = {k: same[k] and all(GB.bits_equal(u[k], v[k]) for u, v in zip(got, GB.emu_adam(*a))) for k in same}
            worst = {k: max(worst[k], v) for k, v in ex.items()}
            bad = [k for k, v in ex.items() if not v <= 1.0]
            assert not bad, f"{bad} out of bound at n={n} segments=({b1}, {b2}) betas={betas}: {ex}"
    report(f"adam betas={betas}", bits_equal_emulation=same, **worst)
    assert same["m"] and same["v"]          # products and sums only: the moments are the emulation's bit for bit


def test_ema_update_every_decay():
    worst = 0.0
    for n in GB.OPT_N:
        t, (s,) = GB.opt_case(n, 1, seed=3)
        for d in GB.EMA_DECAYS:
            tt = flat(t)
            call("u2pl_ema_update_f32", tt, D(s), n, float(d), float(1 - d))
            got = H(tt)[:n]
            ref, unit = GB.ema_ref64(t, s, d)
            ex = GB.rel_excess(got, ref, GB.E_ema() * unit + 1e-300)
            worst = max(worst, ex)
            assert tail_ok(tt) and GB.bits_equal(got, GB.emu_ema(t, s, d)) and ex <= 1.0, (n, d, ex)
    report("ema", excess=worst)


def test_optimizers_second_grid_stride_trip():
    n, (b1, b2) = GB.OPT_STRIDE_N, GB.OPT_STRIDE_SEGS
    assert b1 < GB.GRID_CAP < b2 < n
    p, grads = GB.opt_case(n, 2)
    a = (p, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, 5e-4, 1.0 / 3)
    got, emu = sgd_raw(*a), GB.emu_sgd(*a)
    assert all(GB.bits_equal(u[0], v[0]) and GB.bits_equal(u[1], v[1]) for u, v in zip(got, emu))
    es = GB.sgd_excess(got, GB.sgd_ref64(*a))
    betas = GB.ADAM_BETAS[1]
    a = (p, grads, b1, b2, GB.ADAM_LRS, betas, GB.ADAM_EPS)
    ea = GB.adam_excess(adam_raw(*a), GB.adam_ref64(*a), p, grads, GB.seg_lr(n, b1, b2, GB.ADAM_LRS).astype(f64), betas)
    tt = flat(p)
    call("u2pl_ema_update_f32", tt, D(grads[0]), n, float(0.99), float(1 - 0.99))
    report("optimizers second trip", sgd_excess=es, **{"adam_" + k: v for k, v in ea.items()})
    assert tail_ok(tt) and GB.bits_equal(H(tt)[:n], GB.emu_ema(p, grads[0], 0.99))
    assert es <= 1.0 and max(ea.values()) <= 1.0, (es, ea)


def arena_of(sizes, seed, with_grad=True):
    """a ParamArena of three groups of 1-D / 2-D parameters (every parameter is padded to a multiple of 64 elements)"""
    from u2pl_amd.nn import ParamArena
    rng = np.random.default_rng([24, seed])
    groups = [[torch.nn.Parameter(D(rng.standard_normal(s, dtype=f32))) for s in grp] for grp in sizes]
    return ParamArena(groups, with_grad=with_grad)


ARENA_SIZES = (((70,), (5, 13)), ((129,),), ((64,), (3,)))


def arena_grads(ar, steps, seed):
    """gradients over the flat arena, zero in the padding (what zero_grad and the layer kernels leave there)"""
    live = np.zeros(ar.n, dtype=bool)
    for p in ar.params:
        live[ar._offs[id(p)]:ar._offs[id(p)] + p.numel()] = True
    rng = np.random.default_rng([25, seed])
    return [np.where(live, rng.standard_normal(ar.n, dtype=f32), f32(0)) for _ in range(steps)]


def test_param_arena_sgd_adam_ema_wrappers():
    ar = arena_of(ARENA_SIZES, 0)
    b1, b2 = ar.bounds[0], ar.bounds[1]
    assert 0 < b1 < b2 < ar.n and b1 % 64 == 0
    p0 = H(ar.flat).copy()
    grads = arena_grads(ar, GB.SGD_STEPS, 0)
    emu = GB.emu_sgd(p0, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, 5e-4, 0.125)
    ref = GB.sgd_ref64(p0, grads, b1, b2, GB.SGD_LRS, GB.SGD_MOMENTUM, 5e-4, 0.125)
    got = []
    for g in grads:
        ar.grad.copy_(D(g))
        ar.sgd_step(GB.SGD_LRS, GB.SGD_MOMENTUM, 5e-4, grad_scale=0.125)
        got.append((H(ar.flat).copy(), H(ar.momentum_buf).copy()))
    assert all(GB.bits_equal(u[0], v[0]) and GB.bits_equal(u[1], v[1]) for u, v in zip(got, emu))
    es = GB.sgd_excess(got, ref)
    assert H(ar.params[1]).shape == (5, 13) and GB.bits_equal(H(ar.params[1]).reshape(-1), got[-1][0][128:128 + 65])
    worst = {}
    for betas in GB.ADAM_BETAS:
        ar = arena_of(ARENA_SIZES, 1)
        p0, grads = H(ar.flat).copy(), arena_grads(ar, GB.ADAM_STEPS, 1)
        got = []
        for g in grads:
            ar.grad.copy_(D(g))
            ar.adam_step(GB.ADAM_LRS, betas, GB.ADAM_EPS, 0.0)
            got.append(dict(p=H(ar.flat).copy(), m=H(ar.exp_avg).copy(), v=H(ar.exp_avg_sq).copy()))
        a = (p0, grads, b1, b2, GB.ADAM_LRS, betas, GB.ADAM_EPS)
        live = np.concatenate([np.arange(ar._offs[id(p)], ar._offs[id(p)] + p.numel()) for p in ar.params])
        pick = lambda seq: [{k: v[live] for k, v in st.items()} for st in seq]          # (the padding has v = 0: no relative unit)
        ex = GB.adam_excess(pick(got), pick(GB.adam_ref64(*a)), p0[live], [g[live] for g in grads],
                            GB.seg_lr(ar.n, b1, b2, GB.ADAM_LRS).astype(f64)[live], betas)
        worst[betas[1]] = ex
        bad = [k for k, v in ex.items() if not v <= 1.0]
        assert not bad, f"{bad} out of bound through ParamArena.adam_step, betas={betas}: {ex}"
        assert not got[-1]["p"][~np.isin(np.arange(ar.n), live)].any()
    src, dst = arena_of(ARENA_SIZES, 2, with_grad=False), arena_of(ARENA_SIZES, 3, with_grad=False)
    for d in GB.EMA_DECAYS:
        t0, s0 = H(dst.flat).copy(), H(src.flat).copy()
        dst.ema_from(src, d)
        assert GB.bits_equal(H(dst.flat), GB.emu_ema(t0, s0, d)), d
    report("ParamArena", sgd_excess=es, **{f"adam_{b}_{k}": v for b, e in worst.items() for k, v in e.items()})
    assert es <= 1.0


# ------------------------------------------------------------------ cutmix, cutout, classmix, label presence
def mix_raw(mode, img, lab, conf, boxes=None, sel=None):
    B, C, Hh, W = img.shape
    i, l, c = D(img), D(lab), D(conf)
    oi, ol, oc = flat(np.zeros(img.size, dtype=f32)), torch.full((lab.size + 8,), -7, dtype=torch.int64, device=DEV), flat(np.zeros(conf.size, dtype=f32))
    bx = None if boxes is None else D(np.asarray(boxes, dtype=np.int32))
    sd = None if sel is None else D(sel.view(np.int64))
    if mode == "cutmix":
        call("u2pl_cutmix_f32", i, l, c, bx, B, C, Hh, W, oi, ol, oc)
    else:
        call("u2pl_strong_aug_f32", i, l, c, bx, sd, 1 if mode == "cutout" else 2, B, C, Hh, W, oi, ol, oc)
    assert tail_ok(oi, oc) and bool((ol[-8:] == -7).all())
    return H(oi)[:-8].reshape(img.shape), H(ol)[:-8].reshape(lab.shape), H(oc)[:-8].reshape(conf.shape)


def same3(a, b):
    return all(GB.bits_equal(np.ascontiguousarray(u), np.ascontiguousarray(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("B", GB.MIX_B)
def test_cutmix_cutout_classmix_bit_equal_to_the_reference_expression(B):
    from u2pl_amd import trainer as Tr
    for C in GB.MIX_C:
        for Hh, W in GB.MIX_HW:
            img, lab, conf = GB.mix_case(B, C, Hh, W)
            dev = (D(img), D(lab), D(conf))
            for boxes in GB.mix_boxes(B, Hh, W):
                for mode, wrap in (("cutmix", Tr.cutmix), ("cutout", Tr.cutout)):
                    ref = GB.mix_ref(mode, img, lab, conf, boxes=boxes)
                    assert same3(mix_raw(mode, img, lab, conf, boxes=boxes), ref), (mode, C, Hh, W, boxes)
                    assert same3([H(t) for t in wrap(*dev, boxes)], ref), (mode, C, Hh, W, boxes)
            for sel in GB.mix_selections(B):
                ref = GB.mix_ref("classmix", img, lab, conf, sel=sel)
                assert same3(mix_raw("classmix", img, lab, conf, sel=sel), ref), (C, Hh, W, sel)
                assert same3([H(t) for t in Tr.classmix(*dev, sel)], ref), (C, Hh, W, sel)


def test_mixes_second_grid_stride_trip():
    B, C, Hh, W = GB.MIX_STRIDE
    assert B * Hh * W > GB.GRID_CAP
    img, lab, conf = GB.mix_case(B, C, Hh, W)
    boxes = [(100, 725, 300, 724), (0, 1, 0, 1)]
    sel = GB.mix_selections(B)[2]
    for mode, kw in (("cutmix", dict(boxes=boxes)), ("cutout", dict(boxes=boxes)), ("classmix", dict(sel=sel))):
        assert same3(mix_raw(mode, img, lab, conf, **kw), GB.mix_ref(mode, img, lab, conf, **kw)), mode


@pytest.mark.parametrize("HW", GB.PRESENCE_HW)
def test_label_presence_and_classmix_select(HW):
    from u2pl_amd import trainer as Tr
    B = 5
    lab = GB.presence_case(B, HW)
    want = GB.presence_ref(lab)
    bits = torch.zeros(B + 1, dtype=torch.int64, device=DEV)
    call("u2pl_label_presence_i64", D(lab), B, HW, bits)
    assert np.array_equal(H(bits)[:B].view(np.uint64), want) and int(bits[B]) == 0
    sel = Tr.classmix_select(D(lab.reshape(B, 1, HW)), randperm=lambda k: torch.arange(k))       # the first half of the sorted classes
    for i in range(B):
        present = [c for c in range(64) if (int(want[i]) >> c) & 1]
        assert int(sel[i]) == sum(1 << c for c in present[:len(present) // 2])


# ------------------------------------------------------------------ sliding-window accumulate / normalize
@pytest.mark.parametrize("C", GB.WIN_C)
def test_window_accumulate_and_normalize(C):
    Hh, W = GB.WIN_ACC
    srcs = GB.window_case(C)
    pred, count = flat(np.zeros(C * Hh * W, dtype=f32)), flat(np.zeros(Hh * W, dtype=f32))
    for (h0, w0, hc, wc), s in zip(GB.WINDOWS, srcs):
        call("u2pl_window_accumulate_f32", pred, count, C, Hh, W, D(s), h0, w0, hc, wc)
    pe, ce = GB.emu_windows(C, srcs)
    assert tail_ok(pred, count)
    assert GB.bits_equal(H(pred)[:-8].reshape(pe.shape), pe) and GB.bits_equal(H(count)[:-8].reshape(ce.shape), ce)
    call("u2pl_window_normalize_f32", pred, count, C, Hh, W)
    got = H(pred)[:-8].reshape(pe.shape)
    covered = np.broadcast_to(ce > 0, pe.shape)
    ref = pe.astype(f64) / np.where(ce > 0, ce, 1).astype(f64)
    same = GB.bits_equal(got[covered], (pe / np.where(ce > 0, ce, f32(1))).astype(f32)[covered])
    ex = GB.rel_excess(got[covered], ref[covered], 2 * GB.EPS * np.abs(ref[covered]) + 1e-300)      # one ulp is at most 2 EPS |ref|
    report(f"window_normalize C={C}", excess_of_one_ulp=ex, bits_equal_ieee_division=same)
    assert tail_ok(pred) and covered.all() and ex <= 1.0


# ------------------------------------------------------------------ the argument contract: 1001 before any launch
def test_out_of_contract_arguments_return_1001_before_any_launch():
    from u2pl_amd._lib import HipError
    a, b = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    tap = torch.zeros(64, dtype=torch.uint8, device=DEV)
    bad = [("u2pl_maxpool3s2_fwd_f32", a, 6, 1, 1, 1, 6, 1, 1, b, 6, tap),
           ("u2pl_maxpool3s2_bwd_f32", a, 6, tap, 1, 1, 1, 6, 1, 1, b, 6),
           ("u2pl_copy_rows_f32", a, 6, b, 6, 1, 6, 0),
           ("u2pl_broadcast_rows_f32", a, 6, 1.0, b, 6, 1, 1, 6),
           ("u2pl_bilinear_rows_fwd_f32", a, 6, 1, 1, 1, 6, 1, 1, b, 6),
           ("u2pl_bilinear_rows_bwd_f32", a, 6, 1, 1, 1, 6, 1, 1, b, 6),
           ("u2pl_dense_small_f32", a, 4, b, None, b, 1, 0, 4, 1),
           ("u2pl_dense_small_f32", a, 4, b, None, b, 1, 17, 4, 1),
           ("u2pl_dense_small_f32", a, 6, b, None, b, 1, 1, 6, 1),
           ("u2pl_window_accumulate_f32", a, b, 1, 4, 4, a, 2, 2, 3, 2),
           ("u2pl_window_accumulate_f32", a, b, 1, 4, 4, a, 0, -1, 2, 2),
           ("u2pl_window_accumulate_f32", a, b, 1, 4, 4, a, 0, 3, 2, 2)]
    for args in bad:
        with pytest.raises(HipError, match="1001"):
            call(*args)
    torch.cuda.synchronize()
    assert not bool(a.any()) and not bool(b.any()) and not bool(tap.any())
