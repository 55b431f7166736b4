"""Float64 references, numpy fp32 emulations, shape tables and error bounds of the pyramid-pooling kernels in
u2pl_amd/csrc/pool.hip (u2pl_pyramid_pool_fwd_f32 / u2pl_pyramid_pool_bwd_f32), shared by tests/test_psp_cpu.py and
tests/test_gpu_psp.py.  Not a conftest: imported by name, like glue_bounds.

Window rule (torch's adaptive pooling), per axis: window i of b over an axis of length H is [floor(i H / b), ceil((i + 1) H / b)).
Its inverse: the windows that contain position h are the contiguous range floor(h b / H) .. ceil((h + 1) b / H) - 1.

Every element is held to  |got - ref64| <= EPS min(derived, CAL_MARGIN measured) unit  (EPS = 2^-24, one unit per fp32 rounding):

    forward    unit = mean |x| over the window.  derived = fwd_count(area): lane j of 16 adds the pixels j, j + 16, ... of the
               window to 0.0f (ceil(area / 16) - 1 roundings: the first add lands on 0), four rounds of pairwise lane adds (a
               round whose partner lanes are all empty rounds nothing: ceil(log2(min(area, 16))) of them), one division.
    backward   unit = sum over the windows containing the pixel of |g| / area, plus |add|.  derived = bwd_count(T, add): every
               term carries the rounding of 1.0f / area and of the product (2, in units of its own |g| / area), the T terms
               are added to 0.0f one after the other (T - 1) and `add` last (1).
    measured   what torch's own fp32 F.adaptive_avg_pool2d (CPU) reaches against float64 over PSP_HW x PSP_LEVEL_SETS at
               CAL_N, CAL_C -- never a HIP kernel (python -m pytest tests/test_psp_cpu.py -s -k ceilings; the emulation of the
               kernels' order in brackets):
                   forward    units of EPS mean |x|:                       9.72 [2.42]
                   backward   units of EPS (sum |g| / area + |add|):       2.53 [2.42]

Inputs: x = N(0, 1) + 0.5 (a mean that does not vanish), g and add = N(0, 1); no infinities or NaN in any operand (NaN only in
the gaps of pitched buffers, which no kernel may read)."""
import numpy as np
import torch
import torch.nn.functional as F

from contrast_bounds import CAL_MARGIN
from glue_bounds import SENTINEL_BITS, bits_equal, rel_excess  # noqa: F401
from split_bounds import EPS

f32, f64 = np.float32, np.float64

PSP_HW = ((1, 1), (2, 3), (3, 4), (5, 6), (6, 6), (7, 10), (13, 11), (33, 35))
PSP_C = (4, 20, 64, 260)
PSP_N = (1, 3)
PSP_LEVEL_SETS = ((1, 2, 3, 6), (6,), (2, 0, 0, 0), (1, 1, 1, 1))
RULE_H = (1, 2, 3, 4, 5, 6, 7, 11, 13, 33, 97)
RULE_B = (1, 2, 3, 6)
CAL_N, CAL_C = 3, 20
# csrc/pool.hip
FWD_LANES = 16                  # pixel lanes of a forward work item
FWD_CHANNELS = 64               # channels of a forward work item (16 float4 lanes)
FWD_GRID_CAP = 2048             # blocks; one block per work item (level, image, window, channel chunk)
BWD_SEG = 4                     # consecutive pixels of an image row per backward work item
BWD_GRID_CAP = 4096 * 4         # work items of one trip: grid_for()'s 4096 blocks of four waves, one wave per item
BWD_LANE_CHANNELS = 64 * 8 * 4  # channels of one pass of a wave: 64 lanes x 8 float4
FWD_STRIDE_CASE = dict(N=3, C=896, HW=(5, 6), levels=(1, 2, 3, 6))      # 3 * 50 windows * 14 chunks = 2100 items > 2048
BWD_STRIDE_CASE = dict(N=3, C=20, HW=(146, 149), levels=(6, 1))         # 3 * 146 * ceil(149 / 4) = 16644 items > 16384
BWD_CHANNEL_CASE = dict(N=1, C=2052, HW=(5, 6), levels=(1, 2, 3, 6))    # one float4 more than a pass of a wave takes
FAULTS_FWD = ("end_floor", "nominal_area")
FAULTS_BWD = ("one_window_per_axis", "area_of_another_level")

# ---- calibrated ceilings: torch's own fp32 arithmetic against float64 (never the HIP kernels), rounded up by a few per cent
CAL_PSP_FWD = 10.0       # measured 9.72 (level 1 at 33 x 35: torch adds the 1155 pixels of the window one after the other)
CAL_PSP_BWD = 2.6        # measured 2.53


# =================================================================== the window rule ==========================================
def window(i, H, b):
    """-> (start, end) of window i of b over an axis of length H"""
    return (i * H) // b, -((-(i + 1) * H) // b)


def cover(h, H, b):
    """-> (first, last) index of the windows of b over H that contain position h (inclusive): the inverse of window()"""
    return (h * b) // H, -((-(h + 1) * b) // H) - 1


def used(levels):
    return [(k, b) for k, b in enumerate(levels) if b > 0]


def case(N, C, H, W, levels, seed=0):
    """-> x [N, C, H, W], {level slot: g [N, C, b, b]}, add [N, C, H, W]  (float32)"""
    rng = np.random.default_rng([seed, 31, N, C, H, W] + list(levels))
    x = rng.standard_normal((N, C, H, W), dtype=f32) + f32(0.5)
    gs = {k: rng.standard_normal((N, C, b, b), dtype=f32) for k, b in used(levels)}
    add = rng.standard_normal((N, C, H, W), dtype=f32)
    return x, gs, add


# =================================================================== float64 references ========================================
def fwd64(x, b):
    """-> (mean [N, C, b, b], mean |x| the forward's unit, area [b, b])"""
    N, C, H, W = x.shape
    x64 = x.astype(f64)
    y, u, area = np.zeros((N, C, b, b)), np.zeros((N, C, b, b)), np.zeros((b, b), dtype=np.int64)
    for i in range(b):
        h0, h1 = window(i, H, b)
        for j in range(b):
            w0, w1 = window(j, W, b)
            y[:, :, i, j] = x64[:, :, h0:h1, w0:w1].mean((2, 3))
            u[:, :, i, j] = np.abs(x64[:, :, h0:h1, w0:w1]).mean((2, 3))
            area[i, j] = (h1 - h0) * (w1 - w0)
    return y, u, area


def bwd64(gs, levels, add, shape):
    """gs: {slot: g} (a missing slot = a null g) -> (dx, unit, T the number of windows over each pixel [H, W])"""
    N, C, H, W = shape
    dx, unit, T = np.zeros(shape), np.zeros(shape), np.zeros((H, W), dtype=np.int64)
    for k, b in used(levels):
        if k not in gs:
            continue
        g = gs[k].astype(f64)
        for i in range(b):
            h0, h1 = window(i, H, b)
            for j in range(b):
                w0, w1 = window(j, W, b)
                a = (h1 - h0) * (w1 - w0)
                dx[:, :, h0:h1, w0:w1] += (g[:, :, i, j] / a)[:, :, None, None]
                unit[:, :, h0:h1, w0:w1] += (np.abs(g[:, :, i, j]) / a)[:, :, None, None]
                T[h0:h1, w0:w1] += 1
    if add is not None:
        dx += add.astype(f64)
        unit += np.abs(add.astype(f64))
    return dx, unit, T


# =================================================================== bounds ====================================================
def _b(derived, cal):
    return np.minimum(derived, CAL_MARGIN * cal)


def fwd_count(area):
    area = np.asarray(area, dtype=np.int64)
    rounds = np.ceil(np.log2(np.minimum(area, FWD_LANES))).astype(np.int64)
    return (-(-area // FWD_LANES) - 1) + rounds + 1


def bwd_count(T, with_add):
    T = np.asarray(T, dtype=np.int64)
    return np.where(T > 0, 2 + (T - 1), 0) + (1 if with_add else 0)


def E_fwd(area):
    """[b, b] multiples of the unit"""
    return EPS * _b(fwd_count(area), CAL_PSP_FWD)


def E_bwd(T, with_add):
    """[H, W] multiples of the unit"""
    return EPS * _b(bwd_count(T, with_add), CAL_PSP_BWD)


def fwd_excess(got, x, b):
    y, u, area = fwd64(x, b)
    return rel_excess(got, y, E_fwd(area)[None, None] * u)


def bwd_excess(got, gs, levels, add, shape):
    dx, unit, T = bwd64(gs, levels, add, shape)
    return rel_excess(got, dx, E_bwd(T, add is not None)[None, None] * unit)


# =================================================================== numpy fp32 emulations of the kernels' own order ============
def emu_fwd(x, b, fault=None):
    """k_pyramid_pool_fwd.  Faults: end_floor (window end = floor((i + 1) H / b): the shared row is lost), nominal_area (the
    division is by (H / b)(W / b) as a real number rounded to fp32, not by the window's own area)"""
    N, C, H, W = x.shape
    y = np.zeros((N, C, b, b), dtype=f32)
    for i in range(b):
        h0, h1 = window(i, H, b)
        for j in range(b):
            w0, w1 = window(j, W, b)
            if fault == "end_floor":
                h1, w1 = max(h0 + 1, ((i + 1) * H) // b), max(w0 + 1, ((j + 1) * W) // b)
            px = x[:, :, h0:h1, w0:w1].reshape(N, C, -1)
            area = px.shape[2]
            lanes = np.zeros((FWD_LANES, N, C), dtype=f32)
            for k in range(area):
                lanes[k % FWD_LANES] = (lanes[k % FWD_LANES] + px[:, :, k]).astype(f32)
            o = FWD_LANES // 2
            while o:
                lanes[:o] = (lanes[:o] + lanes[o:2 * o]).astype(f32)
                o //= 2
            div = f32((H / b) * (W / b)) if fault == "nominal_area" else f32(area)
            y[:, :, i, j] = (lanes[0] / div).astype(f32)
    return y


def emu_bwd(gs, levels, add, shape, fault=None):
    """k_pyramid_pool_bwd.  Faults: one_window_per_axis (only the first window of the covering range on each axis),
    area_of_another_level (1 / area taken from the next used level's window of the same indices, clamped)"""
    N, C, H, W = shape
    dx = np.zeros(shape, dtype=f32)
    lv = used(levels)
    for h in range(H):
        for w in range(W):
            acc = np.zeros((N, C), dtype=f32)
            for n_, (k, b) in enumerate(lv):
                if k not in gs:
                    continue
                (i0, i1), (j0, j1) = cover(h, H, b), cover(w, W, b)
                if fault == "one_window_per_axis":
                    i1, j1 = i0, j0
                ba = lv[(n_ + 1) % len(lv)][1] if fault == "area_of_another_level" else b
                for i in range(i0, i1 + 1):
                    for j in range(j0, j1 + 1):
                        ia, ja = min(i, ba - 1), min(j, ba - 1)
                        (a0, a1), (c0, c1) = window(ia, H, ba), window(ja, W, ba)
                        inv = f32(1.0) / f32((a1 - a0) * (c1 - c0))
                        acc = (acc + (gs[k][:, :, i, j] * inv).astype(f32)).astype(f32)
            if add is not None:
                acc = (acc + add[:, :, h, w]).astype(f32)
            dx[:, :, h, w] = acc
    return dx


# =================================================================== torch's own fp32 arithmetic ===============================
def torch_fwd_fp32(x, b):
    return F.adaptive_avg_pool2d(torch.from_numpy(x), b).numpy()


def torch_bwd_fp32(gs, levels, add, shape):
    xt = torch.zeros(shape, dtype=torch.float32, requires_grad=True)
    loss = (xt * torch.from_numpy(add)).sum() if add is not None else 0.0
    for k, b in used(levels):
        if k in gs:
            loss = loss + (F.adaptive_avg_pool2d(xt, b) * torch.from_numpy(gs[k])).sum()
    loss.backward()
    return xt.grad.numpy()


def _ratio(got, ref, unit):
    return rel_excess(got, ref, EPS * np.asarray(unit, dtype=f64) + 1e-300)


def measure(form="torch"):
    """-> (forward in EPS mean |x|, backward in EPS (sum |g| / area + |add|)) over PSP_HW x PSP_LEVEL_SETS at CAL_N, CAL_C"""
    fwd = bwd = 0.0
    for H, W in PSP_HW:
        for levels in PSP_LEVEL_SETS:
            x, gs, add = case(CAL_N, CAL_C, H, W, levels)
            for k, b in used(levels):
                y, u, _ = fwd64(x, b)
                fwd = max(fwd, _ratio(torch_fwd_fp32(x, b) if form == "torch" else emu_fwd(x, b), y, u))
            dx, unit, _ = bwd64(gs, levels, add, x.shape)
            got = torch_bwd_fp32(gs, levels, add, x.shape) if form == "torch" else emu_bwd(gs, levels, add, x.shape)
            bwd = max(bwd, _ratio(got, dx, unit))
    return fwd, bwd


# =================================================================== device buffers (GPU file) =================================
def sentinel():
    return np.array([SENTINEL_BITS], dtype=np.uint32).view(f32)[0]


def rows_of(t):
    """[N, C, H, W] numpy -> [N * H * W, C] rows"""
    N, C, H, W = t.shape
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1).reshape(N * H * W, C))


def from_rows(r, N, H, W):
    return np.ascontiguousarray(r.reshape(N, H, W, -1).transpose(0, 3, 1, 2))
