"""Stage-level contract of the Winograd transform kernels of u2pl_amd/csrc/wino.hip: float64 references in the kernels' memory
layouts, an element-wise error bound per stage, and a numpy fp32 emulation of each kernel.  Shared by tests/test_wino_stages_cpu.py
(emulation against reference, faulty emulations against the bound) and tests/test_gpu_wino_stages.py (the kernels against the same
reference and bound).  Not a conftest: imported by name, like split_bounds.py.

Layouts (a = mt + 2, tile id t = (((n dil + py) dil + px) Ty + ty) Tx + tx, Ty = ceil(ceil(H / dil) / mt), Tx likewise):

    V  [a a][tiles][C] = B^T d B          d: the a x a input tile of the zero-padded polyphase sub-image (py, px)
    Mg [a a][tiles][O] = A g A^T          g: the mt x mt tile of the output gradient, zero beyond the map
    U  [a a][O][C]     = G w G^T          U' [a a][C][O]: the same of the taps rotated by 180 degrees (`transposed`)
    y  [N H W][ldy]    = A^T M A + bias   written only inside the map (then the eval BatchNorm epilogue, residual, ReLU)
    dw [O][3][3][C]    = G^T (sum of slabs) G (+ dw)       slabs [nsplit][O][a a][C]

Bound.  Every stage is two 1-D passes L . R of straight-line fp32 code (csrc/wino_t.h; the build uses -ffp-contract=off, so each
written operation is one rounding, and a multiplication by a power of two is none).  If every term c_i t_i of an output passes
through at most k roundings, the output's first-order error is at most k 2^-24 sum |c_i| |t_i|; a first pass of k1 and a second of
k2 roundings give (k1 + k2) 2^-24 (|L| |t| |R|) per element, plus second-order terms for which ONE unit is added (HEADROOM).  The
constants 1/6, 1/12, 1/24 are fp32 roundings of the float64 reference's constants: one rounding each where they are used.

k per 1-D pass, the longest chain of each function of WinoT<4> / WinoT<2>, line by line:

  bt (B^T d), F(4x4): p = d4 + (-4 d2): 1; q likewise: 1; s = d4 - d2: 1; t = 2 (d3 - d1): 1 (the doubling is exact)
      r0 = (4 d0 + (-5 d2)) + d4: d2 passes -5 d2 (1), the first sum (1), the second (1)                         -> 3
      r1 = p + q, r2 = p - q, r3 = s + t, r4 = s - t: 1 + 1                                                      -> 2
      r5 = (4 d1 + (-5 d3)) + d5: as r0                                                                          -> 3     bt = 3
  bt, F(2x2): every output is one difference or sum                                                                        bt = 1
  av (A v), F(4x4): e = v0 + v2: 1; o = v1 + v3: 1; e4 = v0 + 4 v2: 1; o4 = 2 v1 + 8 v3: 1
      r0 = v0, r5 = v3: 0;  r1 = e + o, r2 = e - o, r3 = e4 + o4, r4 = e4 - o4: 1 + 1                            -> 2     av = 2
  av, F(2x2): r0 = v0: 0; r1 = v0 + v1, r2 = v0 - v1: 1; r3 = -v1: 0                                                       av = 1
  at (A^T m), F(4x4): s12, d12, s34, d34: 1 each
      y0 = (m0 + s12) + s34: s12 passes its own sum (1) and both additions (2)                                   -> 3
      y1 = d12 + 2 d34, y2 = s12 + 4 s34: 1 + 1                                                                  -> 2
      y3 = (d12 + 8 d34) + m5: 1 + 1 + 1                                                                         -> 3     at = 3
  at, F(2x2): y0 = (m0 + m1) + m2, y1 = (m1 - m2) - m3: 2                                                                  at = 2
  gg (G g), F(4x4): a = (g0 + g2) (-1/6): the sum (1), the constant (1), the product (1) = 3; b = g1 (1/6): constant + product = 2
      c = g0 (1/24) + g2 (1/6): constant (1), product (1), sum (1) = 3; e = g1 (1/12): 2
      r0 = g0 / 4, r5 = g2: 0;  r1 = a - b, r2 = a + b, r3 = c + e, r4 = c - e: 3 + 1                            -> 4     gg = 4
  gg, F(2x2): r1 = ((g0 + g2) + g1) / 2, r2 likewise: 2 (the constants 1/2 are exact)                                      gg = 2
  gt (G^T v), F(4x4): s12 = v1 + v2: 1; s34 = v3 + v4: 1
      r0 = (v0 / 4 - s12 (1/6)) + s34 (1/24): s12 passes its sum (1), the constant (1), the product (1), both additions (2) -> 5
      r1 = (v2 - v1) (1/6) + (v3 - v4) (1/12): difference, constant, product, sum                                -> 4
      r2 = (s34 - s12) (1/6) + v5: s12's sum (1), the difference (1), constant (1), product (1), sum (1)         -> 5     gt = 5
  gt, F(2x2): r0 = v0 + (v1 + v2) / 2, r2 = (v1 + v2) / 2 + v3: 2; r1 = (v1 - v2) / 2: 1                                   gt = 2

What follows a transform adds roundings on its own condition: the bias 1 (on |A^T| |M| |A| + |bias|); the eval BatchNorm epilogue
((v - mean) invstd gamma + beta: C_EPI = 4, + 1 with a residual, as bn_bounds counts k_bn_apply) on (cond_v + |mean|) |invstd
gamma| + |beta| + |res| (ReLU is 1-Lipschitz); the ordered slab sum nsplit - 1; accumulate 1 (on cond + |dw before|).  A bound is
therefore (k + HEADROOM) 2^-24 cond per element with k = the sum of the stage's roundings; where cond is 0 the output must be
exactly 0.  No constant is fitted to a measured error: tests/test_wino_stages_cpu.py shows that the bounds reject a transform that
rounds G's constants or one pass to bf16.

The emulations (emu_*) restate each kernel with its own index arithmetic (tile decode by % and /, flat pixel index, the in-image
tests) in numpy fp32, one numpy operation per written operation; the references use split_bounds' unfold-based tiles in float64.
The two are written independently so that each checks the other.  `fault` selects the deliberately wrong variants of the CPU test."""
import numpy as np
import torch

from split_bounds import C_EPI, EPS, _lr, _out_tiles, _tiles, _untile, operands, wino_mats

F32 = np.float32
K_PASS = {4: dict(bt=3, av=2, at=3, gg=4, gt=5), 2: dict(bt=1, av=1, at=2, gg=2, gt=2)}
HEADROOM = 1
SENTINEL_BYTE = 0xA5
SENTINEL = np.array([0xA5A5A5A5], dtype=np.uint32).view(F32)[0]        # what a float of 0xA5 bytes reads as (-2.87e-16)

# ---- the shape lists of both test files -------------------------------------------------------------------------------------------
# (N, H, W, C, dil) of the input / gy / output transforms; thread counts tiles C/4 at mt = 4 / mt = 2:
#   (1,1,1,4,1) 1 / 1 and (1,4,4,4,1) 1 / 4: maps of at most one tile; (1,5,7,12,1) 12 / 36: below one wave; (3,9,11,64,1) 432 / 1440:
#   several blocks, no multiple of 64; (2,9,11,20,2) 160 / 360; (2,10,7,8,3) 36 / 144; (1,9,11,64,12) 2304 / 2304 = 9 x 256 with
#   dil > H (phases without a pixel); (2,5,13,8,1) 16 / 84: N > 1 with Ty != Tx at both tile sizes (the others have Ty == Tx at mt = 4)
GEOMS = [(1, 1, 1, 4, 1), (1, 4, 4, 4, 1), (1, 5, 7, 12, 1), (3, 9, 11, 64, 1), (2, 9, 11, 20, 2), (2, 10, 7, 8, 3), (1, 9, 11, 64, 12),
         (2, 5, 13, 8, 1)]
MTS = (4, 2)
KINDS = ("relu_heavy_tail", "six_decade_rows", "cancellation", "zeros")
WEIGHT_SHAPES = [(1, 1), (4, 4), (12, 20), (96, 32), (5, 300)]
FINISH_SHAPES = [(1, 4), (5, 20), (64, 64)]
NSPLITS = (1, 2, 7)
# statistics: (N, H, W, O, dil, mt); tiles-per-block tpb = 256 / (O/4) = 256, 21 (4 idle threads), 4, 3 (28 idle), 1; per O one
# case whose tile count is a multiple of tpb and one whose last block misses tiles (tpb = 1 has no such case)
STAT_CASES = [(2, 32, 32, 4, 1, 2), (1, 5, 7, 4, 1, 2), (2, 12, 28, 48, 1, 4), (2, 9, 11, 48, 2, 4), (2, 9, 11, 256, 2, 4),
              (3, 9, 11, 256, 1, 4), (3, 9, 11, 304, 1, 4), (2, 9, 11, 304, 2, 2), (1, 5, 7, 1024, 1, 4), (1, 4, 4, 1024, 1, 2)]


def geom(N, H, W, dil, mt):
    """-> Ty, Tx, tiles"""
    Ty, Tx = -(-(-(-H // dil)) // mt), -(-(-(-W // dil)) // mt)
    return Ty, Tx, N * dil * dil * Ty * Tx


def stat_tpb(O):
    return max(1, 256 // (O // 4))


def rows(kind, M, C, seed):
    """float32 [M][C] of the data kinds: split_bounds.operands' activation operand, or `zeros`: half the elements exactly zero, half
    of those -0.0"""
    if kind == "zeros":
        rng = np.random.default_rng(seed)
        a = rng.standard_normal((M, C)).astype(F32)
        u = rng.random((M, C))
        a[u < 0.5] = 0.0
        a[u < 0.25] = -0.0
        return a
    return operands(kind, M, C + (C & 1), 1, seed)[0][:, :C].copy()


def weights(shape, seed):
    """tests/test_gpu_weight_planes._data: randn * 0.05 scaled by a random power of two in 2^-30 .. 1, every 97th element zero"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * 0.05 * torch.exp2(-torch.randint(0, 31, shape, generator=g).float())
    w.reshape(-1)[::97] = 0.0
    return w.numpy()


# ---- float64 references and bounds -------------------------------------------------------------------------------------------------
def _t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _planes(T, N):
    """[N][C][T][a][a] -> [a a][N T][C]"""
    _, C, Tn, a, _ = T.shape
    return T.permute(3, 4, 0, 2, 1).reshape(a * a, N * Tn, C).numpy()


def ref_input(x, N, H, W, C, dil, mt):
    """x [N H W][C] -> V [a a][tiles][C] float64 and its bound"""
    BT = wino_mats(mt)[0]
    d, _ = _tiles(_t64(x).reshape(N, H, W, C).permute(0, 3, 1, 2), dil, mt)
    k = 2 * K_PASS[mt]["bt"] + HEADROOM
    return _planes(_lr(BT, d, BT.T), N), k * EPS * _planes(_lr(BT.abs(), d.abs(), BT.abs().T), N)


def ref_gy(gy, N, H, W, O, dil, mt):
    """gy [N H W][O] -> Mg [a a][tiles][O] float64 and its bound"""
    AT = wino_mats(mt)[2]
    g = _out_tiles(_t64(gy).reshape(N, H, W, O).permute(0, 3, 1, 2), dil, mt)
    k = 2 * K_PASS[mt]["av"] + HEADROOM
    return _planes(_lr(AT.T, g, AT), N), k * EPS * _planes(_lr(AT.abs().T, g.abs(), AT.abs()), N)


def ref_weight(w, transposed, mt):
    """w [O][3][3][C] -> U [a a][O][C] (transposed: U' [a a][C][O] of the rotated taps) float64 and its bound"""
    G = wino_mats(mt)[1]
    g = _t64(w).permute(0, 3, 1, 2)                                  # [O][C][3][3]
    if transposed:
        g = g.flip(2, 3).transpose(0, 1)                             # [C][O][3][3]
    a = mt + 2
    out = lambda u: u.permute(2, 3, 0, 1).reshape(a * a, u.shape[0], u.shape[1]).numpy()     # noqa: E731
    k = 2 * K_PASS[mt]["gg"] + HEADROOM
    return out(_lr(G, g, G.T)), k * EPS * out(_lr(G.abs(), g.abs(), G.abs().T))


def tile_of_pixel(N, H, W, dil, mt):
    """[N H W] tile id of each output pixel, from the pixel's coordinates (independent of the kernels' decode)"""
    Ty, Tx, _ = geom(N, H, W, dil, mt)
    n, oy, ox = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing="ij")
    return ((((n * dil + oy % dil) * dil + ox % dil) * Ty + oy // dil // mt) * Tx + ox // dil // mt).reshape(-1)


def ref_output(Mb, N, H, W, O, dil, mt, bias=None, bn=None, res=None, relu=0):
    """Mb [a a][tiles][O] -> y [N H W][O] float64 and its bound.  bn = (mean, invstd, gamma, beta) [O] each; res [N H W][O]"""
    AT = wino_mats(mt)[2]
    a = mt + 2
    Ty, Tx, tiles = geom(N, H, W, dil, mt)
    M = _t64(Mb).reshape(a, a, N, tiles // N, O).permute(2, 4, 3, 0, 1)          # [N][O][T][a][a]
    geo = (N, H, W, dil, mt, Ty, Tx)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(N * H * W, O).numpy()        # noqa: E731
    y, cond = nhwc(_untile(_lr(AT, M, AT.T), geo)), nhwc(_untile(_lr(AT.abs(), M.abs(), AT.abs().T), geo))
    k = 2 * K_PASS[mt]["at"] + HEADROOM
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        y, cond, k = y + b, cond + np.abs(b), k + 1
    if bn is not None:
        mu, iv, ga, be = (np.asarray(v, dtype=np.float64) for v in bn)
        y, cond, k = (y - mu) * iv * ga + be, (cond + np.abs(mu)) * np.abs(iv * ga) + np.abs(be), k + C_EPI
        if res is not None:
            r = np.asarray(res, dtype=np.float64)
            y, cond, k = y + r, cond + np.abs(r), k + 1
        if relu:
            y = np.maximum(y, 0.0)
    return y, k * EPS * cond


def ref_finish(part, mt, dw0=None):
    """part [nsplit][O][a a][C] -> dw [O][3][3][C] float64 (+ dw0: accumulate) and its bound"""
    G = wino_mats(mt)[1]
    a = mt + 2
    p = _t64(part)
    ns, O, _, C = p.shape
    u = lambda s: s.reshape(O, a, a, C).permute(0, 3, 1, 2)                     # noqa: E731
    back = lambda t: t.permute(0, 2, 3, 1).numpy()                              # noqa: E731
    dw, cond = back(_lr(G.T, u(p.sum(0)), G)), back(_lr(G.abs().T, u(p.abs().sum(0)), G.abs()))
    k = (ns - 1) + 2 * K_PASS[mt]["gt"] + HEADROOM
    if dw0 is not None:
        d0 = np.asarray(dw0, dtype=np.float64)
        dw, cond, k = dw + d0, cond + np.abs(d0), k + 1
    return dw, k * EPS * cond


def ref_stats(y, pivot, N, H, W, O, dil, mt, L):
    """the statistics partials [nblk][2][O] of the STORED y [N H W][O] (float32): float64 column sums of y - pivot and its square
    over each block's tpb tiles, and their bounds L 2^-24 sum |d|, (L + 2) 2^-24 sum d^2 (bn_bounds: L roundings per term, the
    square two more)"""
    tpb = stat_tpb(O)
    blk = tile_of_pixel(N, H, W, dil, mt) // tpb
    nblk = -(-geom(N, H, W, dil, mt)[2] // tpb)
    d = np.asarray(y, dtype=np.float64) - (0.0 if pivot is None else np.asarray(pivot, dtype=np.float64))
    out = np.zeros((4, nblk, O))
    for i, v in enumerate((d, d * d, np.abs(d), d * d)):
        np.add.at(out[i], blk, v)
    ref = np.stack((out[0], out[1]), 1)
    return ref, np.stack((L * EPS * out[2], (L + 2) * EPS * out[3]), 1)


def stage_excess(got, ref, bound, written=None):
    """largest |got - ref| / bound over the elements `written` marks (default: all); inf if one of them is not finite, or if an
    element outside `written` no longer holds the sentinel the buffer was filled with"""
    got = np.asarray(got)
    if written is not None:
        if not np.array_equal(got[~written].view(np.uint32), np.full(int((~written).sum()), SENTINEL).view(np.uint32)):
            return float("inf")
        got, ref, bound = got[written], ref[written], bound[written]
    if not np.isfinite(got).all():
        return float("inf")
    if got.size == 0:
        return 0.0
    return float((np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)).max())


# ---- fp32 emulation ----------------------------------------------------------------------------------------------------------------
def bf16(a):
    """round-to-nearest-even to bf16, kept in float32"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def _consts(fault):
    c = [F32(1) / F32(6), F32(1) / F32(12), F32(1) / F32(24)]
    return [bf16(np.array([v]))[0] for v in c] if fault == "g_bf16" else c


def _bt(mt, d):
    if mt == 2:
        return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    p, q = d[4] + F32(-4) * d[2], d[3] + F32(-4) * d[1]
    s, t = d[4] - d[2], F32(2) * (d[3] - d[1])
    return [(F32(4) * d[0] + F32(-5) * d[2]) + d[4], p + q, p - q, s + t, s - t, (F32(4) * d[1] + F32(-5) * d[3]) + d[5]]


def _at(mt, m):
    if mt == 2:
        return [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]
    s12, d12, s34, d34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return [(m[0] + s12) + s34, d12 + F32(2) * d34, s12 + F32(4) * s34, (d12 + F32(8) * d34) + m[5]]


def _av(mt, v):
    if mt == 2:
        return [v[0], v[0] + v[1], v[0] - v[1], F32(-1) * v[1]]
    e, o = v[0] + v[2], v[1] + v[3]
    e4, o4 = v[0] + F32(4) * v[2], F32(2) * v[1] + F32(8) * v[3]
    return [v[0], e + o, e - o, e4 + o4, e4 - o4, v[3]]


def _gt(mt, v, fault=None):
    if mt == 2:
        return [v[0] + F32(0.5) * (v[1] + v[2]), F32(0.5) * (v[1] - v[2]), F32(0.5) * (v[1] + v[2]) + v[3]]
    c6, c12, c24 = _consts(fault)
    s12, s34 = v[1] + v[2], v[3] + v[4]
    return [v[0] * F32(0.25) - s12 * c6 + s34 * c24, (v[2] - v[1]) * c6 + (v[3] - v[4]) * c12, (s34 - s12) * c6 + v[5]]


def _gg(mt, g, fault=None):
    if mt == 2:
        return [g[0], F32(0.5) * ((g[0] + g[2]) + g[1]), F32(0.5) * ((g[0] + g[2]) - g[1]), g[2]]
    c6, c12, c24 = _consts(fault)
    a, b = (g[0] + g[2]) * -c6, g[1] * c6
    c, e = g[0] * c24 + g[2] * c6, g[1] * c12
    return [g[0] * F32(0.25), a - b, a + b, c + e, c - e, g[2]]


def _two_pass(first, second, d, n_in, n_mid, fault):
    """d[i][j], i, j < n_in -> out[i][j]: `first` down the columns (n_in -> n_mid), then `second` along the rows"""
    t = [[None] * n_in for _ in range(n_mid)]
    for j in range(n_in):
        r = first([d[i][j] for i in range(n_in)])
        for i in range(n_mid):
            t[i][j] = bf16(r[i]) if fault == "pass_bf16" else r[i]
    return [second(t[i]) for i in range(n_mid)]


def _decode(tiles, Ty, Tx, dil, fault):
    """tile_coords of every tile id"""
    t = np.arange(tiles, dtype=np.int64)
    txd = Ty if fault == "ty_for_tx" else Tx
    tx = t % txd; t = t // txd          # noqa: E702
    ty = t % Ty; t = t // Ty            # noqa: E702
    px = t % dil; t = t // dil          # noqa: E702
    py = t % dil
    n = t // dil
    if fault == "swap_phase":
        py, px = px, py
    return n, py, px, ty, tx


def _gather(buf, C, N, H, W, n, iy, ix, fault):
    """rows (n H + iy) W + ix of buf [rows][ld], columns < C; zeros outside the image (the buffer load's out-of-range offset)"""
    edge = 1 if fault == "edge_inside" else 0
    ok = (iy >= 0) & (iy < H + edge) & (ix >= 0) & (ix < W + edge)
    pix = np.clip((n * H + iy) * W + ix, 0, buf.shape[0] - 1)       # (the clip only matters to the faulty variants)
    return np.where(ok[:, None], buf[pix, :C], F32(0))


def _behind(buf, W):
    """the faulty variants that read or write behind the last pixel get W + 1 more rows to do it in"""
    return np.concatenate([buf, np.full((W + 1, buf.shape[1]), F32(3))])


def emu_input(x, N, H, W, C, dil, mt, fault=None):
    """k_wino_input: x [>= N H W][ldx] float32 -> V [a a][tiles][C] float32"""
    a = mt + 2
    Ty, Tx, tiles = geom(N, H, W, dil, mt)
    n, py, px, ty, tx = _decode(tiles, Ty, Tx, dil, fault)
    x = _behind(x, W) if fault == "edge_inside" else x
    iy0, ix0 = py + dil * (ty * mt - 1), px + dil * (tx * mt - 1)
    d = [[_gather(x, C, N, H, W, n, iy0 + i * dil, ix0 + j * dil, fault) for j in range(a)] for i in range(a)]
    bt = lambda v: _bt(mt, v)       # noqa: E731
    r = _two_pass(bt, bt, d, a, a, fault)
    return np.stack([r[i][j] for i in range(a) for j in range(a)])


def emu_gy(gy, N, H, W, O, dil, mt, fault=None):
    """k_wino_gy: gy [>= N H W][ldg] float32 -> Mg [a a][tiles][O] float32"""
    a = mt + 2
    Ty, Tx, tiles = geom(N, H, W, dil, mt)
    n, py, px, ty, tx = _decode(tiles, Ty, Tx, dil, fault)
    gy = _behind(gy, W) if fault == "edge_inside" else gy
    v = [[_gather(gy, O, N, H, W, n, py + dil * (ty * mt + i), px + dil * (tx * mt + j), fault) for j in range(mt)] for i in range(mt)]
    av = lambda c: _av(mt, c)       # noqa: E731
    r = _two_pass(av, av, v, mt, a, fault)
    return np.stack([r[i][j] for i in range(a) for j in range(a)])


def emu_weight(w, transposed, mt, fault=None):
    """k_wino_weight: w [O][3][3][C] float32 -> U [a a][O][C], or U' [a a][C][O] of the rotated taps"""
    a = mt + 2
    rot = transposed and fault != "no_rotation"
    gk = [[w[:, 2 - r if rot else r, 2 - s if rot else s, :] for s in range(3)] for r in range(3)]
    gg = lambda c: _gg(mt, c, fault)     # noqa: E731
    t = [[None] * 3 for _ in range(a)]
    for s in range(3):
        r = gg([gk[0][s], gk[1][s], gk[2][s]])
        for i in range(a):
            t[i][s] = bf16(r[i]) if fault == "pass_bf16" else r[i]
    U = np.stack([c for i in range(a) for c in gg(t[i])])
    return np.ascontiguousarray(U.transpose(0, 2, 1)) if transposed else U


def emu_output(Mb, N, H, W, O, dil, mt, bias=None, ldy=None, bn=None, res=None, relu=0, stats=False, pivot=None, fault=None):
    """k_wino_output: Mb [a a][tiles][O] float32 -> y [N H W][ldy] in a sentinel-filled buffer (and the statistics partials
    [nblk][2][O] with stats=True).  res: [N H W][ldr]"""
    a = mt + 2
    ldy = ldy or O
    Ty, Tx, tiles = geom(N, H, W, dil, mt)
    n, py, px, ty, tx = _decode(tiles, Ty, Tx, dil, fault)
    edge = 1 if fault == "edge_inside" else 0
    y = np.full((N * H * W + (W + 1) * edge, ldy), SENTINEL, dtype=F32)
    m = [[Mb[i * a + j] for j in range(a)] for i in range(a)]
    at = lambda c: _at(mt, c)       # noqa: E731
    r = _two_pass(at, at, m, a, mt, fault)
    bv = np.zeros(O, dtype=F32) if bias is None else np.asarray(bias, dtype=F32)
    pv = np.zeros(O, dtype=F32) if pivot is None else np.asarray(pivot, dtype=F32)
    s1, s2 = np.zeros((tiles, O), dtype=F32), np.zeros((tiles, O), dtype=F32)
    for i in range(mt):
        oy = py + dil * (ty * mt + i)
        for j in range(mt):
            ox = px + dil * (tx * mt + j)
            ok = (oy < H + edge) & (ox < W + edge)
            if fault == "ty_for_tx":
                ok &= n < N
            pix = ((n * H + oy) * W + ox)[ok]
            v = r[i][j][ok] + (np.zeros(O, dtype=F32) if fault == "bias_outside" else bv)
            if bn is not None:
                mu, iv, ga, be = (np.asarray(t, dtype=F32) for t in bn)
                v = (v - mu) * iv * ga + be
                if res is not None:
                    v = v + res[pix, :O]
                if relu:
                    v = np.maximum(v, F32(0))
            y[pix, :O] = v
            dv = v - pv
            s1[ok] = s1[ok] + dv
            s2[ok] = s2[ok] + dv * dv
    if not stats:
        return y
    tpb = stat_tpb(O)
    nblk = -(-tiles // tpb)
    part = np.zeros((nblk, 2, O), dtype=F32)
    for tl in range(tpb):
        t = np.arange(nblk) * tpb + tl
        live = t < tiles
        part[live, 0] = part[live, 0] + s1[t[live]]
        part[live, 1] = part[live, 1] + s2[t[live]]
    return y, part


def emu_finish(part, mt, accumulate=0, dw0=None, fault=None):
    """k_wino_wgrad_finish: part [nsplit][O][a a][C] float32 -> dw [O][3][3][C] float32 (dw0: what dw held before)"""
    a = mt + 2
    ns, O, _, C = part.shape
    if fault == "drop_last_slab":
        ns -= 1
    u = np.zeros((O, a * a, C), dtype=F32)
    for z in range(ns):
        u = u + part[z]
    gt = lambda c: _gt(mt, c, fault)     # noqa: E731
    r = _two_pass(gt, gt, [[u[:, i * a + j, :] for j in range(a)] for i in range(a)], a, 3, fault)
    dw = np.stack([np.stack([r[r3][s3] for s3 in range(3)], 1) for r3 in range(3)], 1)        # [O][3][3][C]
    if accumulate and fault != "no_accumulate":
        dw = np.asarray(dw0, dtype=F32) + dw
    return dw
