"""The weight operand planes of the pre-split GEMMs, written down a second time: pure torch on the CPU, no project imports.

A buffer holds, for each of `batch` fp32 matrices [rows][K] (K % 32 == 0), NP piece planes per 32-deep chunk:

    [batch][chunk = K / 32][piece][Np][32]      16-bit elements

Np = rows padded with zero rows to 128, or above 128 to a multiple of 256.  Element k = 32 c + 8 s + q of row n lies in chunk c at
position 8 * (s ^ ((n >> 2) & 3)) + q of the row: the four 16-byte segments of a row are XOR-swizzled with bits 2..3 of the row.

  split3_planes: NP = 3 bf16 pieces.  p0 = bf16(clamp(x, +-bf16max)), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1); the residuals are
    exact in fp32.
  split2h_planes: NP = 2 fp16 pieces of x * 2^e, e = min(14 - (exponent(amax) - 127), 126) with amax = max |w| of the matrix:
    h0 = fp16(x s), h1 = fp16(x s - h0).  Behind the planes of ALL matrices: one 32-bit word per matrix, the fp32 bit pattern of its
    amax, then zero words up to a multiple of 16 bytes.

Conversions round to nearest even and keep fp16 subnormals.  x s and x s - h0 are exact in fp32 (a power-of-two scale; the
residual of an 11-bit rounding), so two separate roundings give the bits of the fused multiply-add-and-convert a kernel may use.
Finite inputs only."""
import torch

BF16_MAX = 3.38953138925153547590e+38


def pad_rows(rows):
    return 128 if rows <= 128 else (rows + 255) & ~255


def _planes(pieces, rows, K):
    """pieces: [NP] int16 tensors [batch][rows][K] -> int16 [batch][K / 32][NP][Np][32] in the swizzled layout"""
    batch, Np, C = pieces[0].shape[0], pad_rows(rows), K // 32
    p = torch.zeros(batch, len(pieces), Np, C, 4, 8, dtype=torch.int16)
    for i, x in enumerate(pieces):
        p[:, i, :rows] = x.reshape(batch, rows, C, 4, 8)
    # slot d of row n holds segment d ^ ((n >> 2) & 3) (the XOR is its own inverse)
    seg = torch.arange(4)[None, :] ^ ((torch.arange(Np)[:, None] >> 2) & 3)     # [Np][4]
    out = torch.gather(p, 4, seg[None, None, :, None, :, None].expand_as(p))
    return out.permute(0, 3, 1, 2, 4, 5).contiguous()                           # [batch][C][NP][Np][4][8]


def _check(w):
    assert w.dtype == torch.float32 and w.dim() == 3 and w.shape[2] % 32 == 0 and bool(torch.isfinite(w).all())
    return w.detach().cpu().contiguous()


def split3_planes(w):
    """fp32 [batch][rows][K] -> uint8: the bytes of a u2pl_weight_split3_bytes(rows, K, batch) buffer"""
    w = _check(w)
    p0 = w.clamp(-BF16_MAX, BF16_MAX).to(torch.bfloat16)
    r1 = w - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    return _planes([p.view(torch.int16) for p in (p0, p1, p2)], w.shape[1], w.shape[2]).reshape(-1).view(torch.uint8)


def split2h_planes(w):
    """fp32 [batch][rows][K] -> uint8: the bytes of a u2pl_weight_split2h_bytes(rows, K, batch) buffer"""
    w = _check(w)
    batch = w.shape[0]
    amax = w.abs().reshape(batch, -1).max(dim=1).values.view(torch.int32)       # bit patterns of max |w|
    e = (14 - (((amax >> 23) & 0xff) - 127)).clamp(max=126)
    s = ((e + 127) << 23).view(torch.float32)[:, None, None]
    xs = w * s
    h0 = xs.to(torch.float16)
    h1 = (xs - h0.float()).to(torch.float16)
    planes = _planes([h.view(torch.int16) for h in (h0, h1)], w.shape[1], w.shape[2]).reshape(-1).view(torch.uint8)
    tail = torch.zeros((batch * 4 + 15) // 16 * 4, dtype=torch.int32)
    tail[:batch] = amax
    return torch.cat([planes, tail.view(torch.uint8)])
