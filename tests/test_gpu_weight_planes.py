"""The weight operand planes -- bf16 (u2pl_weight_split3_f32) and fp16 with their maxima (u2pl_weight_split2h_f32) -- decoded against
tests/plane_ref.py, a pure-torch statement of the format: every byte of the buffer (pieces, swizzle, zero padding rows, maxima words,
the zero tail) with torch.equal.  The operands are built through the C entry points of the lazy path: on the weight as it lies, on
the output of u2pl_weight_transpose_f32 and on the output of u2pl_wino_weight_f32 (the fp32 U from the GPU is the reference's input:
the transform itself is held to float64 by tests/test_gpu_wino_stages.py).  The batched rebuild is held to the lazy path's bytes by
tests/test_gpu_presplit_taps.py, non-finite weights by its test_maxima_edge_cases."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _data(shape, seed):
    """randn * 0.05, each element scaled by a random power of two in 2^-30 .. 1 (fp16 subnormals and zeros in the first pieces, second
    and third pieces at every magnitude); every 97th element exactly zero"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * 0.05 * torch.exp2(-torch.randint(0, 31, shape, generator=g).float())
    w.reshape(-1)[::97] = 0.0
    return w


def _weights(Cout, RS, Cin, seed):
    """three weights [Cout][RS][Cin]: mixed magnitudes, all zero (maximum word 0, the largest scale), largest magnitude negative"""
    w = _data((3, Cout, RS, Cin), seed)
    w[1].zero_()
    w[2, Cout // 2, RS - 1, 3] = -1.5 * float(w[2].abs().max())
    assert float(w[2].min()) < 0 and float(w[2].max()) < -float(w[2].min())
    return w


def _split(which, src, rows, K, batch):
    """src: device fp32 [batch][rows][K] -> the buffer the one-weight entry point writes (pre-filled: every byte must be written)"""
    from u2pl_amd._lib import call, query
    nbytes = query("u2pl_weight_%s_bytes" % which, rows, K, batch)
    buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    call("u2pl_weight_%s_f32" % which, src, rows * K, rows, K, batch, buf)
    torch.cuda.synchronize()
    return buf.cpu()


def _check(which, src, rows, K, batch):
    assert src.is_contiguous() and src.numel() == batch * rows * K
    got = _split(which, src, rows, K, batch)
    want = getattr(plane_ref, which + "_planes")(src.cpu().reshape(batch, rows, K))
    assert got.numel() == want.numel()
    assert torch.equal(got, want), "%d bytes differ, first at %d" % (int((got != want).sum()), int((got != want).nonzero()[0]))


# Cout, Cin, k: rows 96 -> 128 with ONE chunk; rows 160 -> 256 (transposed: 64 -> 128, K = 1440); rows 288 -> 512, the widest padding
SHAPES = [(96, 32, 1), (160, 64, 3), (288, 96, 3)]


@pytest.mark.parametrize("which", ["split3", "split2h"])
@pytest.mark.parametrize("Cout,Cin,k", SHAPES)
def test_planes_of_the_weight_as_it_lies(which, Cout, Cin, k):
    w = _weights(Cout, k * k, Cin, 11).to(DEV)
    _check(which, w, Cout, k * k * Cin, 3)


@pytest.mark.parametrize("which", ["split3", "split2h"])
@pytest.mark.parametrize("Cout,Cin,k", SHAPES)
def test_planes_of_the_transposed_weight(which, Cout, Cin, k):
    from u2pl_amd._lib import call
    w = _weights(Cout, k * k, Cin, 12).to(DEV)
    wT = torch.empty(3, Cin, k * k * Cout, dtype=torch.float32, device=DEV)
    for z in range(3):
        call("u2pl_weight_transpose_f32", w[z], wT[z], Cout, k * k, Cin)
    assert torch.equal(wT, w.permute(0, 3, 2, 1).reshape(3, Cin, k * k * Cout))         # [Cin][rs * Cout + co]
    _check(which, wT, Cin, k * k * Cout, 3)


@pytest.mark.parametrize("which", ["split3", "split2h"])
@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("mt", [4, 2])
def test_planes_of_the_winograd_filters(which, transposed, mt):
    """batched matrices: (mt + 2)^2 components U[z][rows][K] of a 96 <- 32 3x3 weight, one of them zeroed, one given a negative
    largest magnitude"""
    from u2pl_amd._lib import call
    Cout, Cin, a2 = 96, 32, (mt + 2) ** 2
    w = _data((Cout, 9, Cin), 13).to(DEV)
    rows, K = (Cin, Cout) if transposed else (Cout, Cin)
    U = torch.empty(a2, rows, K, dtype=torch.float32, device=DEV)
    call("u2pl_wino_weight_f32", w, Cout, Cin, transposed, mt, U)
    U[5].zero_()
    U[7, rows // 2, 3] = -1.5 * float(U[7].abs().max())
    assert bool(torch.isfinite(U).all()) and float(U.abs().max()) > 0
    _check(which, U, rows, K, a2)
