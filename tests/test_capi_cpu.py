"""CPU-only checks of the drop-in boundary: the C-ABI library loads without a
GPU and exports every symbol include/u2pl_hip.h declares; product ops refuse
CPU tensors (no silent fallback)."""
import ctypes
import os

import pytest
import torch

from u2pl_amd import _lib


def test_library_exports_every_declared_symbol():
    decls = _lib.parse_header()
    assert len(decls) >= 26
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in decls:
        assert hasattr(cdll, name), name


def test_size_queries_run_without_gpu():
    L = _lib.lib()
    assert L.u2pl_select_workspace_bytes() > 0
    assert L.u2pl_infonce_job_bytes() == 56
    assert L.u2pl_ce_workspace_bytes() > 0


def test_no_cpu_fallback():
    from u2pl_amd import hipops as H

    with pytest.raises(_lib.HipError):
        H.bilinear_up(torch.zeros(1, 2, 3, 3), (5, 5))
    with pytest.raises(_lib.HipError):
        H.cross_entropy(torch.zeros(1, 2, 3, 3), torch.zeros(1, 3, 3, dtype=torch.long))


def test_product_never_imports_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for d, _, files in os.walk(os.path.join(root, "u2pl_amd")):
        for f in files:
            if f.endswith(".py"):
                s = open(os.path.join(d, f)).read()
                # any mention at all: also catches importlib.import_module("oracle...") / __import__ / sys.path games
                if "oracle" in s or "/root/reference" in s or "ref_shim" in s:
                    bad.append(os.path.join(d, f))
    assert not bad, bad


def test_winograd_layer_policy():
    """nn.wino_tile: only stride-1 'same' 3x3 layers with MFMA-friendly channel counts, and only where tile
    padding leaves a worthwhile multiply reduction (ASPP d=24 on a 97x97 map does not)."""
    from u2pl_amd import nn as K
    saved = dict(K.CONV_ALGO)
    try:
        K.CONV_ALGO.update(wino=4, min_gain=1.7)
        assert K.wino_tile(256, 256, 3, 3, 1, 2, 2, 97, 97) == 4          # layer3
        assert K.wino_tile(2048, 256, 3, 3, 1, 12, 12, 97, 97) == 4       # ASPP d=12
        assert K.wino_tile(2048, 256, 3, 3, 1, 24, 24, 97, 97) == 0       # 5x5 sub-images: padding eats the gain
        assert K.wino_tile(128, 128, 3, 3, 2, 1, 1, 193, 193) == 0        # strided
        assert K.wino_tile(256, 1024, 1, 1, 1, 0, 1, 97, 97) == 0         # 1x1
        assert K.wino_tile(3, 64, 3, 3, 1, 1, 1, 385, 385) == 0           # stem: Cin % 32
        assert K.wino_tile(256, 19, 3, 3, 1, 1, 1, 97, 97) == 0           # narrow head
        K.CONV_ALGO.update(wino=0)
        assert K.wino_tile(256, 256, 3, 3, 1, 2, 2, 97, 97) == 0
        K.CONV_ALGO.update(wino=2, min_gain=1.7)
        assert K.wino_tile(256, 256, 3, 3, 1, 1, 1, 193, 193) == 2
    finally:
        K.CONV_ALGO.update(saved)


def test_winograd_statistics_rows_and_refusals_need_no_gpu():
    """u2pl_wino_stat_blocks: rows of the statistics partials, 256 / (O/4) tiles per block; 0 for O < 4 (it used to divide by
    O / 4 = 0 there).  The Winograd entry points refuse a shape before any launch -- so also without a device: statistics on
    O < 4 or O > 1024, and a row pitch that is not a multiple of 4 floats (16-byte accesses), like u2pl_absmax_f32."""
    L = _lib.lib()
    assert L.u2pl_wino_stat_blocks(27, 256) == 7 and L.u2pl_wino_stat_blocks(28, 256) == 7
    assert L.u2pl_wino_stat_blocks(32, 304) == 11           # 76 float4 columns: 3 tiles per block
    assert L.u2pl_wino_stat_blocks(4, 1024) == 4 and L.u2pl_wino_stat_blocks(512, 4) == 2
    for O in (0, 1, 2, 3):
        assert L.u2pl_wino_stat_blocks(100, O) == 0
    EINVAL = 1001
    for O in (2, 1028):
        assert L.u2pl_wino_output_f32(None, 1, 4, 4, O, 1, 4, None, None, 1028, 1, None, None) == EINVAL      # (stats != NULL)
    for name in ("u2pl_wino_input_f32", "u2pl_wino_gy_f32"):
        for ld in (9, 10, 11):
            assert getattr(L, name)(None, ld, 1, 4, 4, 8, 1, 4, None, None) == EINVAL
    for name in ("u2pl_wino_input_amax_f32", "u2pl_wino_gy_amax_f32"):
        assert getattr(L, name)(None, 10, 1, 4, 4, 8, 1, 2, None, None, None) == EINVAL
    assert L.u2pl_wino_output_f32(None, 1, 4, 4, 8, 1, 4, None, None, 10, None, None, None) == EINVAL
    assert L.u2pl_absmax_f32(None, 10, 4, 8, None, 0, None) == EINVAL


def test_conv_arithmetic_switch_and_statistics_block_count():
    """u2pl_conv_set_split / u2pl_conv_get_split (host state, no GPU needed) and the planner query that sizes the fused
    BatchNorm-statistics partials: in the split form every launch is ONE grid of 128-row body tiles (no tail launch), with
    the fp32 instruction the planner adds a tail of smaller tiles for the partial last round -- the Python layer sizes its
    partial buffer with this query right before the launch, so the two must always agree with the launcher."""
    L = _lib.lib().cdll
    old = L.u2pl_conv_get_split()
    try:
        assert L.u2pl_conv_set_split(1) == old and L.u2pl_conv_get_split() == 1
        M = 4 * 97 * 97                                     # 37636 pixels: 295 body tiles of 128 rows
        assert L.u2pl_conv2d_fwd_stat_blocks(4, 97, 97, 256) == -(-M // 128)
        assert L.u2pl_conv2d_fwd_stat_blocks(4, 97, 97, 64) == -(-M // 128)      # Cout <= 64: the single-launch shape
        assert L.u2pl_conv_set_split(0) == 1 and L.u2pl_conv_get_split() == 0
        if not os.environ.get("U2PL_IGEMM_TAIL"):
            n = L.u2pl_conv2d_fwd_stat_blocks(4, 97, 97, 256)
            assert n >= -(-M // 128)                         # body tiles in whole rounds + smaller tail tiles
    finally:
        L.u2pl_conv_set_split(old)
