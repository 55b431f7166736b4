// csrc/wgrad_tr.hip: split-fp32 weight gradient with hardware-transposed LDS operand reads (see there).
#pragma once
#include "conv_geom.h"

// one weight-gradient call (every kernel family of conv.hip and wgrad_tr.hip): dY and X rows, the slabs, the geometry (taps = R * S; a
// batched call passes its components as taps, zdy / zx floats apart), the stream and, for split-fp16 (three products), the device-scalar
// maxima of the two operands (both NULL: six bf16 piece products)
struct WgradCall {
    const float* dy; long lddy; const float* x; long ldx; float* part; ConvGeom g; hipStream_t stream; long zdy, zx;
    const float *dy_amax, *x_amax;
};
// slabs of the pixel range: ctiles = Cin tiles, nsplit slabs of cps 32-pixel chunks each
struct WgradSlabs { int ctiles, nsplit, cps; };

// both operand extents of a weight-gradient launch; false: one of them reaches 2 GiB
static inline bool wgrad_extents(const WgradCall& c, unsigned& dyb, unsigned& xb) {
    return span_bytes(geom_rows_out(c.g), c.lddy, c.g.Cout, dyb) && span_bytes(geom_rows_in(c.g), c.ldx, c.g.Cin, xb);
}

bool wgrad_tr_eligible(const ConvGeom& g);
WgradSlabs wgrad_tr_plan(const ConvGeom& g);
int launch_wgrad_tr(const WgradCall& c, const WgradSlabs& s);
