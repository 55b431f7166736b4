// Shared by the implicit-GEMM kernels (conv.hip, igemm_ws.hip) and the weight operand planes (operands.hip): gather geometry, bf16 packing, the exact three-piece split.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define BK 32
#define LDP (BK + 4)  // LDS row pitch (floats): 16 B aligned, breaks the 128 B stride

struct ConvGeom {
    int N, Hin, Win, Cin, Hout, Wout, Cout, R, S;
    int mul, off_h, off_w, step, log2div;  // gather: (o*mul + off + r*step) >> log2div
};

// branch-free: returns validity, writes a coordinate that is ALWAYS in [0, lim).
__device__ __forceinline__ bool gather_coord(int base, int tap, int step, int log2div, int lim, int& out) {
    const int v = base + tap * step;
    const int q = v >> log2div;
    const bool ok = (v >= 0) & ((v & ((1 << log2div) - 1)) == 0) & (q < lim);
    out = ok ? q : 0;
    return ok;
}

// WM = wave rows of the block (2: 4 waves / 256 threads; 4: 8 waves / 512 threads with half the rows per wave)
// BF: the A / B tiles are rounded to bf16 (round-to-nearest-even) on their way into LDS and multiplied on the bf16
// matrix cores (v_mfma_f32_32x32x16_bf16, 16x the f32-input rate) with fp32 accumulation -- BASELINE configs[4]
// ("config 5": reduced-precision student, fp32 master weights / EMA teacher).  Tensors in HBM stay fp32.
// BF == 3 ("split fp32"): fp32 products ON THE bf16 MATRIX CORES without giving up fp32 accuracy.  Every operand is split
// exactly into three bf16 pieces x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1): 3 x 8 = 24
// significand bits, both subtractions are exact in fp32) while it is staged into LDS, and a product a.b is accumulated
// in fp32 from the six piece products whose weight is >= 2^-16: a0b0 + a0b1 + a1b0 + a0b2 + a1b1 + a2b0.  The dropped
// terms (a1b2, a2b1, a2b2) are <= 2^-23 |ab| -- the size of ONE fp32 rounding, i.e. of what the fp32 MFMA's own
// accumulation commits K times per output.  Six v_mfma_f32_32x32x16_bf16 (6 x 32 cycles for a 32x32x16 block) replace
// eight v_mfma_f32_32x32x2_f32 (8 x 64 cycles): 2.7x fewer matrix-pipe cycles for the same fp32-class result
// (measured against float64 in tests/test_gpu_conv_stack.py).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
#define LDPH (BK + 8)   // LDS row pitch of the bf16 tiles (elements): 80 B, 16 B aligned
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// two fp32 -> packed bf16 pair (lo in bits 0..15): ONE v_cvt_pk_bf16_f32 on gfx950 (round to nearest even, NaN stays a
// quiet NaN, Inf stays Inf) instead of the 4-5 integer VALU operations per element of an add-and-shift rounding (which
// also turned small-payload NaNs into Inf)
__device__ __forceinline__ unsigned pack2_bf16(float lo, float hi) {
    bf16x2_t v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return *(unsigned*)&v;
}
__device__ __forceinline__ uint2 pack4_bf16(float4 v) { return make_uint2(pack2_bf16(v.x, v.y), pack2_bf16(v.z, v.w)); }
// exact three-way split of four fp32 values into bf16 pieces (see BF == 3 below): v = p0 + p1 + p2 up to 2^-24 |v|
__device__ __forceinline__ float bf16_lo_f(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi_f(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// First piece of the split: bf16(x) with the conversion's overflow taken out -- a FINITE |x| above the largest bf16
// (3.3895e38 <= |x| <= 3.4028e38) would round to +-Inf and the residual x - Inf to NaN; clamped to +-bf16-max first the first
// piece is the largest bf16 and the residual (< 2^120) goes into the other two pieces: the split stays exact for every finite
// fp32 (VERDICT r4 / ADVICE r3).  One v_med3_f32 per value; values inside the bf16 range, +-Inf (first piece bf16-max, residual
// Inf, last piece NaN) and NaN (the residual x - p0 is NaN) behave as before.
#define U2PL_BF16_MAX 3.38953138925153547590e+38f
__device__ __forceinline__ float clamp_bf16(float x) { return __builtin_amdgcn_fmed3f(x, -U2PL_BF16_MAX, U2PL_BF16_MAX); }
__device__ __forceinline__ unsigned pack2_bf16_first(float lo, float hi) { return pack2_bf16(clamp_bf16(lo), clamp_bf16(hi)); }
__device__ __forceinline__ void split3_bf16(float4 v, uint2& p0, uint2& p1, uint2& p2) {
    p0 = make_uint2(pack2_bf16_first(v.x, v.y), pack2_bf16_first(v.z, v.w));
    const float4 r1 = make_float4(v.x - bf16_lo_f(p0.x), v.y - bf16_hi_f(p0.x), v.z - bf16_lo_f(p0.y), v.w - bf16_hi_f(p0.y));
    p1 = pack4_bf16(r1);
    const float4 r2 = make_float4(r1.x - bf16_lo_f(p1.x), r1.y - bf16_hi_f(p1.x), r1.z - bf16_lo_f(p1.y), r1.w - bf16_hi_f(p1.y));
    p2 = pack4_bf16(r2);
}


// ---- "split-fp16" (round 6): fp32 products from THREE fp16 piece products -------------------------------------------------
// An fp32 value scaled by a power of two into the fp16 range is the sum of TWO fp16 pieces to within one fp32 ulp:
// h0 = fp16(x s) carries 11 significant bits (|x s - h0| <= 2^-11 |x s|), the residual is exact in fp32 and h1 = fp16(x s - h0)
// carries 11 bits of IT, so |x s - h0 - h1| <= 2^-23 |x s| -- twice fp32's own rounding bound, unbiased, rms 2^-24.4 (fp32:
// 2^-25.2; tests/test_split_fp32_cpu.py).  A product a b is accumulated in fp32 from a1 b0 + a0 b1 + a0 b0 (the dropped a1 b1 is
// <= 2^-22 |a b|): per term at most ~2^-21 |a b| in the worst case and ~2^-24 |a b| rms, against <= 2^-23 worst / ~2^-25 rms for
// the six-product bf16 form -- both far below what the fp32 ACCUMULATION of a K-term sum commits (sqrt(K) .. K roundings), which
// is why the two forms measure the same against float64 on every layer shape (tools/bench_igemm_wsh.py, tests/test_gpu_igemm_ws.py;
// the fp16 form is usually the closer one).  Three v_mfma_f32_32x32x16_f16 instead of six v_mfma_f32_32x32x16_bf16 per 32x32x16
// block, two piece planes per operand in LDS instead of three.  fp16 has 5 exponent bits, so the operands are scaled PER TENSOR by
// a power of two (exact) chosen from max|x| (split2_exp_bits: the largest magnitude lands in [2^14, 2^15)), and the accumulators
// are scaled back by ldexp in the epilogue (exact).  gfx950's matrix cores and v_cvt_pk_f16_f32 honour fp16 subnormals
// (tools/micro/f16_denorm.hip), so an element far below the tensor's maximum degrades gracefully: its absolute error is <= 2^-25
// in scaled units = 2^-40 max|x|, i.e. elements down to 2^-17 of the maximum keep the accuracy above and no element contributes
// more error than 2^-40 max|x| |b|.  What this gives up against the bf16 form: operands whose elements span more than ~2^26 INSIDE
// one tensor with the small ones mattering (tests/test_gpu_conv_stack.py: the twelve-decade case) -- U2PL_CONV_H=0 selects the
// six-product form for such data.
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned pack2_f16(float lo, float hi) {        // ONE v_cvt_pk_f16_f32 (round to nearest even)
    f16x2_t v;
    v[0] = (_Float16)lo;
    v[1] = (_Float16)hi;
    return *(unsigned*)&v;
}
__device__ __forceinline__ float f16_lo_f(unsigned p) { return (float)(*(f16x2_t*)&p)[0]; }
__device__ __forceinline__ float f16_hi_f(unsigned p) { return (float)(*(f16x2_t*)&p)[1]; }
// power-of-two scale exponent for a tensor whose largest magnitude is amax: amax * 2^e lies in [2^14, 2^15); zero / subnormal
// maxima take the largest scale, Inf / NaN the smallest (the pieces of such elements are Inf / NaN as they should be)
__host__ __device__ static inline int split2_exp_bits(unsigned amax_bits) {
    const int ex = (int)((amax_bits >> 23) & 0xffu);
    const int e = 14 - (ex - 127);
    return e > 126 ? 126 : e;          // (ex = 255 gives -114: a normal scale)
}
__device__ __forceinline__ float split2_scale(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }
// The two pieces of a pair of values in FIVE instructions: written as fused multiply-adds with the power-of-two scale, the
// compiler selects v_fma_mixlo_f16 / v_fma_mixhi_f16 -- fp32 sources, ONE rounding to fp16 -- for "fp16(x s)" and, with the first
// piece as the fp16 addend, for "fp16(x s - h0)" (x s and the residual are exact, so these are the bits of the separate scale /
// convert / subtract / convert sequence: 8 instructions).
__device__ __forceinline__ unsigned split2_first(float lo, float hi, float s) {
    f16x2_t v;
    v[0] = (_Float16)__builtin_fmaf(lo, s, 0.0f);
    v[1] = (_Float16)__builtin_fmaf(hi, s, 0.0f);
    return *(unsigned*)&v;
}
__device__ __forceinline__ unsigned split2_second(float lo, float hi, float s, unsigned h0) {
    const f16x2_t a = *(f16x2_t*)&h0;
    f16x2_t v;
    v[0] = (_Float16)__builtin_fmaf(lo, s, -(float)a[0]);
    v[1] = (_Float16)__builtin_fmaf(hi, s, -(float)a[1]);
    return *(unsigned*)&v;
}
__device__ __forceinline__ void split2_f16(float4 v, float s, uint2& p0, uint2& p1) {
    p0 = make_uint2(split2_first(v.x, v.y, s), split2_first(v.z, v.w, s));
    p1 = make_uint2(split2_second(v.x, v.y, s, p0.x), split2_second(v.z, v.w, s, p0.y));
}

// ---- host side: every ConvGeom is built here, and so is every buffer extent --------------------------------------------------------
// forward: gather o * stride - pad + r * dil
static inline ConvGeom geom_fwd(int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil) {
    return ConvGeom{N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, -pad, -pad, dil, 0};
}
// data gradient: the roles swap (the gathered tensor is dY, Hout x Wout x Cout; the output is dX), gather (i + pad - r * dil) >> log2(stride)
// with a divisibility test.  A stride that is no power of two gives log2div = -1, which geom_ok reports and every GEMM entry refuses.
static inline ConvGeom geom_dgrad(int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil) {
    int l2 = 0;
    while ((1 << l2) < stride) ++l2;
    return ConvGeom{N, Hout, Wout, Cout, Hin, Win, Cin, R, S, 1, pad, pad, -dil, (1 << l2) == stride ? l2 : -1};
}
static inline bool geom_ok(const ConvGeom& g) { return g.log2div >= 0; }
// row-major GEMM Y[M][Nn] = X[M][K] W[Nn][K]^T (one matrix of a batch): a 1x1 forward over an M x 1 map.  Also the geometry of the
// queries that only need channel counts.
static inline ConvGeom geom_gemm(long M, int K, int Nn) { return geom_fwd(1, (int)M, 1, K, (int)M, 1, Nn, 1, 1, 1, 0, 1); }
// batch of weight-gradient GEMMs P_z[Cout][Cin] = dY_z[M][Cout]^T X_z[M][Cin]: the components are the "taps" (R = batch) of an identity
// gather (step = 0, offsets 0)
static inline ConvGeom geom_wgrad_batched(long M, int Cin, int Cout, int batch) { return geom_fwd(1, (int)M, 1, Cin, (int)M, 1, Cout, batch, 1, 1, 0, 0); }
// a planner query: output pixels and channel counts only, no input map
static inline ConvGeom geom_query(int N, int Hout, int Wout, int Cin, int Cout, int R, int S) { return geom_fwd(N, 0, 0, Cin, Hout, Wout, Cout, R, S, 1, 0, 1); }
// bytes spanned by `rows` rows of pitch `ld` floats with `cols` columns in the last one; false at 2 GiB (raw-buffer descriptors, 32-bit offsets)
static inline bool span_bytes(long rows, long ld, long cols, unsigned& bytes) {
    const long b = ((rows - 1) * ld + cols) * 4;
    bytes = (unsigned)b;
    return b < (1L << 31);
}
static inline long geom_rows_in(const ConvGeom& g) { return (long)g.N * g.Hin * g.Win; }
static inline long geom_rows_out(const ConvGeom& g) { return (long)g.N * g.Hout * g.Wout; }
