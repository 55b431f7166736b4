// Depthwise 3x3 convolution (nn.Conv2d(C, C, 3, groups=C): the spatial half of an atrous separable convolution, the layers of a
// separable DeepLabv3+ decoder and of light plug-in encoders) on channels_last rows: forward, data gradient and weight gradient in
// exact fp32 (one product and one add per tap, -ffp-contract=off).  These are stencils, not matrix products: a channel meets only
// its own nine taps, so there is nothing for an MFMA to reduce and every kernel is bound by reading its input once and writing its
// output once.
//
// Tensors: activations [N*H*W][ld] (ld >= C: channel slices of wider buffers work), the weight is the module's own tensor
// (C, 1, 3, 3) = [C][9].  All three kernels read or write THAT layout; there is no derived operand.
//
// Tiling (all three kernels): a lane owns 4 consecutive channels (one 16-byte load per tap), 32 lanes = one channel tile of
// DW_CT = 128 channels = 512 contiguous bytes of a pixel row; the 8 lane groups of a 256-thread block hold 8 consecutive pixels.
// The taps of a pixel are gathered straight from global memory: neighbouring pixels share them through L1 / L2.  Blocks are
// numbered channel tile SLOW, pixels FAST, and the grid is dealt so that each XCD (blocks b, b + 8, ... share one) sweeps one
// contiguous range of that numbering.  Why: at C = 2048 a pixel row is 8 KB and the taps of a dilated layer (d = 12 / 24 / 36 at
// 97 x 97) lie 2 d image rows apart: 24 rows x 97 pixels x 8 KB = 19 MB, far beyond an XCD's 4 MB L2, so a pixel-major sweep
// over whole rows would fetch x from HBM up to three times (once per tap row).  Restricted to one 512-byte channel tile the same
// window is 2 d x 97 x 512 B = 1.2 MB (d = 12) to 3.6 MB (d = 36, where at 97 x 97 most off-centre taps are padding anyway) and
// stays in the sweeping XCD's L2; the price is 512-byte instead of 8 KB contiguous pieces per pixel, still four whole 128-byte
// lines.
//
// Forward / data gradient (k_dwconv<DG>): a thread computes DW_PPT = 4 pixels (pix0 + lane group + 8 i) of its 4 channels; its
// 36 weights stay in registers.  The data gradient is the gather form: dx(h, w) collects dy((h + pad - r d) / s, (w + pad - s d) / s)
// over the taps whose numerators are non-negative multiples of the stride (the parity test), no scatter and no atomics.
//
// Weight gradient (k_dwconv_wgrad + k_dwconv_wgrad_finish): the reduction runs over the N*Ho*Wo pixels, cut into SLABS of
// consecutive pixels.  A block owns one channel tile and one slab: each thread walks the slab's pixels p = s0 + lane group, + 8, ...
// in ascending order with 36 accumulators (4 channels x 9 taps), the 8 lane groups are added through LDS in lane-group order and
// the block writes its [128][9] partial sums to the caller's workspace; the finish kernel adds the slabs in slab order.  No
// floating-point atomics, one fixed order: two runs give the same bits.
#include "common.h"
#include "u2pl_hip.h"

#define DW_CT 128       // channels per tile (32 lanes x 4)
#define DW_PPT 4        // pixels per thread of the forward / data-gradient kernel
#define DW_PB (8 * DW_PPT)

struct DwP {
    long lds, ldd;          // row pitch of the gathered / the written activation
    long M;                 // written pixels (N * Hd * Wd)
    long nblocks, per, pblocks;
    int Hs, Ws, Hd, Wd;     // gathered map, written map
    int C, stride, pad, dil;
};

// consecutive logical blocks on one XCD: hardware block b runs on XCD b % 8 and takes the (b / 8)-th block of that XCD's range
__device__ __forceinline__ long dw_logical_block(long per) { return (long)(blockIdx.x & 7) * per + (blockIdx.x >> 3); }

__device__ __forceinline__ void dw_load_weights(const float* __restrict__ w, int c0, float (&wv)[36]) {
    const float4* q = (const float4*)(w + (long)c0 * 9);       // [4 channels][9 taps], 144 bytes
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float4 v = q[k];
        wv[4 * k] = v.x, wv[4 * k + 1] = v.y, wv[4 * k + 2] = v.z, wv[4 * k + 3] = v.w;
    }
}

template <bool DG>
__global__ __launch_bounds__(256) U2PL_HBM_KERNEL void k_dwconv(const float* __restrict__ src, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ dst,
                                                                const DwP p) {
    const long bid = dw_logical_block(p.per);
    if (bid >= p.nblocks) return;
    const int ct = (int)(bid / p.pblocks);
    const int c0 = ct * DW_CT + (threadIdx.x & 31) * 4;
    if (c0 >= p.C) return;                                      // (C % 4 == 0: the four channels are in or out together)
    long P = (bid - (long)ct * p.pblocks) * DW_PB + (threadIdx.x >> 5);
    if (P >= p.M) return;
    float wv[36];
    dw_load_weights(w, c0, wv);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!DG && bias != nullptr) bv = make_float4(bias[c0], bias[c0 + 1], bias[c0 + 2], bias[c0 + 3]);   // (any alignment)
    const int sh = p.stride - 1;                                // stride is 1 or 2

    const int hw = p.Hd * p.Wd;
    int n = (int)(P / hw);
    const int rem = (int)(P - (long)n * hw);
    int hd = rem / p.Wd, wd = rem - hd * p.Wd;
#pragma unroll
    for (int i = 0; i < DW_PPT; ++i) {
        if (P < p.M) {
            const long nb = (long)n * p.Hs * p.Ws;
            const int bh = DG ? hd + p.pad : hd * p.stride - p.pad;
            const int bw = DG ? wd + p.pad : wd * p.stride - p.pad;
            float4 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r = t / 3, s = t - 3 * r;
                int hi, wi;
                bool ok;
                if (DG) {
                    const int hh = bh - r * p.dil, ww = bw - s * p.dil;
                    ok = hh >= 0 && ww >= 0 && ((hh | ww) & sh) == 0;
                    hi = hh >> sh;
                    wi = ww >> sh;
                    ok = ok && hi < p.Hs && wi < p.Ws;
                } else {
                    hi = bh + r * p.dil;
                    wi = bw + s * p.dil;
                    ok = (unsigned)hi < (unsigned)p.Hs && (unsigned)wi < (unsigned)p.Ws;
                }
                v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) v[t] = *(const float4*)(src + (nb + (long)hi * p.Ws + wi) * p.lds + c0);
            }
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 9; ++t) {                       // taps in (r, s) order; weight of channel j, tap t: wv[9 j + t]
                a.x += v[t].x * wv[t];
                a.y += v[t].y * wv[9 + t];
                a.z += v[t].z * wv[18 + t];
                a.w += v[t].w * wv[27 + t];
            }
            if (!DG && bias != nullptr) a.x += bv.x, a.y += bv.y, a.z += bv.z, a.w += bv.w;
            *(float4*)(dst + P * p.ldd + c0) = a;
        }
        P += 8;
        wd += 8;
        while (wd >= p.Wd) {
            wd -= p.Wd;
            if (++hd >= p.Hd) hd = 0, ++n;
        }
    }
}

// the convolution's output extent along one axis, or -1
static inline int dw_out(int n, int stride, int pad, int dil) {
    const long num = (long)n + 2L * pad - 2L * dil - 1;
    return num < 0 ? -1 : (int)(num / stride + 1);
}

static bool dwconv_args_ok(const void* a, long lda, const void* b, long ldb, const void* w, int N, int Hin, int Win, int Cin, int Hout,
                           int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups) {
    if (N < 1 || Hin < 1 || Win < 1 || Cin < 1 || pad < 0 || dil < 1) return false;
    if (groups != Cin || Cout != Cin) return false;                         // depthwise, depth multiplier 1
    if (Cin % 4) return false;
    if (R != 3 || S != 3) return false;
    if (stride != 1 && stride != 2) return false;
    if (pad > (1 << 20) || dil > (1 << 20)) return false;                   // tap coordinates stay far inside an int
    if (Hout != dw_out(Hin, stride, pad, dil) || Wout != dw_out(Win, stride, pad, dil)) return false;
    if (Hout < 1 || Wout < 1) return false;
    if ((long)N * Hin * Win >= (1L << 31) - 256 || (long)N * Hout * Wout >= (1L << 31) - 256) return false;
    if (lda < Cin || ldb < Cout || lda % 4 || ldb % 4) return false;        // 16-byte row loads
    if (a == nullptr || b == nullptr || w == nullptr) return false;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)w) & 15) return false;
    return true;
}

template <bool DG>
static int dwconv_launch(const float* src, const float* w, const float* bias, float* dst, DwP p, hipStream_t stream) {
    p.pblocks = (p.M + DW_PB - 1) / DW_PB;
    p.nblocks = p.pblocks * ((p.C + DW_CT - 1) / DW_CT);
    p.per = (p.nblocks + 7) / 8;
    if (p.per * 8 >= (1L << 31)) return U2PL_EINVAL;
    U2PL_LAUNCH((k_dwconv<DG>), dim3((unsigned)(p.per * 8)), dim3(256), 0, stream, src, w, bias, dst, p);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API int u2pl_dwconv2d_fwd_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N, int Hin,
                                   int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                                   int groups, hipStream_t stream) {
    if (!dwconv_args_ok(x, ldx, y, ldy, w, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    DwP p = {};
    p.lds = ldx, p.ldd = ldy, p.M = (long)N * Hout * Wout;
    p.Hs = Hin, p.Ws = Win, p.Hd = Hout, p.Wd = Wout;
    p.C = Cin, p.stride = stride, p.pad = pad, p.dil = dil;
    return dwconv_launch<false>(x, w, bias, y, p, stream);
}

U2PL_API int u2pl_dwconv2d_dgrad_f32(const float* dy, long lddy, const float* w, float* dx, long lddx, int N, int Hin, int Win, int Cin,
                                     int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups,
                                     hipStream_t stream) {
    if (!dwconv_args_ok(dx, lddx, dy, lddy, w, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    DwP p = {};
    p.lds = lddy, p.ldd = lddx, p.M = (long)N * Hin * Win;
    p.Hs = Hout, p.Ws = Wout, p.Hd = Hin, p.Wd = Win;
    p.C = Cin, p.stride = stride, p.pad = pad, p.dil = dil;
    return dwconv_launch<true>(dy, w, nullptr, dx, p, stream);
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
struct DwWgradP {
    long lddy, ldx, M, rows;        // rows: pixels per slab
    long nblocks, per;
    int Hin, Win, Hout, Wout;
    int C, stride, pad, dil;
    int tiles, NS;                  // channel tiles, slabs
};

// slab plan, shared by the workspace query and the launcher: about 2048 blocks, at least 64 pixels per slab, at most 512 slabs
static void dwwgrad_plan(DwWgradP& p) {
    p.tiles = (p.C + DW_CT - 1) / DW_CT;
    long ns = (2048 + p.tiles - 1) / p.tiles;
    const long cap = (p.M + 63) / 64;
    if (ns > cap) ns = cap;
    if (ns > 512) ns = 512;
    if (ns < 1) ns = 1;
    p.rows = (p.M + ns - 1) / ns;
    p.NS = (int)((p.M + p.rows - 1) / p.rows);
    p.nblocks = (long)p.tiles * p.NS;
    p.per = (p.nblocks + 7) / 8;
}

__global__ __launch_bounds__(256) U2PL_HBM_KERNEL void k_dwconv_wgrad(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      float* __restrict__ part, const DwWgradP p) {
    __shared__ float red[8][36][32];
    const long bid = dw_logical_block(p.per);
    if (bid >= p.nblocks) return;                               // (whole block)
    const int ct = (int)(bid / p.NS), slab = (int)(bid - (long)ct * p.NS);
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int c0 = ct * DW_CT + lane * 4;
    const bool cv = c0 < p.C;
    const long s0 = (long)slab * p.rows;
    const long s1 = s0 + p.rows < p.M ? s0 + p.rows : p.M;

    float acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.f;
    long P = s0 + grp;
    if (cv && P < s1) {
        const int hw = p.Hout * p.Wout;
        int n = (int)(P / hw);
        const int rem = (int)(P - (long)n * hw);
        int ho = rem / p.Wout, wo = rem - ho * p.Wout;
        for (; P < s1; P += 8) {
            const float4 g = *(const float4*)(dy + P * p.lddy + c0);
            const long nb = (long)n * p.Hin * p.Win;
            const int bh = ho * p.stride - p.pad, bw = wo * p.stride - p.pad;
            float4 v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r = t / 3, s = t - 3 * r;
                const int hi = bh + r * p.dil, wi = bw + s * p.dil;
                v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((unsigned)hi < (unsigned)p.Hin && (unsigned)wi < (unsigned)p.Win)
                    v[t] = *(const float4*)(x + (nb + (long)hi * p.Win + wi) * p.ldx + c0);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                acc[t] += g.x * v[t].x;
                acc[9 + t] += g.y * v[t].y;
                acc[18 + t] += g.z * v[t].z;
                acc[27 + t] += g.w * v[t].w;
            }
            wo += 8;
            while (wo >= p.Wout) {
                wo -= p.Wout;
                if (++ho >= p.Hout) ho = 0, ++n;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 36; ++k) red[grp][k][lane] = acc[k];
    __syncthreads();
    // element (lane, k) = channel ct * 128 + 4 lane + k / 9, tap k % 9: the lane's 36 values are contiguous in [C][9]
    const long E = (long)p.C * 9;
    for (int o = threadIdx.x; o < 36 * 32; o += 256) {
        const int k = o >> 5, l = o & 31;
        if (ct * DW_CT + l * 4 >= p.C) continue;
        float s = red[0][k][l];
#pragma unroll
        for (int gq = 1; gq < 8; ++gq) s += red[gq][k][l];      // fixed order: lane group 0, 1, ...
        part[(long)slab * E + ((long)ct * DW_CT + l * 4) * 9 + k] = s;
    }
}

__global__ __launch_bounds__(256) void k_dwconv_wgrad_finish(const float* __restrict__ part, int NS, long E, int accumulate,
                                                             float* __restrict__ dw) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < E; i += (long)gridDim.x * 256) {
        float s = part[i];
        for (int k = 1; k < NS; ++k) s += part[(long)k * E + i];      // fixed order: slab 0, 1, ...
        dw[i] = accumulate ? dw[i] + s : s;
    }
}

U2PL_API size_t u2pl_dwconv2d_wgrad_workspace_bytes(int N, int Hout, int Wout, int Cin, int Cout, int R, int S, int groups) {
    if (N < 1 || Hout < 1 || Wout < 1 || Cin < 1 || groups != Cin || Cout != Cin || R != 3 || S != 3) return 0;
    DwWgradP p = {};
    p.M = (long)N * Hout * Wout, p.C = Cin;
    dwwgrad_plan(p);
    return (size_t)p.NS * Cin * 9 * sizeof(float);
}

U2PL_API int u2pl_dwconv2d_wgrad_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace, int accumulate,
                                     int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                                     int dil, int groups, hipStream_t stream) {
    if (!dwconv_args_ok(x, ldx, dy, lddy, dw, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    if (workspace == nullptr) return U2PL_EINVAL;
    DwWgradP p = {};
    p.M = (long)N * Hout * Wout, p.C = Cin;
    p.Hin = Hin, p.Win = Win, p.Hout = Hout, p.Wout = Wout;
    p.stride = stride, p.pad = pad, p.dil = dil;
    p.lddy = lddy, p.ldx = ldx;
    dwwgrad_plan(p);
    if (p.per * 8 >= (1L << 31)) return U2PL_EINVAL;
    float* part = (float*)workspace;
    U2PL_LAUNCH(k_dwconv_wgrad, dim3((unsigned)(p.per * 8)), dim3(256), 0, stream, dy, x, part, p);
    U2PL_LAUNCH_CHECK();
    const long E = (long)Cin * 9;
    U2PL_LAUNCH(k_dwconv_wgrad_finish, dim3(grid_for(E, 256)), dim3(256), 0, stream, part, p.NS, E, accumulate, dw);
    U2PL_LAUNCH_CHECK();
    return 0;
}
