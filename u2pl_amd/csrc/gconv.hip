// Grouped convolution (nn.Conv2d(groups > 1): the 3x3 of a ResNeXt bottleneck, reference resnet.py:25-36 / :108-112) on
// channels_last rows: forward, data gradient and weight gradient in exact fp32 (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain
// with fp32 accumulation).  No split-fp16 / bf16 product forms here: a grouped layer carries 1/groups of a dense layer's
// multiplies and is bound by reading x once and writing y once.
//
// Tensors: activations [N*H*W][ld] (ld >= C: channel slices of wider buffers work), the weight is the module's own tensor
// (Cout, Cin/groups, R, S) stored channels_last = [Cout][R][S][Cin/groups].  All three kernels read THAT tensor: the data gradient
// swaps the per-group channel roles and mirrors the taps in its addressing, so there is no derived operand to keep current.
//
// Forward / data gradient (k_gconv<JT, DG>): one wave computes 32 output pixels x all output channels of ONE group
// (JT = ceil(channels / 16) column tiles of a 16x16 MFMA tile, 2 row tiles).  The reduction index of a group, (tap, channel), is
// cut into UNITS of 4 consecutive channels (one 16-byte load): the four k-lanes of the 16x16x4 instruction hold four consecutive
// units and the four components of the loaded float4 feed four MFMAs, so any Cin/groups that is a multiple of 4 fills the k
// dimension (4 channels x 9 taps = 9 units = 3 steps, the last one 1/4 full) without a per-width kernel.  Weights are streamed
// per step from L2 / L1 (per-group weights are up to 147 KB: they do not fit LDS beside anything); the input is gathered
// straight from global memory -- the nine taps of a pixel and the groups of a row share cache lines, the block order keeps the
// groups of one pixel block on one XCD's L2.
//
// Weight gradient (k_gconv_wgrad<NT>): the reduction runs over the N*Ho*Wo pixels (k-lanes = 4 consecutive pixels), one wave owns
// a 16 (out channels) x 16 (in channels) tile of one group for NT taps and one SLAB of pixels and writes its partial sums to the
// caller's workspace; k_gconv_wgrad_finish adds the slabs in slab order.  No floating-point atomics: two runs give the same bits.
#include "common.h"
#include "u2pl_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define GCONV_DIV_SHIFT 20
// floor(u / d) = (u * ceil(2^20 / d)) >> 20, exact for u < 2^20 / d, d <= 16 (host checks R * S * units < 2048)
__device__ __forceinline__ int gdiv(int u, unsigned magic) { return (int)(((unsigned)u * magic) >> GCONV_DIV_SHIFT); }
static inline unsigned gmagic(int d) { return (unsigned)(((1u << GCONV_DIV_SHIFT) + d - 1) / d); }

struct GConvP {
    long lds, ldd;          // row pitch of the gathered / the written activation
    long M;                 // written pixels (N * Hd * Wd)
    long nblocks;
    int Hs, Ws, Hd, Wd;     // gathered map, written map
    int RS, S, stride, pad, dil, groups;
    int cs, cd;             // channels per group on the gathered / the written side
    int cig;                // the weight's innermost extent (Cin / groups)
    int U;                  // reduction units = RS * cs / 4
    unsigned m_cu, m_S;     // division magics: units per tap, S
    int remap;
};

template <int JT, bool DG>
__global__ __launch_bounds__(256) void k_gconv(const float* __restrict__ src, const float* __restrict__ w,
                                               const float* __restrict__ bias, float* __restrict__ dst, const GConvP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    long bid = blockIdx.x;
    if (p.remap) {          // consecutive logical blocks (the groups of one pixel block) on one XCD
        const long per = p.nblocks >> 3;
        bid = (bid & 7) * per + (bid >> 3);
    }
    const int g = (int)(bid % p.groups);
    const long pix0 = (bid / p.groups) * 128 + wave * 32;
    if (pix0 >= p.M) return;
    const int cu = p.cs >> 2;
    const int sh = p.stride - 1;            // stride is 1 or 2

    int bh[2], bw[2], nb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long P = pix0 + t * 16 + li;
        if (P < p.M) {
            const int hw = p.Hd * p.Wd;
            const int n = (int)(P / hw), rem = (int)(P - (long)n * hw);
            const int hd = rem / p.Wd, wd = rem - hd * p.Wd;
            nb[t] = n * p.Hs * p.Ws;
            bh[t] = DG ? hd + p.pad : hd * p.stride - p.pad;
            bw[t] = DG ? wd + p.pad : wd * p.stride - p.pad;
        } else {
            nb[t] = 0;
            bh[t] = bw[t] = -(1 << 24);     // every tap out of the map
        }
    }
    f32x4 acc[2][JT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < JT; ++j) acc[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const float* wg = w + (long)g * (DG ? p.cs : p.cd) * p.RS * p.cig;      // this group's [cog][RS][cig] block
    for (int u0 = 0; u0 < p.U; u0 += 4) {
        const int u = u0 + lk;
        const bool uv = u < p.U;
        const int tap = gdiv(u, p.m_cu), cc = u - tap * cu;
        const int r = gdiv(tap, p.m_S), s = tap - r * p.S;
        float4 a[2], b[JT];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            int hi, wi;
            bool ok;
            if (DG) {
                const int hh = bh[t] - r * p.dil, ww = bw[t] - s * p.dil;
                ok = uv && hh >= 0 && ww >= 0 && ((hh | ww) & sh) == 0;
                hi = hh >> sh;
                wi = ww >> sh;
                ok = ok && hi < p.Hs && wi < p.Ws;
            } else {
                hi = bh[t] + r * p.dil;
                wi = bw[t] + s * p.dil;
                ok = uv && (unsigned)hi < (unsigned)p.Hs && (unsigned)wi < (unsigned)p.Ws;
            }
            a[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) a[t] = *(const float4*)(src + (long)(nb[t] + hi * p.Ws + wi) * p.lds + g * p.cs + 4 * cc);
        }
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int oc = j * 16 + li;
            b[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (uv && oc < p.cd) {
                if (DG) {   // w[out = 4cc + m][tap][in = oc]: the forward's weight with the channel roles swapped
                    const float* q = wg + ((long)(4 * cc) * p.RS + tap) * p.cig + oc;
                    const long st = (long)p.RS * p.cig;
                    b[j] = make_float4(q[0], q[st], q[2 * st], q[3 * st]);
                } else {    // w[out = oc][tap][in = 4cc .. 4cc + 3]
                    b[j] = *(const float4*)(wg + (long)oc * p.RS * p.cig + 4 * u);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, b[j].x, acc[t][j], 0, 0, 0);
                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, b[j].y, acc[t][j], 0, 0, 0);
                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, b[j].z, acc[t][j], 0, 0, 0);
                acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, b[j].w, acc[t][j], 0, 0, 0);
            }
    }
    // accumulator tile: column (channel) = lane & 15, row (pixel) = 4 * (lane >> 4) + register
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        const int oc = j * 16 + li;
        if (oc >= p.cd) continue;
        const float bv = (!DG && bias != nullptr) ? bias[g * p.cd + oc] : 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long P = pix0 + t * 16 + lk * 4 + e;
                if (P < p.M) dst[P * p.ldd + g * p.cd + oc] = (!DG && bias != nullptr) ? acc[t][j][e] + bv : acc[t][j][e];
            }
    }
}

static bool gconv_args_ok(const void* a, long lda, const void* b, long ldb, const void* w, int N, int Hin, int Win, int Cin, int Hout,
                          int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups) {
    if (groups < 1 || N < 1 || Hin < 1 || Win < 1 || Cin < 1 || Cout < 1 || R < 1 || S < 1 || pad < 0 || dil < 1) return false;
    if (Cin % groups || Cout % groups) return false;
    const int cig = Cin / groups, cog = Cout / groups;
    if (cig % 4 || cog % 4 || cig > 64 || cog > 64) return false;
    if (stride != 1 && stride != 2) return false;
    if ((long)R * S * 16 >= 2048 || S > 16) return false;                   // range of the division magics
    if (Hout != (Hin + 2 * pad - dil * (R - 1) - 1) / stride + 1 || Wout != (Win + 2 * pad - dil * (S - 1) - 1) / stride + 1) return false;
    if (Hout < 1 || Wout < 1) return false;
    if ((long)N * Hin * Win >= (1L << 31) - 256 || (long)N * Hout * Wout >= (1L << 31) - 256) return false;
    if (lda < Cin || ldb < Cout || lda % 4 || ldb % 4) return false;       // 16-byte row loads
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)w) & 15) return false;
    if (a == nullptr || b == nullptr || w == nullptr) return false;
    return true;
}

template <bool DG>
static int gconv_launch(const float* src, const float* w, const float* bias, float* dst, GConvP p, hipStream_t stream) {
    const long pblocks = (p.M + 127) / 128;
    p.nblocks = pblocks * p.groups;
    if (p.nblocks >= (1L << 31)) return U2PL_EINVAL;
    p.remap = (p.nblocks % 8 == 0) ? 1 : 0;
    p.U = p.RS * (p.cs / 4);
    p.m_cu = gmagic(p.cs / 4);
    p.m_S = gmagic(p.S);
    const dim3 grid((unsigned)p.nblocks), block(256);
    switch ((p.cd + 15) / 16) {
        case 1: U2PL_LAUNCH((k_gconv<1, DG>), grid, block, 0, stream, src, w, bias, dst, p); break;
        case 2: U2PL_LAUNCH((k_gconv<2, DG>), grid, block, 0, stream, src, w, bias, dst, p); break;
        case 3: U2PL_LAUNCH((k_gconv<3, DG>), grid, block, 0, stream, src, w, bias, dst, p); break;
        default: U2PL_LAUNCH((k_gconv<4, DG>), grid, block, 0, stream, src, w, bias, dst, p); break;
    }
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API int u2pl_gconv2d_fwd_f32(const float* x, long ldx, const float* w, const float* bias, float* y, long ldy, int N, int Hin,
                                  int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                                  int groups, hipStream_t stream) {
    if (!gconv_args_ok(x, ldx, y, ldy, w, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    GConvP p = {};
    p.lds = ldx, p.ldd = ldy, p.M = (long)N * Hout * Wout;
    p.Hs = Hin, p.Ws = Win, p.Hd = Hout, p.Wd = Wout;
    p.RS = R * S, p.S = S, p.stride = stride, p.pad = pad, p.dil = dil, p.groups = groups;
    p.cs = Cin / groups, p.cd = Cout / groups, p.cig = Cin / groups;
    return gconv_launch<false>(x, w, bias, y, p, stream);
}

U2PL_API int u2pl_gconv2d_dgrad_f32(const float* dy, long lddy, const float* w, float* dx, long lddx, int N, int Hin, int Win, int Cin,
                                    int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil, int groups,
                                    hipStream_t stream) {
    if (!gconv_args_ok(dx, lddx, dy, lddy, w, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    GConvP p = {};
    p.lds = lddy, p.ldd = lddx, p.M = (long)N * Hin * Win;
    p.Hs = Hout, p.Ws = Wout, p.Hd = Hin, p.Wd = Win;
    p.RS = R * S, p.S = S, p.stride = stride, p.pad = pad, p.dil = dil, p.groups = groups;
    p.cs = Cout / groups, p.cd = Cin / groups, p.cig = Cin / groups;
    return gconv_launch<true>(dy, w, nullptr, dx, p, stream);
}

// ---- weight gradient ---------------------------------------------------------------------------------------------------------
struct GWgradP {
    long lddy, ldx, M, rows;        // rows: pixels per slab (a multiple of 4)
    int Hin, Win, Hout, Wout;
    int RS, S, stride, pad, dil, groups, cig, cog, Cout;
    int JT, CT, ntc, NS;            // tiles over cog / cig, tap chunks, slabs
    unsigned m_S;
    long nwaves;
};

// slab plan, shared by the workspace query and the launcher: enough waves to fill the device, at least 64 pixels per slab
static void gwgrad_plan(GWgradP& p) {
    p.JT = (p.cog + 15) / 16, p.CT = (p.cig + 15) / 16;
    p.ntc = (p.RS == 9 || p.RS == 1) ? 1 : p.RS;
    const long tiles = (long)p.groups * p.JT * p.CT * p.ntc;
    long ns = (8192 + tiles - 1) / tiles;
    const long cap = (p.M + 63) / 64;
    if (ns > cap) ns = cap;
    if (ns > 512) ns = 512;
    if (ns < 1) ns = 1;
    long rows = (p.M + ns - 1) / ns;
    rows = (rows + 3) / 4 * 4;
    p.rows = rows;
    p.NS = (int)((p.M + rows - 1) / rows);
    p.nwaves = tiles * p.NS;
}

template <int NT>
__global__ __launch_bounds__(256) void k_gconv_wgrad(const float* __restrict__ dy, const float* __restrict__ x,
                                                     float* __restrict__ part, const GWgradP p) {
    const int lane = threadIdx.x & 63;
    const int li = lane & 15, lk = lane >> 4;
    long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= p.nwaves) return;
    const int per_slab = p.groups * p.JT * p.CT * p.ntc;
    const int slab = (int)(wid / per_slab);
    int rest = (int)(wid - (long)slab * per_slab);
    const int tc = rest % p.ntc;
    rest /= p.ntc;
    const int ct = rest % p.CT;
    rest /= p.CT;
    const int jt = rest % p.JT;
    const int g = rest / p.JT;
    const int tap0 = tc * NT;

    const long s0 = (long)slab * p.rows;
    const long s1 = s0 + p.rows < p.M ? s0 + p.rows : p.M;
    const int oc = jt * 16 + li, ic = ct * 16 + li;
    const bool ocv = oc < p.cog, icv = ic < p.cig;
    const float* dyc = dy + g * p.cog + oc;
    const float* xc = x + g * p.cig + ic;

    int rr[NT], ss[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int r = gdiv(tap0 + t, p.m_S);
        rr[t] = r * p.dil - p.pad;
        ss[t] = (tap0 + t - r * p.S) * p.dil - p.pad;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // this lane's pixel walks s0 + lk, + 4, ...: decoded once, then advanced without divisions
    long P = s0 + lk;
    const int hw = p.Hout * p.Wout;
    int n = (int)(P / hw);
    int rem = (int)(P - (long)n * hw);
    int ho = rem / p.Wout, wo = rem - ho * p.Wout;
    for (; P - lk < s1; P += 4) {
        const bool pv = P < s1;
        const float a = (pv && ocv) ? dyc[P * p.lddy] : 0.f;
        const int hb = ho * p.stride, wb = wo * p.stride;
        const long nbase = (long)n * p.Hin * p.Win;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int hi = hb + rr[t], wi = wb + ss[t];
            float b = 0.f;
            if (pv && icv && (unsigned)hi < (unsigned)p.Hin && (unsigned)wi < (unsigned)p.Win)
                b = xc[(nbase + (long)hi * p.Win + wi) * p.ldx];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
        }
        wo += 4;
        while (wo >= p.Wout) {
            wo -= p.Wout;
            if (++ho >= p.Hout) ho = 0, ++n;
        }
    }
    // tile: column (in channel) = lane & 15, row (out channel) = 4 * (lane >> 4) + register
    if (icv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = jt * 16 + lk * 4 + e;
            if (o >= p.cog) continue;
            float* q = part + (((long)slab * p.Cout + g * p.cog + o) * p.RS + tap0) * p.cig + ic;
#pragma unroll
            for (int t = 0; t < NT; ++t) q[(long)t * p.cig] = acc[t][e];
        }
    }
}

__global__ __launch_bounds__(256) void k_gconv_wgrad_finish(const float* __restrict__ part, int NS, long E, int accumulate,
                                                            float* __restrict__ dw) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < E; i += (long)gridDim.x * 256) {
        float s = part[i];
        for (int k = 1; k < NS; ++k) s += part[(long)k * E + i];      // fixed order: slab 0, 1, ...
        dw[i] = accumulate ? dw[i] + s : s;
    }
}

static bool gwgrad_fill(GWgradP& p, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                        int dil, int groups) {
    if (groups < 1 || Cin < 1 || Cout < 1 || R < 1 || S < 1 || Cin % groups || Cout % groups) return false;
    p.M = (long)N * Hout * Wout;
    p.Hin = Hin, p.Win = Win, p.Hout = Hout, p.Wout = Wout;
    p.RS = R * S, p.S = S, p.stride = stride, p.pad = pad, p.dil = dil, p.groups = groups;
    p.cig = Cin / groups, p.cog = Cout / groups, p.Cout = Cout;
    p.m_S = gmagic(S);
    if (p.M < 1) return false;
    gwgrad_plan(p);
    return true;
}

U2PL_API size_t u2pl_gconv2d_wgrad_workspace_bytes(int N, int Hout, int Wout, int Cin, int Cout, int R, int S, int groups) {
    GWgradP p = {};
    if (!gwgrad_fill(p, N, 0, 0, Cin, Hout, Wout, Cout, R, S, 1, 0, 1, groups)) return 0;
    return (size_t)p.NS * Cout * p.RS * p.cig * sizeof(float);
}

U2PL_API int u2pl_gconv2d_wgrad_f32(const float* dy, long lddy, const float* x, long ldx, float* dw, void* workspace, int accumulate,
                                    int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad,
                                    int dil, int groups, hipStream_t stream) {
    if (!gconv_args_ok(x, ldx, dy, lddy, dw, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    if (workspace == nullptr) return U2PL_EINVAL;
    GWgradP p = {};
    if (!gwgrad_fill(p, N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil, groups)) return U2PL_EINVAL;
    p.lddy = lddy, p.ldx = ldx;
    const long blocks = (p.nwaves + 3) / 4;
    if (blocks >= (1L << 31)) return U2PL_EINVAL;
    float* part = (float*)workspace;
    if (p.ntc == 1 && p.RS == 9)
        U2PL_LAUNCH((k_gconv_wgrad<9>), dim3((unsigned)blocks), dim3(256), 0, stream, dy, x, part, p);
    else
        U2PL_LAUNCH((k_gconv_wgrad<1>), dim3((unsigned)blocks), dim3(256), 0, stream, dy, x, part, p);
    U2PL_LAUNCH_CHECK();
    const long E = (long)Cout * p.RS * p.cig;
    U2PL_LAUNCH(k_gconv_wgrad_finish, dim3(grid_for(E, 256)), dim3(256), 0, stream, part, p.NS, E, accumulate, dw);
    U2PL_LAUNCH_CHECK();
    return 0;
}
