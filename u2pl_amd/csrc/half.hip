// fp16 prediction path (eval-mode forward with fp16 activations and fp16 weights in HBM):
//   u2pl_half_weight_f16      fp32 [Cout][Cin][R][S] -> fp16 [Cout][R][S][Cin], round to nearest even
//   u2pl_hconv2d_fwd_f16      dense convolution as an implicit GEMM on v_mfma_f32_32x32x16_f16, fp32 accumulation,
//                             fp32 epilogue (scale, shift, residual, ReLU), ONE rounding to fp16 (or fp32 output)
//   u2pl_hconv2d_stem_f16     direct form for a few input channels, reading the fp32 normalised image (the stem)
//   u2pl_hmaxpool3s2_f16      MaxPool2d(3, 2, 1, ceil_mode=True)
//   u2pl_hgap_f16             global average, fp32 sums
//   u2pl_hbilinear_f16        bilinear(align_corners=True): ac_coord + the three-FMA expression of k_bilinear_up
// Activations are NHWC rows of fp16 with a pitch (elements), so channel slices of concat buffers are read and written
// in place.  A value whose magnitude exceeds 65504 is stored as +-65504 and counted into an int32 of the caller's (an
// integer atomicAdd per wave: the count feeds no floating-point result, outputs are bit-identical from run to run).
#include "common.h"
#include "u2pl_hip.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float hacc16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16;

#define H_MAX 65504.0f
#define H_BK 32            // K chunk (fp16 elements): one 64-byte row segment
#define H_LDP 40           // LDS row pitch (fp16 elements): 80 bytes, 16-byte aligned, rows 20 banks apart

struct HGeom {
    int N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil;
};

__device__ __forceinline__ float h2f(u16 b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ u16 f2h(float v) { return __builtin_bit_cast(u16, (_Float16)v); }   // v_cvt_f16_f32: RNE

// the epilogue of one output element, shared by the GEMM and the direct kernel: fp32 throughout, one rounding at the end
__device__ __forceinline__ float h_epi(float acc, bool has_scale, float sc, float sh, const u16* __restrict__ res, long ridx,
                                       int relu) {
    float v = has_scale ? acc * sc : acc;
    v = v + sh;
    if (res) v = v + h2f(res[ridx]);
    if (relu) v = fmaxf(v, 0.f);
    return v;
}
// clamp to the finite fp16 range; returns 1 when it had to
__device__ __forceinline__ int h_clamp(float& v) {
    if (fabsf(v) > H_MAX) {
        v = v > 0.f ? H_MAX : -H_MAX;
        return 1;
    }
    return 0;
}
__device__ __forceinline__ void h_count_flush(unsigned cnt, int* __restrict__ sat) {   // every lane of the wave calls this
    cnt = wave_sum_u(cnt);
    if ((threadIdx.x & 63) == 0 && cnt && sat) atomicAdd(sat, (int)cnt);
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_hweight(const float* __restrict__ w, int Cout, int Cin, int R, int S, u16* __restrict__ out) {
    const long total = (long)Cout * Cin * R * S;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin);
        long t = i / Cin;
        const int s = (int)(t % S);
        t /= S;
        const int r = (int)(t % R), co = (int)(t / R);
        out[i] = f2h(w[(((long)co * Cin + ci) * R + r) * S + s]);
    }
}
U2PL_API int u2pl_half_weight_f16(const float* w, int Cout, int Cin, int R, int S, unsigned short* out, hipStream_t stream) {
    if (!w || !out || Cout < 1 || Cin < 1 || R < 1 || S < 1) return U2PL_EINVAL;
    U2PL_LAUNCH(k_hweight, dim3(grid_for((long)Cout * Cin * R * S, 256)), dim3(256), 0, stream, w, Cout, Cin, R, S, out);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Y[m][co] = sum_{r,s,ci} X[pixel(m) * stride - pad + (r,s) * dil][ci] * W[co][r][s][ci].  256 threads = 4 waves (2 x 2),
// a wave owns (32 TM) x (32 TN) outputs as TM x TN 32x32 accumulators; K chunk = 32 channels of one tap.  Global ->
// register loads of chunk k+1 are issued before the MFMAs of chunk k and parked in the other LDS buffer after them.
// All gathers are raw buffer loads: an out-of-image tap, a row past M and a weight row past Cout read zeros.
// Operand lane map of v_mfma_f32_32x32x16_f16: lane (li = lane & 31, lh = lane >> 5) supplies A[row li][k = 8 lh + j] and
// B[k = 8 lh + j][col li], j = 0..7: one 16-byte LDS read each; C/D: col = li, row = (e & 3) + 8 (e >> 2) + 4 lh.
template <int TM, int TN>
__global__ __launch_bounds__(256) void k_hconv(const u16* __restrict__ x, long ldx, const u16* __restrict__ w,
                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                               const u16* __restrict__ res, long ldr, void* __restrict__ yv, long ldy, HGeom g,
                                               unsigned xbytes, unsigned wbytes, long M, int relu, int out_f32,
                                               int* __restrict__ sat) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    __shared__ __attribute__((aligned(16))) u16 lds[2 * (BM + BN) * H_LDP];
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, xbytes), rw = make_rsrc(w, wbytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int K = g.R * g.S * g.Cin, nk = K / H_BK, cpt = g.Cin / H_BK;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;

    const int kq = tid & 3, r0 = tid >> 2;       // 4 threads x 16 bytes = one 32-channel row segment; 64 rows per pass
    int bh[TM], bw[TM], nb[TM];
    bool mv[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long m = m0 + r0 + 64 * i;
        mv[i] = m < M;
        const unsigned mm = mv[i] ? (unsigned)m : 0u;
        const unsigned t = mm / (unsigned)g.Wout;
        const int wo = (int)(mm - t * (unsigned)g.Wout);
        const unsigned n = t / (unsigned)g.Hout;
        const int ho = (int)(t - n * (unsigned)g.Hout);
        bh[i] = ho * g.stride - g.pad;
        bw[i] = wo * g.stride - g.pad;
        nb[i] = (int)n * g.Hin * g.Win;
    }
    const int ldxb = (int)ldx * 2;
    u32x4 ra[TM], rb[TN];
    auto load_chunk = [&](int kc) {
        const int tap = kc / cpt, c0 = (kc - tap * cpt) * H_BK;
        const int r = tap / g.S, s = tap - r * g.S;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int ih = bh[i] + r * g.dil, iw = bw[i] + s * g.dil;
            const bool ok = mv[i] && ih >= 0 && ih < g.Hin && iw >= 0 && iw < g.Win;
            const int off = (nb[i] + ih * g.Win + iw) * ldxb + (c0 + kq * 8) * 2;
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, ok ? off : OOB_OFF, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int co = n0 + r0 + 64 * i;
            const int off = (co * K + kc * H_BK + kq * 8) * 2;
            rb[i] = __builtin_amdgcn_raw_buffer_load_b128(rw, co < g.Cout ? off : OOB_OFF, 0, 0);
        }
    };
    auto store_chunk = [&](int buf) {
        u16* A = lds + (long)buf * (BM + BN) * H_LDP;
        u16* B = A + BM * H_LDP;
#pragma unroll
        for (int i = 0; i < TM; ++i) *(u32x4*)(A + (r0 + 64 * i) * H_LDP + kq * 8) = ra[i];
#pragma unroll
        for (int i = 0; i < TN; ++i) *(u32x4*)(B + (r0 + 64 * i) * H_LDP + kq * 8) = rb[i];
    };

    hacc16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    const int li = lane & 31, lh = lane >> 5;
    auto mma = [&](int buf) {
        const u16* A = lds + (long)buf * (BM + BN) * H_LDP + (wm * 32 * TM + li) * H_LDP + 8 * lh;
        const u16* B = lds + (long)buf * (BM + BN) * H_LDP + (BM + wn * 32 * TN + li) * H_LDP + 8 * lh;
#pragma unroll
        for (int gk = 0; gk < H_BK / 16; ++gk) {
            h16x8 a8[TM], b8[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) a8[a] = __builtin_bit_cast(h16x8, *(const u32x4*)(A + a * 32 * H_LDP + gk * 16));
#pragma unroll
            for (int b = 0; b < TN; ++b) b8[b] = __builtin_bit_cast(h16x8, *(const u32x4*)(B + b * 32 * H_LDP + gk * 16));
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a8[a], b8[b], acc[a][b], 0, 0, 0);
        }
    };

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
        const bool more = kc + 1 < nk;           // block-uniform
        if (more) load_chunk(kc + 1);
        mma(kc & 1);
        if (more) store_chunk((kc + 1) & 1);     // the other buffer: last read in iteration kc - 1, before its barrier
        __syncthreads();
    }

    unsigned cnt = 0;
    u16* yh = (u16*)yv;
    float* yf = (float*)yv;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int c = n0 + wn * 32 * TN + b * 32 + li;
        const bool cv = c < g.Cout;              // ragged columns are masked
        const float sc = (cv && scale) ? scale[c] : 1.f;
        const float sh = (cv && shift) ? shift[c] : 0.f;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long m = m0 + wm * 32 * TM + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (cv && m < M) {
                    float v = h_epi(acc[a][b][e], scale != nullptr, sc, sh, res, m * ldr + c, relu);
                    if (out_f32) yf[m * ldy + c] = v;
                    else {
                        cnt += h_clamp(v);
                        yh[m * ldy + c] = f2h(v);
                    }
                }
            }
    }
    h_count_flush(cnt, sat);
}

template <int TM, int TN>
static int launch_hconv(const u16* x, long ldx, const u16* w, const float* scale, const float* shift, const u16* res, long ldr,
                        void* y, long ldy, const HGeom& g, unsigned xb, unsigned wb, long M, int relu, int out_f32, int* sat,
                        hipStream_t stream) {
    dim3 grid((unsigned)cdiv(M, 64 * TM), (unsigned)cdiv(g.Cout, 64 * TN));
    U2PL_LAUNCH((k_hconv<TM, TN>), grid, dim3(256), 0, stream, x, ldx, w, scale, shift, res, ldr, y, ldy, g, xb, wb, M, relu,
                out_f32, sat);
    U2PL_LAUNCH_CHECK();
    return 0;
}

static bool hgeom_ok(const HGeom& g) {
    if (g.N < 1 || g.Hin < 1 || g.Win < 1 || g.Cin < 1 || g.Cout < 1 || g.R < 1 || g.S < 1 || g.stride < 1 || g.pad < 0 ||
        g.dil < 1)
        return false;
    const long eh = (long)g.Hin + 2 * g.pad - (long)g.dil * (g.R - 1) - 1, ew = (long)g.Win + 2 * g.pad - (long)g.dil * (g.S - 1) - 1;
    if (eh < 0 || ew < 0) return false;
    return g.Hout == eh / g.stride + 1 && g.Wout == ew / g.stride + 1;
}

U2PL_API int u2pl_hconv2d_fwd_f16(const unsigned short* x, long ldx, const unsigned short* w, const float* scale,
                                  const float* shift, const unsigned short* res, long ldr, void* y, long ldy, int N, int Hin,
                                  int Win, int Cin, int Hout, int Wout, int Cout, int R, int S, int stride, int pad, int dil,
                                  int relu, int out_f32, int tile, int* sat, hipStream_t stream) {
    const HGeom g{N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil};
    if (!x || !w || !y || !hgeom_ok(g) || Cin % H_BK || ldx < Cin || ldy < Cout || (res && ldr < Cout)) return U2PL_EINVAL;
    if (ldx % 8 || ((uintptr_t)x & 15) || ((uintptr_t)w & 15) || tile < 0 || tile > 2) return U2PL_EINVAL;   // 16-byte gathers
    const long M = (long)N * Hout * Wout;
    const long xb = (((long)N * Hin * Win - 1) * ldx + Cin) * 2, wb = (long)Cout * R * S * Cin * 2;
    if (xb >= (1L << 31) || wb >= (1L << 31) || M >= (1L << 31)) return U2PL_EINVAL;
    // tile rows: 128 when that still gives every CU a block, else 64 (tile = 1 | 2 forces one: tests); 64 columns for narrow heads
    const bool wide = Cout > 64;
    const long blocks128 = (long)cdiv(M, 128) * cdiv(Cout, wide ? 128 : 64);
    const bool tall = tile ? tile == 2 : blocks128 >= 256;
#define H_GO(TM, TN) \
    return launch_hconv<TM, TN>(x, ldx, w, scale, shift, res, ldr, y, ldy, g, (unsigned)xb, (unsigned)wb, M, relu, out_f32, sat, stream)
    if (tall && wide) H_GO(2, 2);
    if (tall) H_GO(2, 1);
    if (wide) H_GO(1, 2);
    H_GO(1, 1);
#undef H_GO
}

// ---------------------------------------------------------------------------------------------------------------------
// Direct form for a handful of input channels (the stem's first convolution: Cin = 3, 0.25 GFLOP at 769^2): x is the fp32
// NHWC image, the fp16 weights are widened into LDS as [tap][ci][Cout]; one thread per (pixel, output channel), lanes
// along the channels (the image taps are wave-wide broadcasts), an fmaf chain in tap order.
#define H_STEM_MAXW 8192
__global__ __launch_bounds__(256) void k_hstem(const float* __restrict__ x, long ldx, const u16* __restrict__ w,
                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                               u16* __restrict__ y, long ldy, HGeom g, long M, int relu, int* __restrict__ sat) {
    __shared__ float wl[H_STEM_MAXW];
    const int KT = g.R * g.S * g.Cin;
    for (int i = threadIdx.x; i < KT * g.Cout; i += blockDim.x) {
        const int co = i / KT, k = i - co * KT;
        wl[k * g.Cout + co] = h2f(w[i]);
    }
    __syncthreads();
    unsigned cnt = 0;
    const long total = M * g.Cout;
    const long span = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += span) {
        const int c = (int)(i % g.Cout);
        const long m = i / g.Cout;
        const int wo = (int)(m % g.Wout);
        const long t = m / g.Wout;
        const int ho = (int)(t % g.Hout), n = (int)(t / g.Hout);
        float acc = 0.f;
        for (int r = 0; r < g.R; ++r) {
            const int ih = ho * g.stride - g.pad + r * g.dil;
            if (ih < 0 || ih >= g.Hin) continue;
            for (int s = 0; s < g.S; ++s) {
                const int iw = wo * g.stride - g.pad + s * g.dil;
                if (iw < 0 || iw >= g.Win) continue;
                const float* xp = x + ((long)(n * g.Hin + ih) * g.Win + iw) * ldx;
                const float* wp = wl + (r * g.S + s) * g.Cin * g.Cout + c;
                for (int ci = 0; ci < g.Cin; ++ci) acc = __fmaf_rn(xp[ci], wp[ci * g.Cout], acc);
            }
        }
        float v = h_epi(acc, scale != nullptr, scale ? scale[c] : 1.f, shift ? shift[c] : 0.f, nullptr, 0, relu);
        cnt += h_clamp(v);
        y[m * ldy + c] = f2h(v);
    }
    h_count_flush(cnt, sat);
}
U2PL_API int u2pl_hconv2d_stem_f16(const float* x, long ldx, const unsigned short* w, const float* scale, const float* shift,
                                   unsigned short* y, long ldy, int N, int Hin, int Win, int Cin, int Hout, int Wout, int Cout,
                                   int R, int S, int stride, int pad, int dil, int relu, int* sat, hipStream_t stream) {
    const HGeom g{N, Hin, Win, Cin, Hout, Wout, Cout, R, S, stride, pad, dil};
    if (!x || !w || !y || !hgeom_ok(g) || ldx < Cin || ldy < Cout || (long)R * S * Cin * Cout > H_STEM_MAXW) return U2PL_EINVAL;
    const long M = (long)N * Hout * Wout;
    if ((long)N * Hin * Win >= (1L << 31)) return U2PL_EINVAL;
    U2PL_LAUNCH(k_hstem, dim3(grid_for(M * Cout, 256)), dim3(256), 0, stream, x, ldx, w, scale, shift, y, ldy, g, M, relu, sat);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1, ceil_mode=True) on fp16 rows: 8 channels per thread; the comparison is k_maxpool_fwd's (scan order,
// strict '>', a NaN wins) on the widened values, which is exact
__global__ void k_hmaxpool(const u16* __restrict__ x, long ldx, int N, int H, int W, int C, int Ho, int Wo, u16* __restrict__ y,
                           long ldy) {
    const int C8 = C >> 3;
    const long total = (long)N * Ho * Wo * C8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int wo = (int)(p % Wo);
        const long t = p / Wo;
        const int ho = (int)(t % Ho), n = (int)(t / Ho);
        float best[8];
        u16 bb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bb[j] = 0xfc00; }
        bool first = true;
        for (int r = 0; r < 3; ++r) {
            const int ih = ho * 2 - 1 + r;
            if (ih < 0 || ih >= H) continue;
            for (int s = 0; s < 3; ++s) {
                const int iw = wo * 2 - 1 + s;
                if (iw < 0 || iw >= W) continue;
                const u32x4 q = *(const u32x4*)(x + ((long)(n * H + ih) * W + iw) * ldx + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const u16 hb = (u16)(q[j >> 1] >> (16 * (j & 1)));
                    const float v = h2f(hb);
                    if (first || v > best[j] || v != v) { best[j] = v; bb[j] = hb; }
                }
                first = false;
            }
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (unsigned)bb[2 * j] | ((unsigned)bb[2 * j + 1] << 16);
        *(u32x4*)(y + p * ldy + c) = o;
    }
}
U2PL_API int u2pl_hmaxpool3s2_f16(const unsigned short* x, long ldx, int N, int H, int W, int C, int Ho, int Wo,
                                  unsigned short* y, long ldy, hipStream_t stream) {
    if (!x || !y || N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C ||
        ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
        return U2PL_EINVAL;
    // torch's ceil-mode size: ceil((H + 2 - 3) / 2) + 1, minus one when the last window would start in the padding
    int eh = (H - 1 + 1) / 2 + 1, ew = (W - 1 + 1) / 2 + 1;
    if ((eh - 1) * 2 >= H + 1) --eh;
    if ((ew - 1) * 2 >= W + 1) --ew;
    if (Ho != eh || Wo != ew) return U2PL_EINVAL;
    U2PL_LAUNCH(k_hmaxpool, dim3(grid_for((long)N * Ho * Wo * (C / 8), 256)), dim3(256), 0, stream, x, ldx, N, H, W, C, Ho, Wo,
                y, ldy);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// y[n][c] = fp16(sum_p x[n][p][c] / HW): a block owns 64 channels of one image, 16 pixel phases of 64 lanes; fp32 partial
// sums in a fixed order (phase-strided, then phases 0..15): deterministic
__global__ __launch_bounds__(1024) void k_hgap(const u16* __restrict__ x, long ldx, int HW, int C, u16* __restrict__ y) {
    __shared__ float part[16][64];
    const int cg = (C + 63) >> 6;
    const int n = blockIdx.x / cg, c = (blockIdx.x % cg) * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C)
        for (int p = ph; p < HW; p += 16) s += h2f(x[((long)n * HW + p) * ldx + c]);
    part[ph][threadIdx.x & 63] = s;
    __syncthreads();
    if (ph == 0 && c < C) {
        float t = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += part[k][threadIdx.x];
        y[(long)n * C + c] = f2h(t / (float)HW);
    }
}
U2PL_API int u2pl_hgap_f16(const unsigned short* x, long ldx, int N, int HW, int C, unsigned short* y, hipStream_t stream) {
    if (!x || !y || N < 1 || HW < 1 || C < 1 || ldx < C) return U2PL_EINVAL;
    U2PL_LAUNCH(k_hgap, dim3((unsigned)(N * ((C + 63) / 64))), dim3(1024), 0, stream, x, ldx, HW, C, y);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// y[n][oy][ox][c] = fp16(bilinear(align_corners=True) of the widened taps): the bits u2pl_bilinear_up_f32 would store for
// the widened input, rounded once.  8 channels per thread.
__global__ void k_hbilinear(const u16* __restrict__ x, long ldx, int N, int h, int w, int C, u16* __restrict__ y, long ldy,
                            int H, int W, float sy, float sx) {
    const int C8 = C >> 3;
    const long total = (long)N * H * W * C8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C8) * 8;
        const long p = i / C8;
        const int ox = (int)(p % W);
        const long t = p / W;
        const int oy = (int)(t % H), n = (int)(t / H);
        const AcCoord cy = ac_coord(oy, sy, h), cx = ac_coord(ox, sx, w);
        const u16* b = x + (long)n * h * w * ldx + c;
        const u32x4 q00 = *(const u32x4*)(b + ((long)cy.i0 * w + cx.i0) * ldx), q01 = *(const u32x4*)(b + ((long)cy.i0 * w + cx.i1) * ldx);
        const u32x4 q10 = *(const u32x4*)(b + ((long)cy.i1 * w + cx.i0) * ldx), q11 = *(const u32x4*)(b + ((long)cy.i1 * w + cx.i1) * ldx);
        u16 ob[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sh = 16 * (j & 1);
            const float v00 = h2f((u16)(q00[j >> 1] >> sh)), v01 = h2f((u16)(q01[j >> 1] >> sh));
            const float v10 = h2f((u16)(q10[j >> 1] >> sh)), v11 = h2f((u16)(q11[j >> 1] >> sh));
            const float top = __fmaf_rn(cx.l0, v00, __fmul_rn(cx.l1, v01));
            const float bot = __fmaf_rn(cx.l0, v10, __fmul_rn(cx.l1, v11));
            ob[j] = f2h(__fmaf_rn(cy.l0, top, __fmul_rn(cy.l1, bot)));
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (unsigned)ob[2 * j] | ((unsigned)ob[2 * j + 1] << 16);
        *(u32x4*)(y + p * ldy + c) = o;
    }
}
U2PL_API int u2pl_hbilinear_f16(const unsigned short* x, long ldx, int N, int h, int w, int C, unsigned short* y, long ldy,
                                int H, int W, hipStream_t stream) {
    if (!x || !y || N < 1 || h < 1 || w < 1 || H < 1 || W < 1 || C < 8 || C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C ||
        ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
        return U2PL_EINVAL;
    U2PL_LAUNCH(k_hbilinear, dim3(grid_for((long)N * H * W * (C / 8), 256)), dim3(256), 0, stream, x, ldx, N, h, w, C, y, ldy, H,
                W, ac_scale_host(h, H), ac_scale_host(w, W));
    U2PL_LAUNCH_CHECK();
    return 0;
}
