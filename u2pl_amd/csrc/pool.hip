// Pyramid pooling (PSPNet, Zhao et al. 2017): nn.AdaptiveAvgPool2d((b, b)) for up to four levels b of one NHWC input, forward
// in one launch, and the gather backward that writes dx once.
//
// ARITHMETIC CONTRACT (part of the interface; tests/psp_bounds.py emulates exactly this order)
//   window rule   window i of b over an axis of length H is [floor(i H / b), ceil((i + 1) H / b)) -- torch's rule; windows of
//                 neighbouring indices share a row when H % b != 0, and b may exceed H (windows of one or two rows)
//   forward       a window's pixels are numbered k = r * wlen + s (row-major inside the window).  Lane j of PSP_LANES (16) adds
//                 the pixels k = j, j + 16, j + 32, ... to 0.0f in that order, in fp32; the 16 lane sums are then added pairwise
//                 over four rounds, lane j += lane j + 8, then + 4, + 2, + 1 (lanes past the window hold 0.0f).  The result
//                 is DIVIDED by (float)area, one IEEE division, area = hlen * wlen the true size of the window.
//   backward      acc = 0.0f; levels in the order of the arguments (null g: skipped); inside a level the windows that contain the
//                 pixel in ascending (i, j), i the window row; each term is g * inv, inv = 1.0f / (float)area one IEEE division,
//                 the product rounded, then added to acc; `add` (when given) is added LAST; one store.  (Pixels of a row that
//                 lie in the same windows share acc up to `add`: the same value by the same operations.)
//   The order depends on nothing but the shapes: not on the grid, the block or the run.  No atomics, no memset; eager and
//   graph-replayed launches give the same bits.  -ffp-contract=off (build_ext) keeps products and sums apart.
#include "common.h"
#include "u2pl_hip.h"

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

#define PSP_LANES 16           // pixel lanes of a forward work item
#define PSP_CH4 16             // float4 channel lanes of a forward work item (64 channels, 256 B per pixel)
#define PSP_FWD_MAX_BLOCKS 2048

struct PspLevels {
    int b[4];
    float* y[4];
    long ldy[4];
    long first[4];             // first work item of the level; first[l + 1] - first[l] = N * b * b * chunks
};

// (32-bit: the entry points hold b <= 16384 and H <= 65535, so (i + 1) H + b < 2^31)
__device__ __forceinline__ int psp_start(int i, int H, int b) { return (i * H) / b; }
__device__ __forceinline__ int psp_end(int i, int H, int b) { return ((i + 1) * H + b - 1) / b; }

// one work item = (level, image, window, chunk of 64 channels), one block of 256 threads per item, grid-stride over items
__global__ void __launch_bounds__(256) k_pyramid_pool_fwd(const float* __restrict__ x, long ldx, int N, int H, int W, int C,
                                                          PspLevels lv, long items) {
    __shared__ float4 s_part[PSP_LANES][PSP_CH4];
    const int C4 = C >> 2;
    const int chunks = (C4 + PSP_CH4 - 1) / PSP_CH4;
    const int cl = threadIdx.x % PSP_CH4, pl = threadIdx.x / PSP_CH4;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        int l = 0;
        while (l < 3 && (lv.b[l] == 0 || it >= lv.first[l] + (long)N * lv.b[l] * lv.b[l] * chunks)) ++l;
        const int b = lv.b[l];
        long r = it - lv.first[l];
        const int ch = (int)(r % chunks);
        r /= chunks;                       // r = (n * b + i) * b + j: the output row
        const int j = (int)(r % b);
        const long t = r / b;
        const int i = (int)(t % b), n = (int)(t / b);
        const int h0 = psp_start(i, H, b), hlen = psp_end(i, H, b) - h0;
        const int w0 = psp_start(j, W, b), wlen = psp_end(j, W, b) - w0;
        const int area = hlen * wlen;
        const int c4 = ch * PSP_CH4 + cl;
        float4 acc = f4zero();
        if (c4 < C4) {
            // pixel k of the window is (rr, ss) = (k / wlen, k % wlen); k advances by PSP_LANES, (rr, ss) without a division.  Four
            // loads are issued before their four adds: the adds keep the order k, k + 16, k + 32, ...
            const float* base = x + (((long)n * H + h0) * W + w0) * ldx + c4 * 4;
            int k = pl, rr = pl / wlen, ss = pl - rr * wlen;
            auto next = [&]() -> const float4* {
                const float4* q = (const float4*)(base + ((long)rr * W + ss) * ldx);
                k += PSP_LANES; ss += PSP_LANES;
                while (ss >= wlen) { ss -= wlen; ++rr; }
                return q;
            };
            while (k + 3 * PSP_LANES < area) {
                const float4* q0 = next(); const float4* q1 = next(); const float4* q2 = next(); const float4* q3 = next();
                const float4 v0 = *q0, v1 = *q1, v2 = *q2, v3 = *q3;
                acc = f4add(f4add(f4add(f4add(acc, v0), v1), v2), v3);
            }
            while (k < area) acc = f4add(acc, *next());
        }
        s_part[pl][cl] = acc;
        __syncthreads();
#pragma unroll
        for (int o = PSP_LANES / 2; o > 0; o >>= 1) {
            if (pl < o) {
                acc = f4add(acc, s_part[pl + o][cl]);
                s_part[pl][cl] = acc;
            }
            __syncthreads();
        }
        if (pl == 0 && c4 < C4) {
            const float a = (float)area;
            acc.x = __fdiv_rn(acc.x, a); acc.y = __fdiv_rn(acc.y, a); acc.z = __fdiv_rn(acc.z, a); acc.w = __fdiv_rn(acc.w, a);
            *(float4*)(lv.y[l] + r * lv.ldy[l] + c4 * 4) = acc;
        }
    }
}

// levels: each >= 0 and not all 0; the kernels index with 32-bit integers: levels <= 16384, H and W <= 65535, N H W < 2^31
#define PSP_MAX_LEVEL 16384
static bool psp_shape_ok(int N, int H, int W, int C, int b0, int b1, int b2, int b3) {
    if (C % 4 || C <= 0 || N <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)N * H * W >= (1L << 31)) return false;
    if (b0 < 0 || b1 < 0 || b2 < 0 || b3 < 0 || (b0 | b1 | b2 | b3) == 0) return false;
    return b0 <= PSP_MAX_LEVEL && b1 <= PSP_MAX_LEVEL && b2 <= PSP_MAX_LEVEL && b3 <= PSP_MAX_LEVEL;
}

U2PL_API int u2pl_pyramid_pool_fwd_f32(const float* x, long ldx, int N, int H, int W, int C, int b0, int b1, int b2, int b3,
                                       float* y0, long ldy0, float* y1, long ldy1, float* y2, long ldy2, float* y3, long ldy3,
                                       hipStream_t stream) {
    if (!psp_shape_ok(N, H, W, C, b0, b1, b2, b3) || !x || ldx < C || ldx % 4)
        return U2PL_EINVAL;
    PspLevels lv;
    const int b[4] = {b0, b1, b2, b3};
    float* const y[4] = {y0, y1, y2, y3};
    const long ld[4] = {ldy0, ldy1, ldy2, ldy3};
    const long chunks = (C / 4 + PSP_CH4 - 1) / PSP_CH4;
    long items = 0;
    for (int l = 0; l < 4; ++l) {
        if (b[l] && (!y[l] || ld[l] < C || ld[l] % 4)) return U2PL_EINVAL;
        lv.b[l] = b[l]; lv.y[l] = y[l]; lv.ldy[l] = ld[l]; lv.first[l] = items;
        items += (long)N * b[l] * b[l] * chunks;
    }
    const long g = items < PSP_FWD_MAX_BLOCKS ? items : PSP_FWD_MAX_BLOCKS;
    U2PL_LAUNCH(k_pyramid_pool_fwd, dim3((unsigned)g), dim3(256), 0, stream, x, ldx, N, H, W, C, lv, items);
    U2PL_LAUNCH_CHECK();
    return 0;
}

struct PspGrads {
    int b[4];
    const float* g[4];         // null: the level is skipped
    long ldg[4];
};

// gather: one work item = PSP_SEG consecutive pixels of one image row, taken by one wave; lane j of 64 owns the float4 channel groups
// j, j + 64, ... (PSP_KC of them per pass), so the window arithmetic is wave-uniform and is done once for up to 2048 channels.  The
// windows of a level that contain row h are the contiguous range floor(h b / H) .. ceil((h + 1) b / H) - 1 (the inverse of the
// window rule; two at most while b <= H, more when b > H).  Neighbouring pixels of a row lie in the same windows until the next
// window edge: the pooled sum (everything before `add`) is formed for the first pixel of the item and again only where a window
// range changes -- the same operations in the same order as forming it per pixel, hence the same bits -- so the pooled rows go
// through the cache once per run of pixels, not once per pixel.
#define PSP_KC 8
#define PSP_SEG 4
__global__ void __launch_bounds__(256) k_pyramid_pool_bwd(PspGrads lv, const float* __restrict__ add, long ldadd, int N, int H,
                                                          int W, int C, float* __restrict__ dx, long lddx) {
    const int C4 = C >> 2;
    const int lane = threadIdx.x & 63;
    const int nseg = (W + PSP_SEG - 1) / PSP_SEG;
    const int items = N * H * nseg, nwaves = gridDim.x * 4;
    for (int it = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); it < items; it += nwaves) {
        const int seg = it % nseg, t = it / nseg;
        const int h = t % H, n = t / H;
        const int w_first = seg * PSP_SEG, w_end = min(W, w_first + PSP_SEG);
        for (int cb = lane; cb < C4 + lane; cb += 64 * PSP_KC) {       // cb - lane is wave-uniform: every lane makes the same trips
            float4 acc[PSP_KC];
            int j_lo[4] = {0, 0, 0, 0}, j_hi[4] = {0, 0, 0, 0};
            for (int w = w_first; w < w_end; ++w) {
                bool fresh = w == w_first;
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const int b = lv.b[l];
                    if (b == 0 || lv.g[l] == nullptr) continue;
                    const int lo = (w * b) / W, hi = ((w + 1) * b + W - 1) / W - 1;
                    fresh = fresh || lo != j_lo[l] || hi != j_hi[l];
                    j_lo[l] = lo; j_hi[l] = hi;
                }
                if (fresh) {
#pragma unroll
                    for (int k = 0; k < PSP_KC; ++k) acc[k] = f4zero();
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const int b = lv.b[l];
                        const float* __restrict__ g = lv.g[l];
                        if (b == 0 || g == nullptr) continue;
                        const int i_lo = (h * b) / H, i_hi = ((h + 1) * b + H - 1) / H - 1;
                        for (int i = i_lo; i <= i_hi; ++i) {
                            const int hlen = psp_end(i, H, b) - psp_start(i, H, b);
                            for (int j = j_lo[l]; j <= j_hi[l]; ++j) {
                                const int wlen = psp_end(j, W, b) - psp_start(j, W, b);
                                const float inv = __fdiv_rn(1.0f, (float)(hlen * wlen));
                                const float* row = g + (((long)n * b + i) * b + j) * lv.ldg[l] + (long)cb * 4;
#pragma unroll
                                for (int k = 0; k < PSP_KC; ++k) {
                                    if (cb + 64 * k < C4) {
                                        const float4 v = *(const float4*)(row + 256 * k);
                                        acc[k].x += __fmul_rn(v.x, inv); acc[k].y += __fmul_rn(v.y, inv);
                                        acc[k].z += __fmul_rn(v.z, inv); acc[k].w += __fmul_rn(v.w, inv);
                                    }
                                }
                            }
                        }
                    }
                }
                const long p = ((long)n * H + h) * W + w;
#pragma unroll
                for (int k = 0; k < PSP_KC; ++k) {
                    if (cb + 64 * k < C4) {
                        const long c = ((long)cb + 64 * k) * 4;
                        float4 a = acc[k];
                        if (add != nullptr) a = f4add(a, *(const float4*)(add + p * ldadd + c));
                        *(float4*)(dx + p * lddx + c) = a;
                    }
                }
            }
        }
    }
}

U2PL_API int u2pl_pyramid_pool_bwd_f32(const float* g0, long ldg0, const float* g1, long ldg1, const float* g2, long ldg2,
                                       const float* g3, long ldg3, const float* add, long ldadd, int N, int H, int W, int C,
                                       int b0, int b1, int b2, int b3, float* dx, long lddx, hipStream_t stream) {
    if (!psp_shape_ok(N, H, W, C, b0, b1, b2, b3) || !dx || lddx < C || lddx % 4)
        return U2PL_EINVAL;
    if (add && (ldadd < C || ldadd % 4)) return U2PL_EINVAL;
    PspGrads lv;
    const int b[4] = {b0, b1, b2, b3};
    const float* const g[4] = {g0, g1, g2, g3};
    const long ld[4] = {ldg0, ldg1, ldg2, ldg3};
    for (int l = 0; l < 4; ++l) {
        if (b[l] && g[l] && (ld[l] < C || ld[l] % 4)) return U2PL_EINVAL;
        lv.b[l] = b[l]; lv.g[l] = b[l] ? g[l] : nullptr; lv.ldg[l] = ld[l];
    }
    const long items = (long)N * H * ((W + PSP_SEG - 1) / PSP_SEG);
    U2PL_LAUNCH(k_pyramid_pool_bwd, dim3(grid_for(items * 64, 256)), dim3(256), 0, stream, lv, add, ldadd, N, H, W, C, dx, lddx);
    U2PL_LAUNCH_CHECK();
    return 0;
}
