// Object-contextual representations (OCRNet, Yuan et al., ECCV 2020): the two operations of the head that are not convolutions.
//   region pool        m = softmax over the PIXELS of an image of scale * s,  f[n, k, :] = sum_p m[n, p, k] x[n, p, :]
//   region attention   w = softmax over the K regions of scale * q . kk,      y[n, p, :] = sum_k w[n, p, k] v[n, k, :]
// forward and backward.  x, q, y, ... are NHWC rows [N*HW][C]; region-side tensors are [N*K][C]; per-pixel weights are [N*HW][K].
//
// ARITHMETIC CONTRACT (part of the interface; tests/ocr_bounds.py emulates this order)
//   everything is fp32 on the vector ALU.  fma(a, b, c) below is ONE rounding of a * b + c (__fmaf_rn); products and sums that are
//   written apart are rounded apart (-ffp-contract=off, build_ext).  No atomics, no memset; every workspace word that is read
//   was written by the same call before.  The order depends on the shapes alone: eager and graph-replayed launches give the same
//   bits.
//   wave sum           64 lane values are added pairwise in six rounds (wave_sum_sgpr of common.h): 6 roundings.
//   dot(row, xrow)     channels are taken in passes of OCR_PASS (256): in a pass, lane l forms p = a0 b0, p = fma(a1, b1, p),
//                      fma(a2, b2, p), fma(a3, b3, p) over its float4 (channels 4 l .. 4 l + 3 of the pass; lanes past the row
//                      hold 0); the pass's wave sum is added to the running dot, which starts at 0.0f.
//   mix(wt, rows)      out[c] = fma(wt[K - 1], rows[K - 1][c], ... fma(wt[0], rows[0][c], 0.0f)), regions ascending; `add` last.
//   column sums        (softmax over pixels) a slab is OCR_SLAB (256) consecutive pixels of one image.  With R = 256 / K, row r of
//                      a block adds the slab's pixels r, r + R, ... to 0.0f in that order; the R row sums are added in ascending
//                      r to row 0's; the slab sums of an image are added in ascending slab order.  Maxima are exact.
//   region pool fwd    t = scale * s; M = max over the image's pixels of t; m = expf(t - M) / Z (one IEEE division), Z the column
//                      sum of expf(t - M).
//   weighted sum       (f, dv, dk)  out[k][c] = sum_p a[p][k] x[p][c]: wave j of four takes the pixels 64 j .. 64 j + 63 of a slab,
//                      acc = fma(a[p][k], x[p][c], acc) from 0.0f in ascending p; the four wave sums are added in ascending j
//                      to wave 0's; the slab sums are added in ascending slab order to slab 0's.
//   region pool bwd    c[k] = dot over ALL channels by one wave (per lane one fma chain over the passes, then one wave sum);
//                      ds = (scale * m) * (dot(g_f[k], x[p]) - c[k]);  dx = mix(m[p], g_f) + add.
//   region attn fwd    t = scale * dot(kk[k], q[p]); w = expf(t - max_k t) / Z, Z = wave sum of the lane sums ((e0 + e1) + e2) + e3
//                      (lane l holds the regions l, l + 64, l + 128, l + 192); y = mix(w, v).
//   region attn bwd    dw = dot(v[k], g_y[p]); sd = wave sum of the lanes' fma chains w0 dw0, fma(w1, dw1, .), ...;
//                      e = (scale * w) * (dw - sd)   [scale enters here, once, for dq and dk];  dq = mix(e, kk);
//                      dv = weighted sum (w, g_y); dk = weighted sum (e, q).
#include "common.h"
#include "u2pl_hip.h"

#define OCR_SLAB 256           // pixels of one slab (column sums and weighted sums)
#define OCR_WAVE_PX 64         // pixels one wave of a weighted-sum block adds up (OCR_SLAB / 4 waves)
#define OCR_KT 16              // regions of one weighted-sum work item (16 float4 accumulators per lane)
#define OCR_KCHUNK 64          // regions per lane register of the per-pixel kernels: lane l of register r holds region 64 r + l
#define OCR_KREGS 4            // K <= 255 < OCR_KCHUNK * OCR_KREGS
#define OCR_PX 4               // consecutive pixels of one image taken by one wave of the per-pixel kernels
#define OCR_PASS 256           // channels of one pass of a wave: 64 lanes x float4
#define OCR_MAX_BLOCKS 1024    // grid cap of every kernel of this file (grid-stride over work items)
#define OCR_MAX_K 255

__device__ __forceinline__ float4 o4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 o4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 o4fma(float s, float4 b, float4 c) {
    return make_float4(__fmaf_rn(s, b.x, c.x), __fmaf_rn(s, b.y, c.y), __fmaf_rn(s, b.z, c.z), __fmaf_rn(s, b.w, c.w));
}
__device__ __forceinline__ float o4dot(float4 a, float4 b) {
    return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmul_rn(a.x, b.x))));
}
__device__ __forceinline__ float4 o4ld(const float* p) { return *(const float4*)p; }

// ---- softmax over the pixels of an image: column maxima, column sums, normalised write ---------------------------------------------
// one work item = one slab of one image, one block of 256 threads; thread t = r * K + k (r < R = 256 / K) walks the slab's pixels
// r, r + R, ... of column k.  wmax / wsum: [N * S][K] slab partials, S = slabs per image.
__device__ __forceinline__ float ocr_col_fold_max(float v, float* s_red, int K, int R) {
    const int t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    if (t < K)
        for (int r = 1; r < R; ++r) v = fmaxf(v, s_red[r * K + t]);
    __syncthreads();
    return v;
}
__device__ __forceinline__ float ocr_col_fold_sum(float v, float* s_red, int K, int R) {
    const int t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    if (t < K)
        for (int r = 1; r < R; ++r) v += s_red[r * K + t];
    __syncthreads();
    return v;
}

__global__ void __launch_bounds__(256) k_region_colmax(const float* __restrict__ s, long lds, float scale, int N, int HW, int K, int S,
                                                       float* __restrict__ wmax) {
    __shared__ float s_red[256];
    const int R = 256 / K, t = threadIdx.x, r = t / K, k = t - r * K;
    for (int it = blockIdx.x; it < N * S; it += gridDim.x) {
        const int n = it / S, sl = it - n * S;
        const int p0 = sl * OCR_SLAB, p1 = min(HW, p0 + OCR_SLAB);
        float mx = -INFINITY;
        if (r < R)
            for (int p = p0 + r; p < p1; p += R) mx = fmaxf(mx, __fmul_rn(scale, s[((long)n * HW + p) * lds + k]));
        mx = ocr_col_fold_max(mx, s_red, K, R);
        if (t < K) wmax[(long)it * K + t] = mx;
    }
}

// column k's maximum over the image (thread t < K; others: 0)
__device__ __forceinline__ float ocr_image_max(const float* __restrict__ wmax, int n, int S, int K) {
    float M = 0.f;
    if ((int)threadIdx.x < K) {
        M = wmax[(long)n * S * K + threadIdx.x];
        for (int j = 1; j < S; ++j) M = fmaxf(M, wmax[((long)n * S + j) * K + threadIdx.x]);
    }
    return M;
}

__global__ void __launch_bounds__(256) k_region_colsum(const float* __restrict__ s, long lds, float scale, int N, int HW, int K, int S,
                                                       const float* __restrict__ wmax, float* __restrict__ wsum) {
    __shared__ float s_red[256];
    __shared__ float s_M[256];
    const int R = 256 / K, t = threadIdx.x, r = t / K, k = t - r * K;
    for (int it = blockIdx.x; it < N * S; it += gridDim.x) {
        const int n = it / S, sl = it - n * S;
        s_M[t] = ocr_image_max(wmax, n, S, K);
        __syncthreads();
        const int p0 = sl * OCR_SLAB, p1 = min(HW, p0 + OCR_SLAB);
        float z = 0.f;
        if (r < R) {
            const float M = s_M[k];
            for (int p = p0 + r; p < p1; p += R) z += expf(__fsub_rn(__fmul_rn(scale, s[((long)n * HW + p) * lds + k]), M));
        }
        z = ocr_col_fold_sum(z, s_red, K, R);
        if (t < K) wsum[(long)it * K + t] = z;
    }
}

__global__ void __launch_bounds__(256) k_region_colnorm(const float* __restrict__ s, long lds, float scale, int N, int HW, int K, int S,
                                                        const float* __restrict__ wmax, const float* __restrict__ wsum,
                                                        float* __restrict__ m, long ldm) {
    __shared__ float s_M[256];
    __shared__ float s_Z[256];
    const int R = 256 / K, t = threadIdx.x, r = t / K, k = t - r * K;
    for (int it = blockIdx.x; it < N * S; it += gridDim.x) {
        const int n = it / S, sl = it - n * S;
        s_M[t] = ocr_image_max(wmax, n, S, K);
        float Z = 0.f;
        if (t < K) {
            Z = wsum[(long)n * S * K + t];
            for (int j = 1; j < S; ++j) Z += wsum[((long)n * S + j) * K + t];
        }
        s_Z[t] = Z;
        __syncthreads();
        const int p0 = sl * OCR_SLAB, p1 = min(HW, p0 + OCR_SLAB);
        if (r < R) {
            const float M = s_M[k], Zk = s_Z[k];
            for (int p = p0 + r; p < p1; p += R) {
                const long row = (long)n * HW + p;
                m[row * ldm + k] = __fdiv_rn(expf(__fsub_rn(__fmul_rn(scale, s[row * lds + k]), M)), Zk);
            }
        }
        __syncthreads();
    }
}

// ---- pixels -> regions weighted sum: out[n, k, :] = sum_p a[n, p, k] x[n, p, :]  (f, dv and dk) ------------------------------------
// one work item = (image, slab, chunk of OCR_PASS channels, chunk of OCR_KT regions), one block of four waves; wave j walks the pixels
// 64 j .. 64 j + 63 of the slab, lane l owns float4 l of the channel chunk and OCR_KT accumulators.  The weights a[p][k0 ..] are
// wave-uniform.  part: [N * S][K][C] slab partials (dense), reduced by k_region_wsum_reduce in ascending slab order.
__global__ void __launch_bounds__(256) k_region_wsum(const float* __restrict__ a, long lda, const float* __restrict__ x, long ldx, int N,
                                                     int HW, int K, int C, int S, float* __restrict__ part) {
    __shared__ float4 s_acc[OCR_KT][64];
    const int C4 = C >> 2, CCH = (C4 + 63) / 64, KCH = (K + OCR_KT - 1) / OCR_KT;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long items = (long)N * S * CCH * KCH;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int kc = (int)(it % KCH);
        long r = it / KCH;
        const int cc = (int)(r % CCH);
        r /= CCH;                                  // r = n * S + sl
        const int sl = (int)(r % S), n = (int)(r / S);
        const int k0 = kc * OCR_KT, kn = min(OCR_KT, K - k0);
        const int c4 = cc * 64 + lane;
        const bool cok = c4 < C4;
        const int c4r = cok ? c4 : C4 - 1;         // lanes past the row read its last float4 (in bounds) and store nothing
        const int pb = sl * OCR_SLAB + wv * OCR_WAVE_PX, pe = min(HW, pb + OCR_WAVE_PX);
        float4 acc[OCR_KT];
#pragma unroll
        for (int j = 0; j < OCR_KT; ++j) acc[j] = o4zero();
        const float* xr = x + ((long)n * HW + pb) * ldx + (long)c4r * 4;
        const float* ar = a + ((long)n * HW + pb) * lda + k0;
#pragma unroll 2
        for (int p = pb; p < pe; ++p, xr += ldx, ar += lda) {
            const float4 xv = o4ld(xr);
#pragma unroll
            for (int j = 0; j < OCR_KT; ++j)
                if (j < kn) acc[j] = o4fma(ar[j], xv, acc[j]);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (wv == w) {
#pragma unroll
                for (int j = 0; j < OCR_KT; ++j)
                    if (j < kn) s_acc[j][lane] = w == 0 ? acc[j] : o4add(s_acc[j][lane], acc[j]);
            }
            __syncthreads();
        }
        if (cok)
            for (int j = wv; j < kn; j += 4) *(float4*)(part + ((r * K) + k0 + j) * (long)C + (long)c4 * 4) = s_acc[j][lane];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_region_wsum_reduce(const float* __restrict__ part, int N, int K, int C, int S,
                                                            float* __restrict__ out, long ldo) {
    const int C4 = C >> 2;
    const long items = (long)N * K * C4;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int c4 = (int)(it % C4);
        const long nk = it / C4;
        const int k = (int)(nk % K), n = (int)(nk / K);
        float4 acc = o4ld(part + (((long)n * S) * K + k) * (long)C + (long)c4 * 4);
        for (int sl = 1; sl < S; ++sl) acc = o4add(acc, o4ld(part + (((long)n * S + sl) * K + k) * (long)C + (long)c4 * 4));
        *(float4*)(out + nk * ldo + (long)c4 * 4) = acc;
    }
}

// ---- per-pixel building blocks: one wave, OCR_PX pixels of one image, lane l of register r <-> region 64 r + l ---------------------
// d[i][r] (lane l) += dot(rows[64 r + l], xrow_i) for every region < K; every lane of the wave must call it (DPP wave sums)
__device__ __forceinline__ void ocr_dots(const float* __restrict__ rows, long ldr, int K, const float* __restrict__ xrow, long ldx,
                                         int npx, int C4, float (&d)[OCR_PX][OCR_KREGS]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < OCR_PX; ++i)
#pragma unroll
        for (int r = 0; r < OCR_KREGS; ++r) d[i][r] = 0.f;
    for (int cb = 0; cb < C4; cb += 64) {
        const int c4 = cb + lane;
        const bool ok = c4 < C4;
        float4 xv[OCR_PX];
#pragma unroll
        for (int i = 0; i < OCR_PX; ++i) xv[i] = (ok && i < npx) ? o4ld(xrow + i * ldx + (long)c4 * 4) : o4zero();
#pragma unroll
        for (int r = 0; r < OCR_KREGS; ++r) {
            const int kn = min(OCR_KCHUNK, K - r * OCR_KCHUNK);
            for (int j = 0; j < kn; ++j) {
                const float4 kv = ok ? o4ld(rows + (long)(r * OCR_KCHUNK + j) * ldr + (long)c4 * 4) : o4zero();
#pragma unroll
                for (int i = 0; i < OCR_PX; ++i) {
                    const float tot = wave_sum_sgpr(o4dot(kv, xv[i]));
                    d[i][r] = lane == j ? d[i][r] + tot : d[i][r];
                }
            }
        }
    }
}

// out_i[c] = sum over regions ascending of wt[i][region] * rows[region][c] (+ add_i[c]) for the npx pixels; rows == nullptr: K = 0
__device__ __forceinline__ void ocr_mix(const float* __restrict__ rows, long ldr, int K, const float (&wt)[OCR_PX][OCR_KREGS],
                                        const float* __restrict__ add, long ldadd, int npx, int C4, float* __restrict__ out, long ldo) {
    const int lane = threadIdx.x & 63;
    for (int cb = 0; cb < C4; cb += 64) {
        const int c4 = cb + lane;
        const bool ok = c4 < C4;
        float4 acc[OCR_PX];
#pragma unroll
        for (int i = 0; i < OCR_PX; ++i) acc[i] = o4zero();
#pragma unroll
        for (int r = 0; r < OCR_KREGS; ++r) {
            const int kn = min(OCR_KCHUNK, K - r * OCR_KCHUNK);
            for (int j = 0; j < kn; ++j) {
                const float4 kv = ok ? o4ld(rows + (long)(r * OCR_KCHUNK + j) * ldr + (long)c4 * 4) : o4zero();
#pragma unroll
                for (int i = 0; i < OCR_PX; ++i) acc[i] = o4fma(lane_get(wt[i][r], j), kv, acc[i]);
            }
        }
        if (ok) {
#pragma unroll
            for (int i = 0; i < OCR_PX; ++i) {
                if (i < npx) {
                    float4 o = acc[i];
                    if (add != nullptr) o = o4add(o, o4ld(add + i * ldadd + (long)c4 * 4));
                    *(float4*)(out + i * ldo + (long)c4 * 4) = o;
                }
            }
        }
    }
}

// wave g of the launch takes the pixel group g: image n, pixels pl .. pl + npx - 1
#define OCR_GROUP_LOOP()                                                                                                          \
    const int lane = threadIdx.x & 63;                                                                                            \
    const int gpi = (HW + OCR_PX - 1) / OCR_PX;                                                                                   \
    const long groups = (long)N * gpi;                                                                                            \
    for (long g_ = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); g_ < groups; g_ += (long)gridDim.x * 4)
#define OCR_GROUP_DECODE()                                                                                                        \
    const int n = (int)(g_ / gpi), pl = (int)(g_ % gpi) * OCR_PX, npx = min(OCR_PX, HW - pl);                                     \
    const long row = (long)n * HW + pl;

__global__ void __launch_bounds__(256) k_region_attn_fwd(const float* __restrict__ q, long ldq, const float* __restrict__ kk, long ldk,
                                                         const float* __restrict__ v, long ldv, float scale, int N, int HW, int K, int D,
                                                         float* __restrict__ w, long ldw, float* __restrict__ y, long ldy) {
    OCR_GROUP_LOOP() {
        OCR_GROUP_DECODE()
        float d[OCR_PX][OCR_KREGS];
        ocr_dots(kk + (long)n * K * ldk, ldk, K, q + row * ldq, ldq, npx, D >> 2, d);
#pragma unroll
        for (int i = 0; i < OCR_PX; ++i) {
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r) {
                d[i][r] = r * OCR_KCHUNK + lane < K ? __fmul_rn(scale, d[i][r]) : -INFINITY;
                mx = fmaxf(mx, d[i][r]);
            }
            mx = wave_max(mx);
            float z = 0.f;
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r) {
                d[i][r] = r * OCR_KCHUNK + lane < K ? expf(__fsub_rn(d[i][r], mx)) : 0.f;
                z = r == 0 ? d[i][r] : z + d[i][r];
            }
            z = wave_sum_sgpr(z);
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r) {
                d[i][r] = __fdiv_rn(d[i][r], z);
                if (i < npx && r * OCR_KCHUNK + lane < K) w[(row + i) * ldw + r * OCR_KCHUNK + lane] = d[i][r];
            }
        }
        ocr_mix(v + (long)n * K * ldv, ldv, K, d, nullptr, 0, npx, D >> 2, y + row * ldy, ldy);
    }
}

// e (workspace, [N * HW][K] dense) is written whenever it is not null
__global__ void __launch_bounds__(256) k_region_attn_bwd(const float* __restrict__ gy, long ldg, const float* __restrict__ w, long ldw,
                                                         const float* __restrict__ kk, long ldk, const float* __restrict__ v, long ldv,
                                                         float scale, int N, int HW, int K, int D, float* __restrict__ e,
                                                         float* __restrict__ dq, long lddq) {
    OCR_GROUP_LOOP() {
        OCR_GROUP_DECODE()
        float d[OCR_PX][OCR_KREGS];
        ocr_dots(v + (long)n * K * ldv, ldv, K, gy + row * ldg, ldg, npx, D >> 2, d);
#pragma unroll
        for (int i = 0; i < OCR_PX; ++i) {
            float wr[OCR_KREGS], sd = 0.f;
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r) {
                wr[r] = (i < npx && r * OCR_KCHUNK + lane < K) ? w[(row + i) * ldw + r * OCR_KCHUNK + lane] : 0.f;
                sd = r == 0 ? __fmul_rn(wr[r], d[i][r]) : __fmaf_rn(wr[r], d[i][r], sd);
            }
            sd = wave_sum_sgpr(sd);
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r) {
                d[i][r] = __fmul_rn(__fmul_rn(scale, wr[r]), __fsub_rn(d[i][r], sd));
                if (e != nullptr && i < npx && r * OCR_KCHUNK + lane < K) e[(row + i) * (long)K + r * OCR_KCHUNK + lane] = d[i][r];
            }
        }
        if (dq != nullptr) ocr_mix(kk + (long)n * K * ldk, ldk, K, d, nullptr, 0, npx, D >> 2, dq + row * lddq, lddq);
    }
}

// c[n * K + k] = g_f[n, k, :] . f[n, k, :]: one wave per row
__global__ void __launch_bounds__(256) k_region_rowdot(const float* __restrict__ g, long ldg, const float* __restrict__ f, long ldf, int rows,
                                                       int C, float* __restrict__ c) {
    const int lane = threadIdx.x & 63, C4 = C >> 2;
    for (int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); r < rows; r += gridDim.x * 4) {
        float p = 0.f;
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const float4 a = o4ld(g + (long)r * ldg + (long)c4 * 4), b = o4ld(f + (long)r * ldf + (long)c4 * 4);
            p = __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmaf_rn(a.x, b.x, p))));
        }
        // (the trip counts differ between lanes: all 64 are back here before the DPP sum)
        p = wave_sum_sgpr(p);
        if (lane == 0) c[r] = p;
    }
}

// g == nullptr: no gradient reached f (ds = 0, dx = add or 0); dx or ds may be null (not both)
__global__ void __launch_bounds__(256) k_region_pool_bwd(const float* __restrict__ g, long ldg, const float* __restrict__ m, long ldm,
                                                         const float* __restrict__ x, long ldx, const float* __restrict__ c,
                                                         const float* __restrict__ add, long ldadd, float scale, int N, int HW, int K,
                                                         int C, float* __restrict__ dx, long lddx, float* __restrict__ ds, long ldds) {
    OCR_GROUP_LOOP() {
        OCR_GROUP_DECODE()
        const int Kg = g != nullptr ? K : 0;
        float mr[OCR_PX][OCR_KREGS];
#pragma unroll
        for (int i = 0; i < OCR_PX; ++i)
#pragma unroll
            for (int r = 0; r < OCR_KREGS; ++r)
                mr[i][r] = (i < npx && r * OCR_KCHUNK + lane < K) ? m[(row + i) * ldm + r * OCR_KCHUNK + lane] : 0.f;
        if (ds != nullptr) {
            float d[OCR_PX][OCR_KREGS] = {};
            if (Kg) ocr_dots(g + (long)n * K * ldg, ldg, Kg, x + row * ldx, ldx, npx, C >> 2, d);     // (x and c are read only here)
#pragma unroll
            for (int i = 0; i < OCR_PX; ++i)
#pragma unroll
                for (int r = 0; r < OCR_KREGS; ++r) {
                    const int k = r * OCR_KCHUNK + lane;
                    if (i < npx && k < K)
                        ds[(row + i) * ldds + k] = Kg ? __fmul_rn(__fmul_rn(scale, mr[i][r]), __fsub_rn(d[i][r], c[(long)n * K + k])) : 0.f;
                }
        }
        if (dx != nullptr)
            ocr_mix(g + (long)n * K * ldg, ldg, Kg, mr, add != nullptr ? add + row * ldadd : nullptr, ldadd, npx, C >> 2, dx + row * lddx,
                    lddx);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool ocr_shape_ok(int N, int HW, int K, int C) {
    return N > 0 && HW > 0 && K >= 1 && K <= OCR_MAX_K && C > 0 && C % 4 == 0 && (long)N * HW < (1L << 31);
}
static bool ocr_rows_ok(const void* p, long ld, int width) {       // a channel-wide tensor: float4 rows
    return p != nullptr && ld >= width && ld % 4 == 0 && ((uintptr_t)p & 15) == 0;
}
static bool ocr_cols_ok(const void* p, long ld, int K) {           // a K-wide tensor: scalar accesses, any pitch >= K
    return p != nullptr && ld >= K;
}
static inline int ocr_slabs(int HW) { return (HW + OCR_SLAB - 1) / OCR_SLAB; }
static inline long ocr_up4(long n) { return (n + 3) & ~3L; }
static inline unsigned ocr_grid(long items) { return (unsigned)(items < OCR_MAX_BLOCKS ? (items < 1 ? 1 : items) : OCR_MAX_BLOCKS); }

static size_t ocr_wsum_floats(int N, int HW, int K, int C) { return (size_t)N * ocr_slabs(HW) * K * C; }

// out[n, k, :] = sum_p a[n, p, k] x[n, p, :]; part: ocr_wsum_floats() floats, 16-byte aligned
static int ocr_wsum(const float* a, long lda, const float* x, long ldx, int N, int HW, int K, int C, float* part, float* out, long ldo,
                    hipStream_t stream) {
    const int S = ocr_slabs(HW), C4 = C / 4;
    const long items = (long)N * S * ((C4 + 63) / 64) * ((K + OCR_KT - 1) / OCR_KT);
    U2PL_LAUNCH(k_region_wsum, dim3(ocr_grid(items)), dim3(256), 0, stream, a, lda, x, ldx, N, HW, K, C, S, part);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_region_wsum_reduce, dim3(ocr_grid(((long)N * K * C4 + 255) / 256)), dim3(256), 0, stream, part, N, K, C, S, out, ldo);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API size_t u2pl_region_pool_fwd_ws_floats(int N, int HW, int K, int C) {
    if (!ocr_shape_ok(N, HW, K, C)) return 0;
    return (size_t)2 * ocr_up4((long)N * ocr_slabs(HW) * K) + ocr_wsum_floats(N, HW, K, C);
}
U2PL_API size_t u2pl_region_pool_bwd_ws_floats(int N, int HW, int K, int C) {
    if (!ocr_shape_ok(N, HW, K, C)) return 0;
    return (size_t)ocr_up4((long)N * K);
}
U2PL_API size_t u2pl_region_attn_bwd_ws_floats(int N, int HW, int K, int D) {
    if (!ocr_shape_ok(N, HW, K, D)) return 0;
    return (size_t)ocr_up4((long)N * HW * K) + ocr_wsum_floats(N, HW, K, D);
}

U2PL_API int u2pl_region_pool_fwd_f32(const float* s, long lds, const float* x, long ldx, float scale, int N, int HW, int K, int C,
                                      float* m, long ldm, float* f, long ldf, float* ws, hipStream_t stream) {
    if (!ocr_shape_ok(N, HW, K, C) || !ocr_cols_ok(s, lds, K) || !ocr_rows_ok(x, ldx, C) || !ocr_cols_ok(m, ldm, K) ||
        !ocr_rows_ok(f, ldf, C) || !ocr_rows_ok(ws, 4, 4))
        return U2PL_EINVAL;
    const int S = ocr_slabs(HW);
    const long nsk = ocr_up4((long)N * S * K);
    float *wmax = ws, *wsum = ws + nsk, *part = ws + 2 * nsk;
    const unsigned gs = ocr_grid((long)N * S);
    U2PL_LAUNCH(k_region_colmax, dim3(gs), dim3(256), 0, stream, s, lds, scale, N, HW, K, S, wmax);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_region_colsum, dim3(gs), dim3(256), 0, stream, s, lds, scale, N, HW, K, S, wmax, wsum);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_region_colnorm, dim3(gs), dim3(256), 0, stream, s, lds, scale, N, HW, K, S, wmax, wsum, m, ldm);
    U2PL_LAUNCH_CHECK();
    return ocr_wsum(m, ldm, x, ldx, N, HW, K, C, part, f, ldf, stream);
}

U2PL_API int u2pl_region_pool_bwd_f32(const float* g_f, long ldg, const float* m, long ldm, const float* x, long ldx, const float* f,
                                      long ldf, const float* add, long ldadd, float scale, int N, int HW, int K, int C, float* dx,
                                      long lddx, float* ds, long ldds, float* ws, hipStream_t stream) {
    if (!ocr_shape_ok(N, HW, K, C) || !ocr_cols_ok(m, ldm, K) || (!dx && !ds) || !ocr_rows_ok(ws, 4, 4)) return U2PL_EINVAL;
    if (g_f && !ocr_rows_ok(g_f, ldg, C)) return U2PL_EINVAL;
    if (add && !ocr_rows_ok(add, ldadd, C)) return U2PL_EINVAL;
    if (dx && !ocr_rows_ok(dx, lddx, C)) return U2PL_EINVAL;
    if (ds && (!ocr_cols_ok(ds, ldds, K) || (g_f && (!ocr_rows_ok(x, ldx, C) || !ocr_rows_ok(f, ldf, C))))) return U2PL_EINVAL;
    if (g_f && ds) {
        U2PL_LAUNCH(k_region_rowdot, dim3(ocr_grid(((long)N * K + 3) / 4)), dim3(256), 0, stream, g_f, ldg, f, ldf, N * K, C, ws);
        U2PL_LAUNCH_CHECK();
    }
    const long groups = (long)N * ((HW + OCR_PX - 1) / OCR_PX);
    U2PL_LAUNCH(k_region_pool_bwd, dim3(ocr_grid((groups + 3) / 4)), dim3(256), 0, stream, g_f, ldg, m, ldm, x, ldx, ws, add, ldadd, scale,
                N, HW, K, C, dx, lddx, ds, ldds);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API int u2pl_region_attn_fwd_f32(const float* q, long ldq, const float* kk, long ldk, const float* v, long ldv, float scale, int N,
                                      int HW, int K, int D, float* w, long ldw, float* y, long ldy, hipStream_t stream) {
    if (!ocr_shape_ok(N, HW, K, D) || !ocr_rows_ok(q, ldq, D) || !ocr_rows_ok(kk, ldk, D) || !ocr_rows_ok(v, ldv, D) ||
        !ocr_cols_ok(w, ldw, K) || !ocr_rows_ok(y, ldy, D))
        return U2PL_EINVAL;
    const long groups = (long)N * ((HW + OCR_PX - 1) / OCR_PX);
    U2PL_LAUNCH(k_region_attn_fwd, dim3(ocr_grid((groups + 3) / 4)), dim3(256), 0, stream, q, ldq, kk, ldk, v, ldv, scale, N, HW, K, D, w,
                ldw, y, ldy);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API int u2pl_region_attn_bwd_f32(const float* g_y, long ldg, const float* w, long ldw, const float* q, long ldq, const float* kk,
                                      long ldk, const float* v, long ldv, float scale, int N, int HW, int K, int D, float* dq, long lddq,
                                      float* dk, long lddk, float* dv, long lddv, float* ws, hipStream_t stream) {
    if (!ocr_shape_ok(N, HW, K, D) || !ocr_rows_ok(g_y, ldg, D) || !ocr_cols_ok(w, ldw, K) || !ocr_rows_ok(kk, ldk, D) ||
        !ocr_rows_ok(v, ldv, D) || (!dq && !dk && !dv) || !ocr_rows_ok(ws, 4, 4))
        return U2PL_EINVAL;
    if (dq && !ocr_rows_ok(dq, lddq, D)) return U2PL_EINVAL;
    if (dk && (!ocr_rows_ok(dk, lddk, D) || !ocr_rows_ok(q, ldq, D))) return U2PL_EINVAL;
    if (dv && !ocr_rows_ok(dv, lddv, D)) return U2PL_EINVAL;
    float *e = ws, *part = ws + ocr_up4((long)N * HW * K);
    if (dq || dk) {
        const long groups = (long)N * ((HW + OCR_PX - 1) / OCR_PX);
        U2PL_LAUNCH(k_region_attn_bwd, dim3(ocr_grid((groups + 3) / 4)), dim3(256), 0, stream, g_y, ldg, w, ldw, kk, ldk, v, ldv, scale, N,
                    HW, K, D, dk ? e : nullptr, dq, lddq);
        U2PL_LAUNCH_CHECK();
    }
    if (dv) {
        const int rc = ocr_wsum(w, ldw, g_y, ldg, N, HW, K, D, part, dv, lddv, stream);
        if (rc) return rc;
    }
    if (dk) return ocr_wsum(e, K, q, ldq, N, HW, K, D, part, dk, lddk, stream);
    return 0;
}
