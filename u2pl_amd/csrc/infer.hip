// Prediction-side kernels (reference infer.py:118-134, eval.py:294-300):
//   u2pl_infer_input_u8_f32   decoded uint8 image -> normalised, resized network input (channels_last)
//   u2pl_predict_map_f32      low-resolution logits -> uint8 label map (+ RGB image through a palette)
//   u2pl_window_fuse_f32      one view's low-resolution logits -> (mirrored) (softmax) += into a window of the accumulator
//   u2pl_predict_entropy_f32  low-resolution scores -> uint8 label map + softmax entropy map (logits or class weights)
//   u2pl_reliable_map_u8      entropy >= device-resident threshold -> label 255, + RGB through a palette, + entropy heat bytes
// All use ac_coord and the three-FMA expression of k_bilinear_up (reliability.hip), in that order, so an interpolated
// value has the bits u2pl_bilinear_up_f32 would have stored; none writes a full-resolution float tensor per class besides
// the accumulator itself and the entropy map.
#include "common.h"
#include "u2pl_hip.h"

// ---------------------------------------------------------------------------
// A thread owns 4 consecutive output pixels of one row (one dword of labels, three dwords of RGB); lanes run along the
// row, so a wave stores 256 contiguous label bytes and 768 contiguous RGB bytes.  Per class it reads the 2 x 2 taps of
// each pixel from the low-resolution tensor (<= 11 MB: L2 resident, neighbouring pixels share taps in the L1) and
// keeps the running maximum: classes upward, replaced on strict '>', i.e. the lowest index wins a tie (k_confusion's
// rule, losses.hip).  A quad whose store address is not dword aligned (W % 4 != 0) or that hangs over the end of the
// row takes byte stores.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_predict_map(const float* __restrict__ in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H, int W,
              unsigned char* __restrict__ label, const unsigned char* __restrict__ palette, unsigned char* __restrict__ rgb,
              float sy, float sx) {
    __shared__ unsigned s_pal[256];   // R | G << 8 | B << 16
    const bool color = palette != nullptr && rgb != nullptr;
    if (color) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x)
            s_pal[i] = (unsigned)palette[3 * i] | ((unsigned)palette[3 * i + 1] << 8) | ((unsigned)palette[3 * i + 2] << 16);
        __syncthreads();
    }
    const int Wq = (W + 3) >> 2;
    const long total = (long)N * H * Wq;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int q = (int)(p % Wq);
        const long t = p / Wq;
        const int oy = (int)(t % H);
        const int n = (int)(t / H);
        const int ox0 = q << 2;
        const AcCoord cy = ac_coord(oy, sy, h);
        const long r0 = cy.i0 * sh, r1 = cy.i1 * sh;
        long c0[4], c1[4];
        float l0[4], l1[4], best[4];
        int am[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const AcCoord cx = ac_coord(min(ox0 + j, W - 1), sx, w);   // past the row end: recompute the last pixel, store nothing
            c0[j] = cx.i0 * sw;
            c1[j] = cx.i1 * sw;
            l0[j] = cx.l0;
            l1[j] = cx.l1;
            am[j] = 0;
            best[j] = 0.f;
        }
        const float* b = in + n * sn;
        for (int c = 0; c < C; ++c) {
            const float* t0 = b + c * sc + r0;
            const float* t1 = b + c * sc + r1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float top = __fmaf_rn(l0[j], t0[c0[j]], __fmul_rn(l1[j], t0[c1[j]]));
                const float bot = __fmaf_rn(l0[j], t1[c0[j]], __fmul_rn(l1[j], t1[c1[j]]));
                const float v = __fmaf_rn(cy.l0, top, __fmul_rn(cy.l1, bot));
                if (c == 0) best[j] = v;
                else if (v > best[j]) { best[j] = v; am[j] = c; }
            }
        }
        const long px = ((long)n * H + oy) * W + ox0;
        const bool full = ox0 + 4 <= W;
        unsigned char* lp = label + px;
        if (full && ((uintptr_t)lp & 3) == 0) {
            *(unsigned*)lp = (unsigned)am[0] | ((unsigned)am[1] << 8) | ((unsigned)am[2] << 16) | ((unsigned)am[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox0 + j < W) lp[j] = (unsigned char)am[j];
        }
        if (color) {
            const unsigned p0 = s_pal[am[0]], p1 = s_pal[am[1]], p2 = s_pal[am[2]], p3 = s_pal[am[3]];
            unsigned char* cp = rgb + 3 * px;
            if (full && ((uintptr_t)cp & 3) == 0) {
                unsigned* d = (unsigned*)cp;
                d[0] = p0 | (p1 << 24);
                d[1] = (p1 >> 8) | (p2 << 16);
                d[2] = (p2 >> 16) | (p3 << 8);
            } else {
                const unsigned pp[4] = {p0, p1, p2, p3};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ox0 + j < W) {
                        cp[3 * j] = (unsigned char)pp[j];
                        cp[3 * j + 1] = (unsigned char)(pp[j] >> 8);
                        cp[3 * j + 2] = (unsigned char)(pp[j] >> 16);
                    }
            }
        }
    }
}

U2PL_API int u2pl_predict_map_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H,
                                  int W, unsigned char* label, const unsigned char* palette, unsigned char* rgb,
                                  hipStream_t stream) {
    if (C > 256 || h < 1 || w < 1 || H < 0 || W < 0 || !in || !label) return U2PL_EINVAL;   // a label is one byte
    if (N <= 0 || C <= 0 || H == 0 || W == 0) return 0;
    const long total = (long)N * H * ((W + 3) >> 2);
    U2PL_LAUNCH(k_predict_map, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, stream, in, sn, sc, sh, sw, N, C, h, w, H,
                W, label, palette, rgb, ac_scale_host(h, H), ac_scale_host(w, W));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// out[oy][ox][c] = bilinear(align_corners=True) of lut[c][img[y][x][c]]: the normalisation is a gather from a table the
// host fills ((v - mean) / std evaluated in float64 and rounded once, as the reference's numpy expression does), so
// the kernel holds no arithmetic of its own besides the interpolation.  One thread per output pixel: 12 contiguous
// bytes per lane.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_infer_input(const unsigned char* __restrict__ img, int h, int w, const float* __restrict__ lut, float* __restrict__ out,
              int H, int W, float sy, float sx) {
    __shared__ float s_lut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) s_lut[i] = lut[i];
    __syncthreads();
    const long total = (long)H * W;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int ox = (int)(p % W), oy = (int)(p / W);
        const AcCoord cy = ac_coord(oy, sy, h), cx = ac_coord(ox, sx, w);
        const unsigned char* p00 = img + 3 * ((long)cy.i0 * w + cx.i0);
        const unsigned char* p01 = img + 3 * ((long)cy.i0 * w + cx.i1);
        const unsigned char* p10 = img + 3 * ((long)cy.i1 * w + cx.i0);
        const unsigned char* p11 = img + 3 * ((long)cy.i1 * w + cx.i1);
        float* o = out + 3 * p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* l = s_lut + 256 * c;
            const float top = __fmaf_rn(cx.l0, l[p00[c]], __fmul_rn(cx.l1, l[p01[c]]));
            const float bot = __fmaf_rn(cx.l0, l[p10[c]], __fmul_rn(cx.l1, l[p11[c]]));
            o[c] = __fmaf_rn(cy.l0, top, __fmul_rn(cy.l1, bot));
        }
    }
}

U2PL_API int u2pl_infer_input_u8_f32(const unsigned char* img_hwc, int h, int w, const float* lut, float* out_hwc, int H,
                                     int W, hipStream_t stream) {
    if (h < 1 || w < 1 || H < 0 || W < 0 || !img_hwc || !lut || !out_hwc) return U2PL_EINVAL;
    const long total = (long)H * W;
    if (total == 0) return 0;
    U2PL_LAUNCH(k_infer_input, dim3(grid_for(total, 256)), dim3(256), 0, stream, img_hwc, h, w, lut, out_hwc, H, W,
                ac_scale_host(h, H), ac_scale_host(w, W));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// Test-time flip / probability fusion (the block the reference leaves commented out in eval.py:166-180): one view's
// low-resolution logits are interpolated to the window size, mirrored back when the view was a mirrored image, turned into
// class probabilities, weighted and added into the window of the accumulator.  A thread owns 4 consecutive window pixels of
// one row and lanes run along the row, so every class plane is read and written in contiguous runs: 16-byte accesses when the
// quad is whole and its address allows (w0 and W are arbitrary, and the alignment changes from plane to plane), scalar ones
// otherwise.  C is a runtime value: instead of keeping v[0..C) per thread (a runtime-indexed array lives in scratch) the
// classes are swept three times -- maximum, sum of exponentials (classes upward), write -- and the taps recomputed; the
// low-resolution tensor is L2 resident.  Every output element has one owner and there are no atomics: windows are successive
// launches on one stream, and two runs give the same bits.  expf is the ~1 ulp library exponential on purpose (the error of
// the fast intrinsic grows with |v - m|).
// ---------------------------------------------------------------------------
template <bool SOFTMAX>
__global__ void __launch_bounds__(256)
k_window_fuse(float* __restrict__ pred, float* __restrict__ count, int C, int H, int W, const float* __restrict__ in, long sc,
              long sh, long sw, int h, int w, int h0, int w0, int hc, int wc, int flip, float weight, int bump, float sy,
              float sx) {
    const int Wq = (wc + 3) >> 2;
    const long total = (long)hc * Wq;
    const long plane = (long)H * W;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int q = (int)(p % Wq);
        const int y = (int)(p / Wq);
        const int x0 = q << 2;
        const AcCoord cy = ac_coord(y, sy, h);
        const long r0 = cy.i0 * sh, r1 = cy.i1 * sh;
        long c0[4], c1[4];
        float l0[4], l1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = min(x0 + j, wc - 1);   // past the window's edge: recompute its last pixel, store nothing
            const AcCoord cx = ac_coord(flip ? wc - 1 - x : x, sx, w);
            c0[j] = cx.i0 * sw;
            c1[j] = cx.i1 * sw;
            l0[j] = cx.l0;
            l1[j] = cx.l1;
        }
        auto value = [&](const float* t0, const float* t1, int j) {
            const float top = __fmaf_rn(l0[j], t0[c0[j]], __fmul_rn(l1[j], t0[c1[j]]));
            const float bot = __fmaf_rn(l0[j], t1[c0[j]], __fmul_rn(l1[j], t1[c1[j]]));
            return __fmaf_rn(cy.l0, top, __fmul_rn(cy.l1, bot));
        };
        float m[4] = {0.f, 0.f, 0.f, 0.f}, sum[4] = {0.f, 0.f, 0.f, 0.f};
        if (SOFTMAX) {
            for (int c = 0; c < C; ++c) {
                const float* t0 = in + c * sc + r0;
                const float* t1 = in + c * sc + r1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = value(t0, t1, j);
                    m[j] = c == 0 ? v : fmaxf(m[j], v);
                }
            }
            for (int c = 0; c < C; ++c) {
                const float* t0 = in + c * sc + r0;
                const float* t1 = in + c * sc + r1;
#pragma unroll
                for (int j = 0; j < 4; ++j) sum[j] = __fadd_rn(sum[j], expf(__fsub_rn(value(t0, t1, j), m[j])));
            }
        }
        const long px = (long)(h0 + y) * W + w0 + x0;
        const bool full = x0 + 4 <= wc;
        for (int c = 0; c < C; ++c) {
            const float* t0 = in + c * sc + r0;
            const float* t1 = in + c * sc + r1;
            float s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = value(t0, t1, j);
                s[j] = __fmul_rn(weight, SOFTMAX ? __fdiv_rn(expf(__fsub_rn(v, m[j])), sum[j]) : v);
            }
            float* o = pred + c * plane + px;
            if (full && ((uintptr_t)o & 15) == 0) {
                float4 a = *(float4*)o;
                a.x = __fadd_rn(a.x, s[0]);
                a.y = __fadd_rn(a.y, s[1]);
                a.z = __fadd_rn(a.z, s[2]);
                a.w = __fadd_rn(a.w, s[3]);
                *(float4*)o = a;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < wc) o[j] = __fadd_rn(o[j], s[j]);
            }
        }
        if (bump) {
            float* o = count + px;
            if (full && ((uintptr_t)o & 15) == 0) {
                float4 a = *(float4*)o;
                a.x += 1.0f;
                a.y += 1.0f;
                a.z += 1.0f;
                a.w += 1.0f;
                *(float4*)o = a;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < wc) o[j] += 1.0f;
            }
        }
    }
}

U2PL_API int u2pl_window_fuse_f32(float* pred, float* count, int C, int H, int W, const float* in, long sc, long sh, long sw,
                                  int h, int w, int h0, int w0, int hc, int wc, int flip, int softmax, float weight, int bump,
                                  hipStream_t stream) {
    if (!pred || !in || (bump && !count) || C < 1 || C > 256 || h < 1 || w < 1) return U2PL_EINVAL;
    if (h0 < 0 || w0 < 0 || hc < 0 || wc < 0 || h0 > H - hc || w0 > W - wc) return U2PL_EINVAL;
    const long total = (long)hc * ((wc + 3) >> 2);
    if (total == 0) return 0;
    const dim3 grid(grid_for(total, 256, 256 * 32));
    if (softmax)
        U2PL_LAUNCH(k_window_fuse<true>, grid, dim3(256), 0, stream, pred, count, C, H, W, in, sc, sh, sw, h, w, h0, w0, hc, wc,
                    flip, weight, bump, ac_scale_host(h, hc), ac_scale_host(w, wc));
    else
        U2PL_LAUNCH(k_window_fuse<false>, grid, dim3(256), 0, stream, pred, count, C, H, W, in, sc, sh, sw, h, w, h0, w0, hc, wc,
                    flip, weight, bump, ac_scale_host(h, hc), ac_scale_host(w, wc));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// Reliability maps on the prediction side (the reference's compute_unsupervised_loss, loss_helper.py:30-48, read as an export
// rule): label and softmax entropy of a pixel from the low-resolution scores in one launch.  Ownership, taps and stores are
// k_predict_map's (4 consecutive pixels of a row per thread, one dword of labels and 16 bytes of entropy when the quad is whole
// and its address allows); C is a runtime value, so as in k_window_fuse the classes are swept twice and the taps recomputed
// instead of keeping z[0..C) per thread.  Sweep 1: arg-max by k_predict_map's rule (classes upward, strict '>') and, with it,
// the maximum (logits) or the sum S of the weights (PROB).  Sweep 2, classes upward:
//   logits  d = z_c - m, e = expf(d), s += e, t += e * d;  entropy = logf(s) - t / s      (k_entropy_up's expression, term for
//           term and in its order: the bits u2pl_entropy_up_f32 stores)
//   PROB    p = a_c / S, entropy = -sum p * logf(p) over the classes with p > 0; S <= 0: logf(C), a pixel that knows nothing.
//           A negative weight contributes nothing and an infinite S gives p = 0: never NaN for finite input.
// The select's pass-0 histogram is not filled here (hist0_flush is reliability.hip's): u2pl_select_f32 runs with hist0_done = 0.
// ---------------------------------------------------------------------------
template <bool PROB>
__global__ void __launch_bounds__(256)
k_predict_entropy(const float* __restrict__ in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H, int W,
                  unsigned char* __restrict__ label, float* __restrict__ ent, float sy, float sx) {
    const int Wq = (W + 3) >> 2;
    const long total = (long)N * H * Wq;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int q = (int)(p % Wq);
        const long t_ = p / Wq;
        const int oy = (int)(t_ % H);
        const int n = (int)(t_ / H);
        const int ox0 = q << 2;
        const AcCoord cy = ac_coord(oy, sy, h);
        const long r0 = cy.i0 * sh, r1 = cy.i1 * sh;
        long c0[4], c1[4];
        float l0[4], l1[4], best[4], m[4];   // m: the maximum (logits) | the sum of the weights (PROB)
        int am[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const AcCoord cx = ac_coord(min(ox0 + j, W - 1), sx, w);   // past the row end: recompute the last pixel, store nothing
            c0[j] = cx.i0 * sw;
            c1[j] = cx.i1 * sw;
            l0[j] = cx.l0;
            l1[j] = cx.l1;
            am[j] = 0;
            best[j] = 0.f;
            m[j] = 0.f;
        }
        const float* b = in + n * sn;
        auto value = [&](const float* t0, const float* t1, int j) {
            const float top = __fmaf_rn(l0[j], t0[c0[j]], __fmul_rn(l1[j], t0[c1[j]]));
            const float bot = __fmaf_rn(l0[j], t1[c0[j]], __fmul_rn(l1[j], t1[c1[j]]));
            return __fmaf_rn(cy.l0, top, __fmul_rn(cy.l1, bot));
        };
        for (int c = 0; c < C; ++c) {
            const float* t0 = b + c * sc + r0;
            const float* t1 = b + c * sc + r1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = value(t0, t1, j);
                if (c == 0) best[j] = v;
                else if (v > best[j]) { best[j] = v; am[j] = c; }
                if (PROB) m[j] = __fadd_rn(m[j], v);
                else m[j] = c == 0 ? v : fmaxf(m[j], v);
            }
        }
        float s[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            const float* t0 = b + c * sc + r0;
            const float* t1 = b + c * sc + r1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = value(t0, t1, j);
                if (PROB) {
                    const float pc = __fdiv_rn(v, m[j]);
                    t[j] = __fadd_rn(t[j], pc > 0.f ? __fmul_rn(pc, logf(pc)) : 0.f);
                } else {
                    const float d = v - m[j];
                    const float e = expf(d);
                    s[j] += e;
                    t[j] += e * d;
                }
            }
        }
        float e4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (PROB) e4[j] = m[j] > 0.f ? __fsub_rn(0.f, t[j]) : logf((float)C);
            else e4[j] = logf(s[j]) - t[j] / s[j];
        }
        const long px = ((long)n * H + oy) * W + ox0;
        const bool full = ox0 + 4 <= W;
        unsigned char* lp = label + px;
        if (full && ((uintptr_t)lp & 3) == 0) {
            *(unsigned*)lp = (unsigned)am[0] | ((unsigned)am[1] << 8) | ((unsigned)am[2] << 16) | ((unsigned)am[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox0 + j < W) lp[j] = (unsigned char)am[j];
        }
        float* ep = ent + px;
        if (full && ((uintptr_t)ep & 15) == 0) {
            *(float4*)ep = make_float4(e4[0], e4[1], e4[2], e4[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ox0 + j < W) ep[j] = e4[j];
        }
    }
}

U2PL_API int u2pl_predict_entropy_f32(const float* in, long sn, long sc, long sh, long sw, int N, int C, int h, int w, int H,
                                      int W, int prob, unsigned char* label, float* entropy, hipStream_t stream) {
    if (C < 1 || C > 256 || h < 1 || w < 1 || H < 1 || W < 1 || !in || !label || !entropy) return U2PL_EINVAL;
    if (N <= 0) return 0;
    const long total = (long)N * H * ((W + 3) >> 2);
    const dim3 grid(grid_for(total, 256, 256 * 32));
    if (prob)
        U2PL_LAUNCH(k_predict_entropy<true>, grid, dim3(256), 0, stream, in, sn, sc, sh, sw, N, C, h, w, H, W, label, entropy,
                    ac_scale_host(h, H), ac_scale_host(w, W));
    else
        U2PL_LAUNCH(k_predict_entropy<false>, grid, dim3(256), 0, stream, in, sn, sc, sh, sw, N, C, h, w, H, W, label, entropy,
                    ac_scale_host(h, H), ac_scale_host(w, W));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// The export rule itself, in place over n pixels: label[p] = 255 where entropy[p] >= *thr (entropy.ge(thresh),
// loss_helper.py:41), then the colour and the heat bytes of the pixel.  The threshold is read from device memory (the
// select's workspace), so the host never waits for it.  A thread owns 4 consecutive pixels: one dword of labels and of heat,
// 16 bytes of entropy, three dwords of RGB when the quad is whole and the address allows, bytes otherwise.  The dropped pixels
// are counted per thread, summed per block and added with one integer atomic per block: two runs give the same count.
// heat = clamp((int)(entropy * heat_scale + 0.5f), 0, 255), the product and the sum each rounded to fp32, which a numpy
// float32 expression restates bit for bit (the clamp is applied to the float, which gives the same byte and keeps the
// conversion in range).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_reliable_map(unsigned char* __restrict__ label, const float* __restrict__ ent, const unsigned* __restrict__ thr_bits, long n,
               const unsigned char* __restrict__ palette, unsigned char* __restrict__ rgb, unsigned char* __restrict__ heat,
               float heat_scale, unsigned* __restrict__ ndropped) {
    __shared__ unsigned s_pal[256];   // R | G << 8 | B << 16
    const bool color = palette != nullptr && rgb != nullptr;
    if (color) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x)
            s_pal[i] = (unsigned)palette[3 * i] | ((unsigned)palette[3 * i + 1] << 8) | ((unsigned)palette[3 * i + 2] << 16);
        __syncthreads();
    }
    const bool drop = thr_bits != nullptr;
    const float thr = drop ? __uint_as_float(*thr_bits) : 0.f;
    const long nq = (n + 3) >> 2;
    unsigned cnt = 0;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < nq; p += (long)gridDim.x * blockDim.x) {
        const long px = p << 2;
        const bool full = px + 4 <= n;
        unsigned char* lp = label + px;
        const float* ep = ent + px;
        const bool lal = full && ((uintptr_t)lp & 3) == 0;
        float e[4];
        unsigned lab[4];
        if (full && ((uintptr_t)ep & 15) == 0) {
            const float4 v = *(const float4*)ep;
            e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = px + j < n ? ep[j] : 0.f;
        }
        if (lal) {
            const unsigned v = *(const unsigned*)lp;
#pragma unroll
            for (int j = 0; j < 4; ++j) lab[j] = (v >> (8 * j)) & 255u;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) lab[j] = px + j < n ? lp[j] : 0u;
        }
        if (drop) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (px + j < n && e[j] >= thr) { lab[j] = 255u; ++cnt; }
            if (lal) {
                *(unsigned*)lp = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < n) lp[j] = (unsigned char)lab[j];
            }
        }
        if (heat) {
            unsigned hb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                hb[j] = (unsigned)(int)fminf(fmaxf(__fadd_rn(__fmul_rn(e[j], heat_scale), 0.5f), 0.f), 255.f);
            unsigned char* hp = heat + px;
            if (full && ((uintptr_t)hp & 3) == 0) {
                *(unsigned*)hp = hb[0] | (hb[1] << 8) | (hb[2] << 16) | (hb[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < n) hp[j] = (unsigned char)hb[j];
            }
        }
        if (color) {
            const unsigned p0 = s_pal[lab[0]], p1 = s_pal[lab[1]], p2 = s_pal[lab[2]], p3 = s_pal[lab[3]];
            unsigned char* cp = rgb + 3 * px;
            if (full && ((uintptr_t)cp & 3) == 0) {
                unsigned* d = (unsigned*)cp;
                d[0] = p0 | (p1 << 24);
                d[1] = (p1 >> 8) | (p2 << 16);
                d[2] = (p2 >> 16) | (p3 << 8);
            } else {
                const unsigned pp[4] = {p0, p1, p2, p3};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (px + j < n) {
                        cp[3 * j] = (unsigned char)pp[j];
                        cp[3 * j + 1] = (unsigned char)(pp[j] >> 8);
                        cp[3 * j + 2] = (unsigned char)(pp[j] >> 16);
                    }
            }
        }
    }
    if (ndropped != nullptr) block_count_flush(cnt, ndropped);
}

U2PL_API int u2pl_reliable_map_u8(unsigned char* label, const float* entropy, const unsigned* thr_bits, long n,
                                  const unsigned char* palette, unsigned char* rgb, unsigned char* heat, float heat_scale,
                                  unsigned* ndropped, hipStream_t stream) {
    if (!label || !entropy || (palette == nullptr) != (rgb == nullptr)) return U2PL_EINVAL;
    if (n <= 0) return 0;
    U2PL_LAUNCH(k_reliable_map, dim3(grid_for((n + 3) >> 2, 256, 1024)), dim3(256), 0, stream, label, entropy, thr_bits, n, palette,
                rgb, heat, heat_scale, ndropped);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// out[i] = lut[in[i]] over n bytes (--raw_ids: class indices -> the dataset's raw ids; 255 -> the raw ignore value).  The
// table sits in LDS: a thread looks up 16 bytes per 16-byte load, so lookups, not memory, set the pace, and the LDS
// serves 64 byte gathers per instruction where the vector cache would take them a few lanes at a time.  The first
// (-in) mod 16 bytes and the last n mod 16 are done bytewise by one thread; every chunk between is ONE aligned 16-byte load
// and, when `out` is aligned like `in` (in place: always), one 16-byte store -- dwords or bytes otherwise.  A thread
// has read its chunk before it writes it and no other thread touches it, so out == in is allowed (a partial overlap is not).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_lut_u8(const unsigned char* __restrict__ lut, const unsigned char* in, unsigned char* out, long n, long head, long body) {
    __shared__ unsigned char s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];        // blockDim.x == 256
    __syncthreads();
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long p = tid; p < body; p += (long)gridDim.x * blockDim.x) {
        const long o = head + (p << 4);
        const uint4 v = *(const uint4*)(in + o);
        const unsigned src[4] = {v.x, v.y, v.z, v.w};
        unsigned dst[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            dst[j] = (unsigned)s_lut[src[j] & 255u] | ((unsigned)s_lut[(src[j] >> 8) & 255u] << 8) |
                     ((unsigned)s_lut[(src[j] >> 16) & 255u] << 16) | ((unsigned)s_lut[src[j] >> 24] << 24);
        unsigned char* q = out + o;
        if (((uintptr_t)q & 15) == 0) {
            *(uint4*)q = make_uint4(dst[0], dst[1], dst[2], dst[3]);
        } else if (((uintptr_t)q & 3) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ((unsigned*)q)[j] = dst[j];
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = (unsigned char)(dst[j >> 2] >> (8 * (j & 3)));
        }
    }
    if (tid == 0) {
        for (long i = 0; i < head; ++i) out[i] = s_lut[in[i]];
        for (long i = head + (body << 4); i < n; ++i) out[i] = s_lut[in[i]];
    }
}

U2PL_API int u2pl_lut_u8(const unsigned char* in, unsigned char* out, long n, const unsigned char* lut256,
                         hipStream_t stream) {
    if (!in || !out || !lut256) return U2PL_EINVAL;
    if (n <= 0) return 0;
    long head = (long)((16 - ((uintptr_t)in & 15)) & 15);
    if (head > n) head = n;
    const long body = (n - head) >> 4;
    U2PL_LAUNCH(k_lut_u8, dim3(grid_for(body, 256, 1024)), dim3(256), 0, stream, lut256, in, out, n, head, body);
    U2PL_LAUNCH_CHECK();
    return 0;
}
