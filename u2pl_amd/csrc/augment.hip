// Training-time data pipeline on the device, full option surface (reference u2pl/dataset/augmentation.py:51-346
// as composed by pascal_voc.py:48-71): ToTensor -> Normalize -> RandResize -> RandRotate -> RandomGaussianBlur ->
// RandomHorizontalFlip -> Crop, for batches whose samples may all differ in size.  k_augment (nn.hip) stays the kernel of
// equal-sized, option-free batches; the resize sample below repeats its arithmetic operation for operation, so a dense
// option-free batch gives the same bits through either entry point.
//
// Per sample a record of U2PL_AUG_REC int32 (include/u2pl_hip.h):
//   {rh, rw, flip, pad_top, pad_left, crop_y, crop_x, flags, H, W, m00, m01, m10, m11 (float32 bit patterns), 0, 0}
// Composed backwards from the output pixel: crop / zero padding -> un-flip -> [5x5 blur over the rotated frame, zeros
// outside it] -> [rotate: 4 bilinear taps of the resized frame, zeros outside; label nearest (half to even), outside ->
// ignore_label] -> resize sample of the uint8 source.
//
//   no blur in the config:  ONE pass (k_augment_ex), 16 source taps per rotated pixel.
//   blur in the config:     pass A (k_augment_stage) writes the normalised / resized / rotated image of the crop window
//                           (mirrored when flipped) plus a 2-pixel halo into the caller's scratch, [B][3][Sh+4][Sw+4]
//                           fp32, zeros where the window leaves the frame;  pass B (k_augment_blur) reads 25 taps of it
//                           per output pixel (x fastest per lane in both passes, so scratch traffic is coalesced) and
//                           writes the label.  A sample whose blur coin fell the other way reads the centre tap only.
//
// Label table (u2pl_augment_lut_u8_f32, dataset.label_map): the kernels that write labels carry a template switch LUT; with
// it the ONE read of a source label byte (resize_lab) goes through a 256-entry uint8 table in device memory.  The index
// is a byte, so the lookup cannot leave the table; padding (0) and rotated-out pixels (ignore_label) are written in
// mapped space and are not looked up.  The table is read through the vector cache, not staged in LDS: it
// is two 128-byte lines that every wave of the launch keeps hot, the lookup follows a gather of the same kind (the label
// byte), and without the switch the kernels are the code they were -- no LDS, no barrier.
#include "common.h"
#include "u2pl_hip.h"

namespace {

struct AugNorm {
    float m[3], s[3];
};

struct AugSrc {                      // one sample of the batch
    const unsigned char* ib;         // [H][W][3]
    const unsigned char* lb;         // [H][W]
    int H, W, rh, rw, flip, pt, pl, ho, wo, flags;
    float m00, m01, m10, m11;
};

__device__ __forceinline__ AugSrc aug_src(const unsigned char* img, const unsigned char* lab, const long long* off,
                                          const int* rec, int b, int H, int W) {
    const int* p = rec + b * U2PL_AUG_REC;
    AugSrc s;
    s.rh = p[0]; s.rw = p[1]; s.flip = p[2]; s.pt = p[3]; s.pl = p[4]; s.ho = p[5]; s.wo = p[6]; s.flags = p[7];
    s.H = off ? p[8] : H;
    s.W = off ? p[9] : W;
    const long o = off ? (long)off[b] : (long)b * H * W;      // in pixels
    s.ib = img + o * 3;
    s.lb = lab + o;
    s.m00 = __int_as_float(p[10]); s.m01 = __int_as_float(p[11]);
    s.m10 = __int_as_float(p[12]); s.m11 = __int_as_float(p[13]);
    return s;
}

// label of pixel (ry, rx) of the resized frame: legacy nearest, src = min(floor(dst * float(in/out)), in-1)
// LUT: the byte indexes the 256-entry table of dataset.label_map -- the only place a source label is read
template <bool LUT>
__device__ __forceinline__ int resize_lab(const AugSrc& s, const unsigned char* __restrict__ lut, int ry, int rx) {
    const int ly = nearest_src(ry, (float)s.H / (float)s.rh, s.H), lx = nearest_src(rx, (float)s.W / (float)s.rw, s.W);
    const unsigned char raw = s.lb[(long)ly * s.W + lx];
    return LUT ? lut[raw] : raw;
}

// normalised pixel (ry, rx) of the resized frame, 0 <= ry < rh, 0 <= rx < rw: the arithmetic of k_augment (nn.hip)
__device__ __forceinline__ void resize_px(const AugSrc& s, const AugNorm& n, int ry, int rx, float v[3]) {
    const int H = s.H, W = s.W;
    if (s.rh == H && s.rw == W) {     // interpolate() with an unchanged size is the identity in torch too
        const unsigned char* q = s.ib + ((long)ry * W + rx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(__fsub_rn((float)q[c], n.m[c]), n.s[c]);
        return;
    }
    // bilinear, align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0, one rounding (fma) like the ATen kernel
    const float sy = (float)H / (float)s.rh, sx = (float)W / (float)s.rw;
    float fy = __fmaf_rn(sy, (float)ry + 0.5f, -0.5f), fx = __fmaf_rn(sx, (float)rx + 0.5f, -0.5f);
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < H - 1 ? y0 : H - 1;     // no-ops for a well-formed record; a malformed one must not read out of bounds
    x0 = x0 < W - 1 ? x0 : W - 1;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = __fsub_rn(fy, (float)y0), lx1 = __fsub_rn(fx, (float)x0);
    const float ly0 = __fsub_rn(1.f, ly1), lx0 = __fsub_rn(1.f, lx1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a00 = __fdiv_rn(__fsub_rn((float)s.ib[((long)y0 * W + x0) * 3 + c], n.m[c]), n.s[c]);
        const float a01 = __fdiv_rn(__fsub_rn((float)s.ib[((long)y0 * W + x1) * 3 + c], n.m[c]), n.s[c]);
        const float a10 = __fdiv_rn(__fsub_rn((float)s.ib[((long)y1 * W + x0) * 3 + c], n.m[c]), n.s[c]);
        const float a11 = __fdiv_rn(__fsub_rn((float)s.ib[((long)y1 * W + x1) * 3 + c], n.m[c]), n.s[c]);
        const float top = __fadd_rn(__fmul_rn(lx0, a00), __fmul_rn(lx1, a01));
        const float bot = __fadd_rn(__fmul_rn(lx0, a10), __fmul_rn(lx1, a11));
        v[c] = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
    }
}

// F.affine_grid + F.grid_sample(align_corners=False) source coordinate of pixel (ry, rx) of the rotated frame, in pixels
// of the resized frame.  torch evaluates this in float32 (error ~ 2^-24 * max(rh, rw) pixels); float64 here costs two
// divisions per pixel and leaves the bilinear weights as the only float32 rounding of the rotation.
__device__ __forceinline__ void rot_coord(const AugSrc& s, int ry, int rx, double& iy, double& ix) {
    const double xn = (2.0 * rx + 1.0) / (double)s.rw - 1.0, yn = (2.0 * ry + 1.0) / (double)s.rh - 1.0;
    ix = (((double)s.m00 * xn + (double)s.m01 * yn + 1.0) * (double)s.rw - 1.0) * 0.5;
    iy = (((double)s.m10 * xn + (double)s.m11 * yn + 1.0) * (double)s.rh - 1.0) * 0.5;
}

// pixel (ry, rx) of the rotated frame: grid_sample(bilinear, zeros) over the resized frame
__device__ __forceinline__ void rot_px(const AugSrc& s, const AugNorm& n, int ry, int rx, float v[3]) {
    double iy, ix;
    rot_coord(s, ry, rx, iy, ix);
    const double fy = floor(iy), fx = floor(ix);
    const float wy1 = (float)(iy - fy), wx1 = (float)(ix - fx);
    const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    // floor() of a coordinate far outside int range (a malformed matrix) must still fail the frame test below
    const int y0 = (int)fmax(fmin(fy, 1e9), -1e9), x0 = (int)fmax(fmin(fx, 1e9), -1e9);
    v[0] = v[1] = v[2] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yy = y0 + (t >> 1), xx = x0 + (t & 1);
        if (yy < 0 || yy >= s.rh || xx < 0 || xx >= s.rw) continue;
        const float w = ((t >> 1) ? wy1 : wy0) * ((t & 1) ? wx1 : wx0);
        float a[3];
        resize_px(s, n, yy, xx, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fmaf_rn(w, a[c], v[c]);
    }
}

// label of pixel (ry, rx) of the rotated frame: grid_sample(nearest) = nearbyint, outside the frame -> ignore_label
template <bool LUT>
__device__ __forceinline__ int rot_lab(const AugSrc& s, const unsigned char* __restrict__ lut, int ry, int rx,
                                       int ignore_label) {
    double iy, ix;
    rot_coord(s, ry, rx, iy, ix);
    const double ny = rint(iy), nx = rint(ix);
    if (!(ny >= 0.0 && ny < (double)s.rh && nx >= 0.0 && nx < (double)s.rw)) return ignore_label;
    return resize_lab<LUT>(s, lut, (int)ny, (int)nx);
}

// ---- no blur: one pass -------------------------------------------------------------------------------------------
template <bool ROT, bool LUT>
__global__ void k_augment_ex(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lab,
                             const long long* __restrict__ off, const int* __restrict__ rec, int B, int H, int W, int Sh,
                             int Sw, int ignore_label, const unsigned char* __restrict__ lut, AugNorm n,
                             float* __restrict__ out_img, long long* __restrict__ out_lab) {
    const long total = (long)B * Sh * Sw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Sw);
        const long t = i / Sw;
        const int y = (int)(t % Sh), b = (int)(t / Sh);
        const AugSrc s = aug_src(img, lab, off, rec, b, H, W);
        const int ry = s.ho + y - s.pt;
        int rx = s.wo + x - s.pl;
        float v[3] = {0.f, 0.f, 0.f};
        long long l = 0;
        if (ry >= 0 && ry < s.rh && rx >= 0 && rx < s.rw) {
            if (s.flip) rx = s.rw - 1 - rx;
            if (ROT && (s.flags & U2PL_AUG_ROTATE)) {
                rot_px(s, n, ry, rx, v);
                l = rot_lab<LUT>(s, lut, ry, rx, ignore_label);
            } else {
                resize_px(s, n, ry, rx, v);
                l = resize_lab<LUT>(s, lut, ry, rx);
            }
        }
        const long plane = (long)Sh * Sw, o = (long)b * 3 * plane + (long)y * Sw + x;
        out_img[o] = v[0];
        out_img[o + plane] = v[1];
        out_img[o + 2 * plane] = v[2];
        out_lab[i] = l;
    }
}

// ---- blur, pass A: the crop window of the rotated frame + halo -> scratch [B][3][Sh+4][Sw+4] ---------------------------
// tile (ty, tx) is pixel (ho - pt - 2 + ty, x_lo - 2 + tx) of the un-flipped rotated frame, x_lo the window's left edge
__device__ __forceinline__ int window_left(const AugSrc& s, int Sw) {
    return s.flip ? s.rw - (s.wo - s.pl) - Sw : s.wo - s.pl;
}
__global__ void k_augment_stage(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lab,
                                const long long* __restrict__ off, const int* __restrict__ rec, int B, int H, int W,
                                int Sh, int Sw, AugNorm n, float* __restrict__ scratch) {
    const int Th = Sh + 4, Tw = Sw + 4;
    const long total = (long)B * Th * Tw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int tx = (int)(i % Tw);
        const long t = i / Tw;
        const int ty = (int)(t % Th), b = (int)(t / Th);
        const AugSrc s = aug_src(img, lab, off, rec, b, H, W);
        const int ry = s.ho - s.pt - 2 + ty, rx = window_left(s, Sw) - 2 + tx;
        float v[3] = {0.f, 0.f, 0.f};
        if (ry >= 0 && ry < s.rh && rx >= 0 && rx < s.rw) {
            if (s.flags & U2PL_AUG_ROTATE) rot_px(s, n, ry, rx, v);
            else resize_px(s, n, ry, rx, v);
        }
        const long plane = (long)Th * Tw, o = (long)b * 3 * plane + (long)ty * Tw + tx;
        scratch[o] = v[0];
        scratch[o + plane] = v[1];
        scratch[o + 2 * plane] = v[2];
    }
}

// ---- blur, pass B: 25 taps of the scratch tile (F.conv2d, zero padding 2, over the rotated frame) + flip + crop + label --
template <bool LUT>
__global__ void k_augment_blur(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lab,
                               const long long* __restrict__ off, const int* __restrict__ rec, int B, int H, int W,
                               int Sh, int Sw, int ignore_label, const unsigned char* __restrict__ lut,
                               const float* __restrict__ blur_w,
                               const float* __restrict__ scratch, float* __restrict__ out_img,
                               long long* __restrict__ out_lab) {
    __shared__ float w[25];
    if (threadIdx.x < 25) w[threadIdx.x] = blur_w[threadIdx.x];
    __syncthreads();
    const int Th = Sh + 4, Tw = Sw + 4;
    const long total = (long)B * Sh * Sw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Sw);
        const long t = i / Sw;
        const int y = (int)(t % Sh), b = (int)(t / Sh);
        const AugSrc s = aug_src(img, lab, off, rec, b, H, W);
        const int ry = s.ho + y - s.pt;
        int rx = s.wo + x - s.pl;
        float v[3] = {0.f, 0.f, 0.f};
        long long l = 0;
        if (ry >= 0 && ry < s.rh && rx >= 0 && rx < s.rw) {
            if (s.flip) rx = s.rw - 1 - rx;
            l = (s.flags & U2PL_AUG_ROTATE) ? rot_lab<LUT>(s, lut, ry, rx, ignore_label) : resize_lab<LUT>(s, lut, ry, rx);
            // centre tap: tile row y + 2, tile column x + 2 (mirrored: Sw + 1 - x); every tap stays inside the tile
            const float* c0 = scratch + (long)b * 3 * Th * Tw + (long)(y + 2) * Tw + (s.flip ? Sw + 1 - x : x + 2);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* q = c0 + (long)c * Th * Tw;
                if (s.flags & U2PL_AUG_BLUR) {
                    float a = 0.f;
#pragma unroll
                    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                        for (int dx = -2; dx <= 2; ++dx) a = __fmaf_rn(w[(dy + 2) * 5 + dx + 2], q[dy * Tw + dx], a);
                    v[c] = a;
                } else {
                    v[c] = q[0];
                }
            }
        }
        const long plane = (long)Sh * Sw, o = (long)b * 3 * plane + (long)y * Sw + x;
        out_img[o] = v[0];
        out_img[o + plane] = v[1];
        out_img[o + 2 * plane] = v[2];
        out_lab[i] = l;
    }
}

}  // namespace

U2PL_API size_t u2pl_augment_ex_scratch_bytes(int B, int Sh, int Sw, int mode) {
    if (!(mode & U2PL_AUG_BLUR) || B <= 0 || Sh <= 0 || Sw <= 0) return 0;
    return (size_t)B * 3 * (size_t)(Sh + 4) * (size_t)(Sw + 4) * sizeof(float);
}

// both entry points: LUT selects the instantiations that map the source label through lut256
template <bool LUT>
static int augment_launch(const unsigned char* img, const unsigned char* lab, const long long* offsets, const int* records,
                          int B, int H, int W, int Sh, int Sw, int ignore_label, int mode, const unsigned char* lut256,
                          const float* mean3, const float* std3, const float* blur_w, float* scratch, float* out_img,
                          long long* out_lab, hipStream_t stream) {
    const long total = (long)B * Sh * Sw;
    if (total <= 0) return 0;
    if (!img || !lab || !records || !mean3 || !std3 || !out_img || !out_lab) return U2PL_EINVAL;
    if (!offsets && (H <= 0 || W <= 0)) return U2PL_EINVAL;
    if ((mode & U2PL_AUG_BLUR) && (!blur_w || !scratch)) return U2PL_EINVAL;
    // mean / std are HOST pointers (three floats each): they travel as kernel arguments
    const AugNorm n = {{mean3[0], mean3[1], mean3[2]}, {std3[0], std3[1], std3[2]}};
    if (mode & U2PL_AUG_BLUR) {
        U2PL_LAUNCH(k_augment_stage, dim3(grid_for((long)B * (Sh + 4) * (Sw + 4), 256)), dim3(256), 0, stream, img, lab,
                    offsets, records, B, H, W, Sh, Sw, n, scratch);
        U2PL_LAUNCH_CHECK();
        U2PL_LAUNCH(k_augment_blur<LUT>, dim3(grid_for(total, 256)), dim3(256), 0, stream, img, lab, offsets, records, B, H,
                    W, Sh, Sw, ignore_label, lut256, blur_w, (const float*)scratch, out_img, out_lab);
    } else if (mode & U2PL_AUG_ROTATE) {
        U2PL_LAUNCH((k_augment_ex<true, LUT>), dim3(grid_for(total, 256)), dim3(256), 0, stream, img, lab, offsets, records,
                    B, H, W, Sh, Sw, ignore_label, lut256, n, out_img, out_lab);
    } else {
        U2PL_LAUNCH((k_augment_ex<false, LUT>), dim3(grid_for(total, 256)), dim3(256), 0, stream, img, lab, offsets, records,
                    B, H, W, Sh, Sw, ignore_label, lut256, n, out_img, out_lab);
    }
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API int u2pl_augment_ex_u8_f32(const unsigned char* img, const unsigned char* lab, const long long* offsets,
                                    const int* records, int B, int H, int W, int Sh, int Sw, int ignore_label, int mode,
                                    const float* mean3, const float* std3, const float* blur_w, float* scratch,
                                    float* out_img, long long* out_lab, hipStream_t stream) {
    return augment_launch<false>(img, lab, offsets, records, B, H, W, Sh, Sw, ignore_label, mode, nullptr, mean3, std3,
                                 blur_w, scratch, out_img, out_lab, stream);
}

U2PL_API int u2pl_augment_lut_u8_f32(const unsigned char* img, const unsigned char* lab, const long long* offsets,
                                     const int* records, int B, int H, int W, int Sh, int Sw, int ignore_label, int mode,
                                     const unsigned char* lut256, const float* mean3, const float* std3,
                                     const float* blur_w, float* scratch, float* out_img, long long* out_lab,
                                     hipStream_t stream) {
    if (!lut256) return U2PL_EINVAL;
    return augment_launch<true>(img, lab, offsets, records, B, H, W, Sh, Sw, ignore_label, mode, lut256, mean3, std3,
                                blur_w, scratch, out_img, out_lab, stream);
}
