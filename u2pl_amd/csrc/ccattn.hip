// Criss-cross attention (CCNet, Huang et al., ICCV 2019, section 3): every pixel p = (y, x) of an image attends to its cross
//   X(p) = {(y, j) : 0 <= j < W} u {(i, x) : 0 <= i < H},  L = H + W - 1 members, p itself once.
//   forward    w[p, m] = softmax over m in X(p) of scale * q[p] . k[m],   out[p] = res[p] + gamma * sum_m w[p, m] v[m]
//   backward   t = g[p] . v[m], s[p] = sum_m w t, e = scale gamma w (t - s);  dq[p] = sum_m e[p, m] k[m];
//              dk[m] = sum_{p in X(m)} e[p, m] q[p];  dv[m] = gamma sum_{p in X(m)} w[p, m] g[p];  dgamma = sum_{n, p} s[p].
// Maps are NHWC rows with pitches; w is [N*H*W][L] with any pitch >= L.
//
// SLOT LAYOUT of w (part of the interface): for the pixel (y, x), slot j < W is the row member (y, j) -- the pixel itself is slot
// x -- and slot W + i - (i > y) is the column member (i, x), i != y, ascending.
//
// KERNEL SHAPE.  A cross is a row line and a column line, and all pixels of a line share the line's k and v rows.  Two kernels walk
// lines, each once for the rows of an image and once for its columns:
//   k_cc_dots   a wave takes CC_PT consecutive pixels of a line and 64 of its members (lane l <-> member 64 c + l): each lane walks
//               its member's row once for the CC_PT pixels, whose rows are wave-uniform.  Writes the raw dots into the slots.
//   k_cc_mix    a wave takes CC_PT consecutive pixels of a line and 256 channels (lane l <-> float4 l): it walks the line's
//               members once, one float4 load per member for CC_PT pixels, the weights are wave-uniform.  The row pass starts from
//               0.0f and writes the row part to the output; the column pass starts from what the row pass wrote and finishes.
//               The transposed form (dk, dv) takes the weight the SOURCE gives to the target: w[source][slot of the target].
// and two per-pixel kernels (one wave per pixel, lane l of register r <-> slot 64 r + l) take the softmax and the backward's e.
// So every operand row is re-read len / CC_PT times per line it lies on (once per group of CC_PT pixels), not L times.
//
// ARITHMETIC CONTRACT (part of the interface; tests/cc_bounds.py emulates this order)
//   everything is fp32 on the vector ALU; fma(a, b, c) is ONE rounding of a * b + c (__fmaf_rn); what is written apart is rounded
//   apart (-ffp-contract=off).  No atomics, no memset; every workspace word that is read was written by the same call before.
//   The order depends on the shapes alone.
//   dot(a, b)     ONE fma chain over the channels ascending from 0.0f: fma(a[c], b[c], acc).
//   wave sum      64 lane values added pairwise in six rounds (wave_sum_sgpr of common.h).
//   softmax       u = scale * dot; mx = max over the slots (exact); e = expf(u - mx); Z = wave sum of the lane sums
//                 ((e[l] + e[l + 64]) + e[l + 128]) + ... (absent slots add 0.0f); w = e / Z (one IEEE division).
//   mix           acc = fma(weight, row[c], acc) from 0.0f over the row slots ascending, then the column slots ascending (the
//                 transposed form: the sources (y, 0 .. W - 1), then (i, x), i != y, ascending).  Finish: out = fma(gamma, acc,
//                 res) (forward with res), gamma * acc (forward without res, dv), acc (dq, dk).
//   backward      t = dot(g[p], v[m]); s[p] = wave sum of the lane chains t0 w0, fma(w1, t1, .), ...;
//                 e = ((scale * gamma) * w) * (t - s).
//   dgamma        thread j of CC_SUM_THREADS adds s[j], s[j + CC_SUM_THREADS], ... to 0.0f; thread u < 32 adds the sums 32 u ..
//                 32 u + 31 ascending to the first of them; thread 0 adds the 32 group sums ascending to the first.
#include "common.h"
#include "u2pl_hip.h"

#define CC_MAX_L 512           // slots of one cross: H + W - 1 <= CC_MAX_L
#define CC_LCHUNK 64           // slots per lane register of the per-pixel kernels
#define CC_LREGS 8             // CC_MAX_L = CC_LCHUNK * CC_LREGS
#define CC_PT 8                // consecutive pixels of a line taken by one wave of k_cc_dots / k_cc_mix
#define CC_PASS 256            // channels of one k_cc_mix work item: 64 lanes x float4
#define CC_MAX_BLOCKS 1024     // grid cap of every kernel of this file but k_cc_sum (grid-stride over work items, 4 waves a block)
#define CC_SUM_THREADS 1024    // k_cc_sum: one block

__device__ __forceinline__ float4 c4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 c4ld(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 c4fma(float s, float4 b, float4 c) {
    return make_float4(__fmaf_rn(s, b.x, c.x), __fmaf_rn(s, b.y, c.y), __fmaf_rn(s, b.z, c.z), __fmaf_rn(s, b.w, c.w));
}

// wave wv_ of the launch takes the work items wv_, wv_ + waves, ...
#define CC_WAVE_LOOP(items)                                                                                                       \
    const int lane = threadIdx.x & 63;                                                                                            \
    for (long it = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); it < (items); it += (long)gridDim.x * 4)

// ---- lines ------------------------------------------------------------------------------------------------------------------------
// COL = false: line ln is the image row ln (members (ln, s), s < W);  COL = true: the image column ln (members (s, ln), s < H)
// T[pixel t of the line][slot of member s] = dot(a[pixel t], b[member s]) over Dl channels; the column pass skips s == t
template <bool COL>
__global__ void __launch_bounds__(256) k_cc_dots(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb, int N,
                                                 int H, int W, int Dl, float* __restrict__ T, long ldt) {
    const int len = COL ? H : W, lines = COL ? W : H, G = (len + CC_PT - 1) / CC_PT, MCH = (len + CC_LCHUNK - 1) / CC_LCHUNK;
    const long stride = COL ? W : 1;
    const int D4 = Dl >> 2;
    CC_WAVE_LOOP((long)N * lines * G * MCH) {
        const int mc = (int)(it % MCH);
        long r = it / MCH;
        const int g = (int)(r % G);
        r /= G;
        const int ln = (int)(r % lines), n = (int)(r / lines);
        const int t0 = g * CC_PT, nt = min(CC_PT, len - t0);
        const long base = (long)n * H * W + (COL ? (long)ln : (long)ln * W);
        const int s = mc * CC_LCHUNK + lane;
        const bool sok = s < len;
        const float* brow = b + (base + (long)(sok ? s : len - 1) * stride) * ldb;    // lanes past the line read its last member
        const float* arow = a + (base + (long)t0 * stride) * lda;
        float acc[CC_PT];
#pragma unroll
        for (int i = 0; i < CC_PT; ++i) acc[i] = 0.f;
        for (int d4 = 0; d4 < D4; ++d4) {
            const float4 bv = c4ld(brow + d4 * 4);
#pragma unroll
            for (int i = 0; i < CC_PT; ++i) {
                if (i < nt) {
                    const float4 av = c4ld(arow + (long)i * stride * lda + d4 * 4);
                    acc[i] = __fmaf_rn(av.w, bv.w, __fmaf_rn(av.z, bv.z, __fmaf_rn(av.y, bv.y, __fmaf_rn(av.x, bv.x, acc[i]))));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CC_PT; ++i) {
            const int t = t0 + i;
            if (i < nt && sok && !(COL && s == t)) T[(base + (long)t * stride) * ldt + (COL ? W + s - (s > t ? 1 : 0) : s)] = acc[i];
        }
    }
}

// out[target t of the line][c] (+)= sum over the line's sources s of weight(t, s) x[s][c].
//   TR = false: weight = A[t][slot of s in t's cross];  TR = true: weight = A[s][slot of t in s's cross].
// The row pass (COL = false) starts from 0.0f and stores the sum; the column pass starts from the stored value, skips s == t and
// finishes: finish 0: acc;  1: gamma * acc;  2: fma(gamma, acc, res).
template <bool COL, bool TR>
__global__ void __launch_bounds__(256) k_cc_mix(const float* __restrict__ A, long lda, const float* __restrict__ x, long ldx,
                                                const float* __restrict__ res, long ldr, const float* __restrict__ gm, int finish, int N,
                                                int H, int W, int C, float* out, long ldo) {
    const int len = COL ? H : W, lines = COL ? W : H, G = (len + CC_PT - 1) / CC_PT;
    const long stride = COL ? W : 1;
    const int C4 = C >> 2, CCH = (C4 + 63) / 64;
    CC_WAVE_LOOP((long)N * lines * G * CCH) {
        const int cc = (int)(it % CCH);
        long r = it / CCH;
        const int g = (int)(r % G);
        r /= G;
        const int ln = (int)(r % lines), n = (int)(r / lines);
        const int t0 = g * CC_PT, nt = min(CC_PT, len - t0);
        const long base = (long)n * H * W + (COL ? (long)ln : (long)ln * W);
        const int c4 = cc * 64 + lane;
        const bool cok = c4 < C4;
        const long co = (long)(cok ? c4 : C4 - 1) * 4;        // lanes past the row read its last float4 (in bounds), store nothing
        float4 acc[CC_PT];
#pragma unroll
        for (int i = 0; i < CC_PT; ++i) acc[i] = (COL && i < nt) ? c4ld(out + (base + (long)(t0 + i) * stride) * ldo + co) : c4zero();
        for (int s = 0; s < len; ++s) {
            const long srow = base + (long)s * stride;
            const float4 xv = c4ld(x + srow * ldx + co);
#pragma unroll
            for (int i = 0; i < CC_PT; ++i) {
                const int t = t0 + i;
                if (i < nt && !(COL && s == t)) {
                    const long trow = base + (long)t * stride;
                    const float wt = TR ? A[srow * lda + (COL ? W + t - (t > s ? 1 : 0) : t)]
                                        : A[trow * lda + (COL ? W + s - (s > t ? 1 : 0) : s)];
                    acc[i] = c4fma(wt, xv, acc[i]);
                }
            }
        }
        if (cok) {
            const float gv = (COL && finish) ? gm[0] : 0.f;
#pragma unroll
            for (int i = 0; i < CC_PT; ++i) {
                if (i < nt) {
                    const long trow = base + (long)(t0 + i) * stride;
                    float4 o = acc[i];
                    if (COL && finish == 1) o = make_float4(__fmul_rn(gv, o.x), __fmul_rn(gv, o.y), __fmul_rn(gv, o.z), __fmul_rn(gv, o.w));
                    if (COL && finish == 2) o = c4fma(gv, o, c4ld(res + trow * ldr + co));
                    *(float4*)(out + trow * ldo + co) = o;
                }
            }
        }
    }
}

// ---- pixels: one wave per pixel, lane l of register r <-> slot 64 r + l -----------------------------------------------------------
// w holds the raw dots on entry and the weights on return
__global__ void __launch_bounds__(256) k_cc_softmax(float* __restrict__ w, long ldw, float scale, long NP, int L) {
    CC_WAVE_LOOP(NP) {
        float d[CC_LREGS], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < CC_LREGS; ++r) {
            const int sl = r * CC_LCHUNK + lane;
            d[r] = sl < L ? __fmul_rn(scale, w[it * ldw + sl]) : -INFINITY;
            mx = fmaxf(mx, d[r]);
        }
        mx = wave_max(mx);
        float z = 0.f;
#pragma unroll
        for (int r = 0; r < CC_LREGS; ++r) {
            d[r] = r * CC_LCHUNK + lane < L ? expf(__fsub_rn(d[r], mx)) : 0.f;
            z = r == 0 ? d[r] : z + d[r];
        }
        z = wave_sum_sgpr(z);
#pragma unroll
        for (int r = 0; r < CC_LREGS; ++r) {
            const int sl = r * CC_LCHUNK + lane;
            if (sl < L) w[it * ldw + sl] = __fdiv_rn(d[r], z);
        }
    }
}

// T [NP][L] dense holds t on entry and e on return; S[p] = s[p]
__global__ void __launch_bounds__(256) k_cc_bwd_e(const float* __restrict__ w, long ldw, const float* __restrict__ gm, float scale, long NP,
                                                  int L, float* __restrict__ T, float* __restrict__ S) {
    const float sg = __fmul_rn(scale, gm[0]);
    CC_WAVE_LOOP(NP) {
        float tr[CC_LREGS], wr[CC_LREGS], sd = 0.f;
#pragma unroll
        for (int r = 0; r < CC_LREGS; ++r) {
            const int sl = r * CC_LCHUNK + lane;
            tr[r] = sl < L ? T[it * L + sl] : 0.f;
            wr[r] = sl < L ? w[it * ldw + sl] : 0.f;
            sd = r == 0 ? __fmul_rn(wr[r], tr[r]) : __fmaf_rn(wr[r], tr[r], sd);
        }
        sd = wave_sum_sgpr(sd);
#pragma unroll
        for (int r = 0; r < CC_LREGS; ++r) {
            const int sl = r * CC_LCHUNK + lane;
            if (sl < L) T[it * L + sl] = __fmul_rn(__fmul_rn(sg, wr[r]), __fsub_rn(tr[r], sd));
        }
        if (lane == 0) S[it] = sd;
    }
}

// dgamma = sum of S[0 .. NP - 1]: one block
__global__ void __launch_bounds__(CC_SUM_THREADS) k_cc_sum(const float* __restrict__ S, long NP, float* __restrict__ out) {
    __shared__ float s_a[CC_SUM_THREADS];
    __shared__ float s_b[32];
    const int t = threadIdx.x;
    float acc = 0.f;
#pragma unroll 4
    for (long p = t; p < NP; p += CC_SUM_THREADS) acc += S[p];
    s_a[t] = acc;
    __syncthreads();
    if (t < 32) {
        acc = s_a[t * 32];
        for (int j = 1; j < 32; ++j) acc += s_a[t * 32 + j];
        s_b[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        acc = s_b[0];
        for (int j = 1; j < 32; ++j) acc += s_b[j];
        out[0] = acc;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool cc_shape_ok(int N, int H, int W, int D, int C) {
    if (N < 1 || H < 1 || W < 1 || D < 4 || C < 4 || D % 4 || C % 4) return false;
    if ((long)H + W - 1 > CC_MAX_L) return false;
    return (long)N * H * W < (1L << 31);
}
static bool cc_rows_ok(const void* p, long ld, int width) {        // a channel-wide tensor: float4 rows
    return p != nullptr && ld >= width && ld % 4 == 0 && ((uintptr_t)p & 15) == 0;
}
static inline long cc_up4(long n) { return (n + 3) & ~3L; }
static inline unsigned cc_grid(long waves) {
    const long blocks = (waves + 3) / 4;
    return (unsigned)(blocks < CC_MAX_BLOCKS ? (blocks < 1 ? 1 : blocks) : CC_MAX_BLOCKS);
}
static inline long cc_groups(int len) { return (len + CC_PT - 1) / CC_PT; }

// T[p][slot] = a[p] . b[member] for every slot of every cross
static int cc_dots(const float* a, long lda, const float* b, long ldb, int N, int H, int W, int Dl, float* T, long ldt,
                   hipStream_t stream) {
    U2PL_LAUNCH(k_cc_dots<false>, dim3(cc_grid((long)N * H * cc_groups(W) * ((W + CC_LCHUNK - 1) / CC_LCHUNK))), dim3(256), 0, stream, a,
                lda, b, ldb, N, H, W, Dl, T, ldt);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_cc_dots<true>, dim3(cc_grid((long)N * W * cc_groups(H) * ((H + CC_LCHUNK - 1) / CC_LCHUNK))), dim3(256), 0, stream, a,
                lda, b, ldb, N, H, W, Dl, T, ldt);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// the row pass, then the column pass with the finish
template <bool TR>
static int cc_mix(const float* A, long lda, const float* x, long ldx, const float* res, long ldr, const float* gm, int finish, int N,
                  int H, int W, int C, float* out, long ldo, hipStream_t stream) {
    const long cch = (C / 4 + 63) / 64;
    U2PL_LAUNCH((k_cc_mix<false, TR>), dim3(cc_grid((long)N * H * cc_groups(W) * cch)), dim3(256), 0, stream, A, lda, x, ldx, res, ldr, gm,
                finish, N, H, W, C, out, ldo);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH((k_cc_mix<true, TR>), dim3(cc_grid((long)N * W * cc_groups(H) * cch)), dim3(256), 0, stream, A, lda, x, ldx, res, ldr, gm,
                finish, N, H, W, C, out, ldo);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API size_t u2pl_cc_attn_bwd_ws_floats(int N, int H, int W, int D, int C) {
    if (!cc_shape_ok(N, H, W, D, C)) return 0;
    const long NP = (long)N * H * W;
    return (size_t)cc_up4(NP * (H + W - 1)) + (size_t)cc_up4(NP);
}

U2PL_API int u2pl_cc_attn_fwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, const float* res,
                                  long ldr, const float* gamma, float scale, int N, int H, int W, int D, int C, float* w, long ldw,
                                  float* out, long ldo, hipStream_t stream) {
    if (!cc_shape_ok(N, H, W, D, C) || !cc_rows_ok(q, ldq, D) || !cc_rows_ok(k, ldk, D) || !cc_rows_ok(v, ldv, C) || gamma == nullptr ||
        w == nullptr || ldw < (long)H + W - 1 || !cc_rows_ok(out, ldo, C))
        return U2PL_EINVAL;
    if (res != nullptr && !cc_rows_ok(res, ldr, C)) return U2PL_EINVAL;
    const long NP = (long)N * H * W;
    int rc = cc_dots(q, ldq, k, ldk, N, H, W, D, w, ldw, stream);
    if (rc) return rc;
    U2PL_LAUNCH(k_cc_softmax, dim3(cc_grid(NP)), dim3(256), 0, stream, w, ldw, scale, NP, H + W - 1);
    U2PL_LAUNCH_CHECK();
    return cc_mix<false>(w, ldw, v, ldv, res, ldr, gamma, res != nullptr ? 2 : 1, N, H, W, C, out, ldo, stream);
}

U2PL_API int u2pl_cc_attn_bwd_f32(const float* g, long ldg, const float* w, long ldw, const float* q, long ldq, const float* k, long ldk,
                                  const float* v, long ldv, const float* gamma, float scale, int N, int H, int W, int D, int C,
                                  float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, float* dgamma, float* ws,
                                  hipStream_t stream) {
    if (!cc_shape_ok(N, H, W, D, C) || !cc_rows_ok(g, ldg, C) || w == nullptr || ldw < (long)H + W - 1 || gamma == nullptr ||
        (!dq && !dk && !dv && !dgamma) || !cc_rows_ok(ws, 4, 4))
        return U2PL_EINVAL;
    if (dq && (!cc_rows_ok(dq, lddq, D) || !cc_rows_ok(k, ldk, D))) return U2PL_EINVAL;
    if (dk && (!cc_rows_ok(dk, lddk, D) || !cc_rows_ok(q, ldq, D))) return U2PL_EINVAL;
    if (dv && !cc_rows_ok(dv, lddv, C)) return U2PL_EINVAL;
    if ((dq || dk || dgamma) && !cc_rows_ok(v, ldv, C)) return U2PL_EINVAL;
    const long NP = (long)N * H * W;
    const int L = H + W - 1;
    float *T = ws, *S = ws + cc_up4(NP * L);
    int rc = 0;
    if (dq || dk || dgamma) {
        rc = cc_dots(g, ldg, v, ldv, N, H, W, C, T, L, stream);
        if (rc) return rc;
        U2PL_LAUNCH(k_cc_bwd_e, dim3(cc_grid(NP)), dim3(256), 0, stream, w, ldw, gamma, scale, NP, L, T, S);
        U2PL_LAUNCH_CHECK();
    }
    if (dgamma) {
        U2PL_LAUNCH(k_cc_sum, dim3(1), dim3(CC_SUM_THREADS), 0, stream, S, NP, dgamma);
        U2PL_LAUNCH_CHECK();
    }
    if (dq) rc = cc_mix<false>(T, L, k, ldk, nullptr, 0, gamma, 0, N, H, W, D, dq, lddq, stream);
    if (rc) return rc;
    if (dk) rc = cc_mix<true>(T, L, q, ldq, nullptr, 0, gamma, 0, N, H, W, D, dk, lddk, stream);
    if (rc) return rc;
    if (dv) rc = cc_mix<true>(w, ldw, g, ldg, nullptr, 0, gamma, 1, N, H, W, C, dv, lddv, stream);
    return rc;
}
