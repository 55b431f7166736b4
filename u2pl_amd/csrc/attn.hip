// Dense (non-local) attention, several heads, Pq queries against Pk keys per image (Non-local networks, Wang et al., CVPR 2018;
// DANet's position attention, Fu et al., CVPR 2019; the attention of a transformer block with spatially reduced keys):
//   forward    S = scale q_h k_h^T ([Pq][Pk], never in memory);  P = softmax over the keys of S;  o_h = P v_h;
//              lse = max_j S + log sum_j exp(S - max)   (natural log)
//   backward   from g = d o and the saved o, lse: P = exp(S - lse) (recomputed), delta[p, h] = g[p, h, :] . o[p, h, :],
//              dP = g v^T, dS = P o (dP - delta);  dq = scale dS k;  dk = scale dS^T q;  dv = P^T g.
// Rows: q, dq [N*Pq][heads*D]; k, dk [N*Pk][heads*D]; v, dv [N*Pk][heads*Dv]; o, g [N*Pq][heads*Dv]; head h owns the columns
// h*D .. / h*Dv ..; lse dense [(n*heads + h)*Pq + p].  Nothing of size Pq x Pk is ever written: the weights of one 16 x 64 tile live
// in a wave's accumulator registers and are recomputed by the backward.
//
// KERNEL SHAPE.  All products run on v_mfma_f32_16x16x4_f32.  A wave OWNS 16 rows of one side (lane & 15 <-> owned row) and WALKS
// the other side in tiles of ATTN_BK = 64 rows; a block is 4 waves = ATTN_BQ = 64 owned rows.  The score tile is computed
// transposed, walked rows down the accumulator (row 16 t + 4 (lane >> 4) + r of sub-tile t, register r), the owned row on the lane,
// so the registers feed the next product's B operand with no lane movement and no LDS: k-slot (lane >> 4) of the step (t, r)
// is the walked row 16 t + 4 (lane >> 4) + r, and the other operand is loaded in that same permuted order.
//   k_attn_fwd    owns queries, walks keys ascending, online softmax; one pass holds ATTN_DVC = 128 value channels, a wider Dv
//                 is cut into chunks (work items of their own) that recompute S; chunk 0 writes lse.
//   k_attn_delta  one thread per (image, head, query).
//   k_attn_dq     owns queries, walks keys ascending.
//   k_attn_kgrad  <true>: dk, <false>: dv in chunks of ATTN_DVC channels; owns keys, walks the queries of one SLAB ascending.  With
//                 few key tiles the queries are cut into NS slabs (attn_slabs: a function of N, heads, Pq, Pk alone), the partial
//                 sums go to the workspace and k_attn_finish adds them in slab order (the pattern of k_gconv_wgrad_finish).
// Every kernel is a grid-stride loop over its work items under the cap ATTN_MAX_BLOCKS; an item is computed by one block, so
// the grid does not enter the arithmetic.  Operands come straight from global memory (L1 / L2); no LDS.
//
// ARITHMETIC CONTRACT (part of the interface; tests/attn_bounds.py emulates this order)
//   fp32 throughout; an MFMA is bit for bit a k-ordered fmaf chain into its accumulator; what is written apart is rounded apart
//   (-ffp-contract=off).  No atomics, no memset; every workspace word that is read was written by the same call before.  The
//   order depends on the shapes alone.
//   dots(a, b; Wd)   the chain of S (Wd = D) and of dP (Wd = Dv) from 0.0f: for c0 = 0, 16, .. : for x = 0 .. 3: for s = 0 .. 3:
//                    channel c0 + 4 s + x (channels >= Wd feed 0.0f, never the pitch gap).
//   mix              the chain of o, dq, dk, dv over the walked rows: walked tiles of 64 ascending; inside a tile t = 0 .. 3,
//                    r = 0 .. 3, s = 0 .. 3: row 16 t + 4 s + r.  Rows past the end feed weight 0.0f and operand 0.0f, never memory.
//   forward, per key tile: u = scale * S (one rounding); padding keys of the last tile are EXCLUDED (they do not enter the
//                    maximum, their weight is exactly 0.0f; they are not scored 0); mt = max over the tile (exact);
//                    m' = max(m, mt); alpha = expf(m - m') (m = -inf before the first tile: alpha = 0; every processed tile
//                    holds at least one real key, so m' is finite and -inf - (-inf) cannot arise); p = expf(u - m');
//                    every lane keeps the sum z over ITS keys: z = z * alpha, then z += p for t, r ascending;
//                    every accumulator register of o is multiplied by alpha (one rounding per key tile), then the mix chain.
//   forward, end:    Z = (z[s] + z[s ^ 1]) + (z[s ^ 2] + z[s ^ 3]) over the four lanes s = lane >> 4 of a query;
//                    o = acc / Z (ONE IEEE division per element);  lse = m + logf(Z).
//   delta            one fmaf chain over the Dv channels ascending from 0.0f.
//   backward         P = expf(scale * S - lse); dS = P * (dP - delta) (rows past the end: 0.0f); dq = scale * acc, dk = scale *
//                    acc, dv = acc; with NS > 1 slabs: dk, dv = ((part[0] + part[1]) + part[2]) + .. (scale already applied).
#include "common.h"
#include "u2pl_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define ATTN_BQ 64             // owned rows of a block: 4 waves of 16
#define ATTN_BK 64             // walked rows of one tile: 4 sub-tiles of 16
#define ATTN_DVC 128           // channels of one mix pass: 8 accumulator tiles of 16
#define ATTN_JT 8              // ATTN_DVC / 16
#define ATTN_MAX_D 128
#define ATTN_MAX_DV 512
#define ATTN_MAX_BLOCKS 4096   // grid cap of every kernel of this file (grid-stride over work items)
#define ATTN_FILL 512          // key-owning blocks wanted before the queries are cut into slabs
#define ATTN_SLAB_MIN 256      // a slab has at least this many queries
#define ATTN_MAX_SLABS 32

__device__ __forceinline__ float4 a4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 a4ld(const float* p) { return *(const float4*)p; }
#define ATTN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// acc[t][r] = sum over c < Wd of A[a0 + 16 t + 4 (lane >> 4) + r][c] * brow[c]  (brow: the lane's owned row, null: a padding row)
// rows of A at or past aend feed 0.0f
__device__ __forceinline__ void attn_dots(const float* __restrict__ A, long lda, long a0, long aend, const float* __restrict__ brow,
                                          int Wd, int li, int lk, f32x4 acc[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Wd; c0 += 16) {
        const int c = c0 + 4 * lk;
        const bool cok = c < Wd;
        const float4 b = (brow != nullptr && cok) ? a4ld(brow + c) : a4zero();
        float4 a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long row = a0 + 16 * t + li;
            a[t] = (row < aend && cok) ? a4ld(A + row * lda + c) : a4zero();
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = ATTN_MFMA(a[t].x, b.x, acc[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = ATTN_MFMA(a[t].y, b.y, acc[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = ATTN_MFMA(a[t].z, b.z, acc[t]);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = ATTN_MFMA(a[t].w, b.w, acc[t]);
    }
}

// acc[j][r'] (channel c0 + 16 j + 4 (lane >> 4) + r', owned row lane & 15) += sum over the walked rows a0 + 16 t + 4 s + r of
// X[row][channel] * w[t][r] of the lane (s, owned row); rows at or past aend and channels at or past Wd feed 0.0f
__device__ __forceinline__ void attn_mix(const float* __restrict__ X, long ldx, long a0, long aend, int c0, int Wd, const f32x4 w[4],
                                         int li, int lk, f32x4 acc[ATTN_JT]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (a0 + 16 * t >= aend) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = a0 + 16 * t + 4 * lk + r;
            const bool rok = row < aend;
            const float* xr = X + row * ldx + c0 + li;
#pragma unroll
            for (int j = 0; j < ATTN_JT; ++j) {
                if (c0 + 16 * j >= Wd) continue;
                const float a = (rok && c0 + 16 * j + li < Wd) ? xr[16 * j] : 0.f;
                acc[j] = ATTN_MFMA(a, w[t][r], acc[j]);
            }
        }
    }
}

// out[owned row][c0 + 16 j + 4 (lane >> 4) .. + 3] = f * acc[j] (mode 0), acc[j] / f (mode 1)
template <int MODE>
__device__ __forceinline__ void attn_store(float* __restrict__ orow, int c0, int Wd, const f32x4 acc[ATTN_JT], float f, int lk) {
#pragma unroll
    for (int j = 0; j < ATTN_JT; ++j) {
        const int c = c0 + 16 * j + 4 * lk;
        if (c >= Wd) continue;
        float4 o;
        if (MODE == 1)
            o = make_float4(__fdiv_rn(acc[j][0], f), __fdiv_rn(acc[j][1], f), __fdiv_rn(acc[j][2], f), __fdiv_rn(acc[j][3], f));
        else
            o = make_float4(__fmul_rn(f, acc[j][0]), __fmul_rn(f, acc[j][1]), __fmul_rn(f, acc[j][2]), __fmul_rn(f, acc[j][3]));
        *(float4*)(orow + c) = o;
    }
}

struct AttnP {
    long ldq, ldk, ldv, ldo, ldg, ldout;
    float scale;
    int N, heads, Pq, Pk, D, Dv;
    int NS, rows;           // query slabs of the key-owning kernels, queries per slab (a multiple of ATTN_BK)
};

// items: (image, head) x value chunk x query tile
__global__ void __launch_bounds__(256) k_attn_fwd(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                  float* __restrict__ o, float* __restrict__ lse, const AttnP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const long QT = (p.Pq + ATTN_BQ - 1) / ATTN_BQ, CH = (p.Dv + ATTN_DVC - 1) / ATTN_DVC;
    const long items = (long)p.N * p.heads * CH * QT;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long qt = it % QT;
        const int ch = (int)((it / QT) % CH);
        const long nh = it / (QT * CH);
        const int h = (int)(nh % p.heads);
        const long n = nh / p.heads;
        const long qw = qt * ATTN_BQ + wave * 16;
        if (qw >= p.Pq) continue;
        const long qrow = qw + li;
        const bool qok = qrow < p.Pq;
        const float* qp = qok ? q + (n * p.Pq + qrow) * p.ldq + (long)h * p.D : nullptr;
        const float* kb = k + n * p.Pk * p.ldk + (long)h * p.D;
        const float* vb = v + n * p.Pk * p.ldv + (long)h * p.Dv;
        const int c0 = ch * ATTN_DVC;
        f32x4 acc[ATTN_JT];
#pragma unroll
        for (int j = 0; j < ATTN_JT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float m = -INFINITY, z = 0.f;
        for (long k0 = 0; k0 < p.Pk; k0 += ATTN_BK) {
            f32x4 s[4];
            attn_dots(kb, p.ldk, k0, p.Pk, qp, p.D, li, lk, s);
            float mt = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = k0 + 16 * t + 4 * lk + r < p.Pk;
                    s[t][r] = ok ? __fmul_rn(p.scale, s[t][r]) : -INFINITY;
                    mt = fmaxf(mt, s[t][r]);
                }
            mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float mn = fmaxf(m, mt);
            const float alpha = expf(__fsub_rn(m, mn));
            m = mn;
            z = __fmul_rn(z, alpha);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = k0 + 16 * t + 4 * lk + r < p.Pk;
                    s[t][r] = ok ? expf(__fsub_rn(s[t][r], mn)) : 0.f;
                    z = __fadd_rn(z, s[t][r]);
                }
#pragma unroll
            for (int j = 0; j < ATTN_JT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] = __fmul_rn(acc[j][r], alpha);
            attn_mix(vb, p.ldv, k0, p.Pk, c0, p.Dv, s, li, lk, acc);
        }
        z = __fadd_rn(z, __shfl_xor(z, 16, 64));
        z = __fadd_rn(z, __shfl_xor(z, 32, 64));
        if (qok) {
            attn_store<1>(o + (n * p.Pq + qrow) * p.ldo + (long)h * p.Dv, c0, p.Dv, acc, z, lk);
            if (ch == 0 && lk == 0) lse[nh * p.Pq + qrow] = __fadd_rn(m, logf(z));
        }
    }
}

// delta[(n heads + h) Pq + p] = g[p, h, :] . o[p, h, :]
__global__ void __launch_bounds__(256) k_attn_delta(const float* __restrict__ g, const float* __restrict__ o, float* __restrict__ delta,
                                                    const AttnP p) {
    const long total = (long)p.N * p.heads * p.Pq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i % p.Pq, nh = i / p.Pq;
        const int h = (int)(nh % p.heads);
        const long n = nh / p.heads;
        const float* gp = g + (n * p.Pq + row) * p.ldg + (long)h * p.Dv;
        const float* op = o + (n * p.Pq + row) * p.ldo + (long)h * p.Dv;
        float acc = 0.f;
        for (int c = 0; c < p.Dv; c += 4) {
            const float4 a = a4ld(gp + c), b = a4ld(op + c);
            acc = __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, __fmaf_rn(a.x, b.x, acc))));
        }
        delta[i] = acc;
    }
}

// items: (image, head) x query tile
__global__ void __launch_bounds__(256) k_attn_dq(const float* __restrict__ g, const float* __restrict__ q, const float* __restrict__ k,
                                                 const float* __restrict__ v, const float* __restrict__ lse,
                                                 const float* __restrict__ delta, float* __restrict__ dq, const AttnP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const long QT = (p.Pq + ATTN_BQ - 1) / ATTN_BQ;
    const long items = (long)p.N * p.heads * QT;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long qt = it % QT, nh = it / QT;
        const int h = (int)(nh % p.heads);
        const long n = nh / p.heads;
        const long qw = qt * ATTN_BQ + wave * 16;
        if (qw >= p.Pq) continue;
        const long qrow = qw + li;
        const bool qok = qrow < p.Pq;
        const float* qp = qok ? q + (n * p.Pq + qrow) * p.ldq + (long)h * p.D : nullptr;
        const float* gp = qok ? g + (n * p.Pq + qrow) * p.ldg + (long)h * p.Dv : nullptr;
        const float ls = qok ? lse[nh * p.Pq + qrow] : 0.f;
        const float dl = qok ? delta[nh * p.Pq + qrow] : 0.f;
        const float* kb = k + n * p.Pk * p.ldk + (long)h * p.D;
        const float* vb = v + n * p.Pk * p.ldv + (long)h * p.Dv;
        f32x4 acc[ATTN_JT];
#pragma unroll
        for (int j = 0; j < ATTN_JT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (long k0 = 0; k0 < p.Pk; k0 += ATTN_BK) {
            f32x4 s[4], dp[4];
            attn_dots(kb, p.ldk, k0, p.Pk, qp, p.D, li, lk, s);
            attn_dots(vb, p.ldv, k0, p.Pk, gp, p.Dv, li, lk, dp);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = k0 + 16 * t + 4 * lk + r < p.Pk;
                    const float pw = expf(__fsub_rn(__fmul_rn(p.scale, s[t][r]), ls));
                    s[t][r] = ok ? __fmul_rn(pw, __fsub_rn(dp[t][r], dl)) : 0.f;
                }
            attn_mix(kb, p.ldk, k0, p.Pk, 0, p.D, s, li, lk, acc);
        }
        if (qok) attn_store<0>(dq + (n * p.Pq + qrow) * p.ldout + (long)h * p.D, 0, p.D, acc, p.scale, lk);
    }
}

// items: slab x (image, head) x channel chunk x key tile.  DK: out = dk (one chunk: D <= ATTN_DVC); else out = dv.
// NS == 1: out is the caller's tensor (pitch ldout); NS > 1: the partials [slab][N*Pk][heads*width], dense.
template <bool DK>
__global__ void __launch_bounds__(256) k_attn_kgrad(const float* __restrict__ g, const float* __restrict__ q, const float* __restrict__ k,
                                                    const float* __restrict__ v, const float* __restrict__ lse,
                                                    const float* __restrict__ delta, float* __restrict__ out, const AttnP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int Wd = DK ? p.D : p.Dv;
    const long KT = (p.Pk + ATTN_BQ - 1) / ATTN_BQ, CH = (Wd + ATTN_DVC - 1) / ATTN_DVC;
    const long per_slab = (long)p.N * p.heads * CH * KT;
    const long items = per_slab * p.NS;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long slab = it / per_slab;
        long rest = it - slab * per_slab;
        const long kt = rest % KT;
        rest /= KT;
        const int ch = (int)(rest % CH);
        const long nh = rest / CH;
        const int h = (int)(nh % p.heads);
        const long n = nh / p.heads;
        const long kw = kt * ATTN_BQ + wave * 16;
        if (kw >= p.Pk) continue;
        const long krow = kw + li;
        const bool kok = krow < p.Pk;
        const float* kp = kok ? k + (n * p.Pk + krow) * p.ldk + (long)h * p.D : nullptr;
        const float* vp = (DK && kok) ? v + (n * p.Pk + krow) * p.ldv + (long)h * p.Dv : nullptr;
        const float* qb = q + n * p.Pq * p.ldq + (long)h * p.D;
        const float* gb = g + n * p.Pq * p.ldg + (long)h * p.Dv;
        const float* lb = lse + nh * p.Pq;
        const float* db = DK ? delta + nh * p.Pq : nullptr;
        const long r0 = slab * p.rows;
        const long r1 = r0 + p.rows < p.Pq ? r0 + p.rows : (long)p.Pq;
        const int c0 = ch * ATTN_DVC;
        f32x4 acc[ATTN_JT];
#pragma unroll
        for (int j = 0; j < ATTN_JT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (long q0 = r0; q0 < r1; q0 += ATTN_BK) {
            f32x4 s[4], dp[4];
            attn_dots(qb, p.ldq, q0, r1, kp, p.D, li, lk, s);
            if (DK) attn_dots(gb, p.ldg, q0, r1, vp, p.Dv, li, lk, dp);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long row = q0 + 16 * t + 4 * lk + r;
                    const bool ok = row < r1;
                    const float ls = ok ? lb[row] : 0.f;
                    const float pw = expf(__fsub_rn(__fmul_rn(p.scale, s[t][r]), ls));
                    if (DK) {
                        const float dl = ok ? db[row] : 0.f;
                        s[t][r] = ok ? __fmul_rn(pw, __fsub_rn(dp[t][r], dl)) : 0.f;
                    } else {
                        s[t][r] = ok ? pw : 0.f;
                    }
                }
            attn_mix(DK ? qb : gb, DK ? p.ldq : p.ldg, q0, r1, c0, Wd, s, li, lk, acc);
        }
        if (kok) {
            const long wt = (long)p.heads * Wd;
            float* orow = p.NS > 1 ? out + ((slab * p.N + n) * p.Pk + krow) * wt + (long)h * Wd
                                   : out + (n * p.Pk + krow) * p.ldout + (long)h * Wd;
            attn_store<0>(orow, c0, Wd, acc, DK ? p.scale : 1.f, lk);
        }
    }
}

// out[row][c] = ((part[0] + part[1]) + part[2]) + ..: slab order
__global__ void __launch_bounds__(256) k_attn_finish(const float* __restrict__ part, int NS, long rows, int width, float* __restrict__ out,
                                                     long ldo) {
    const long E = rows * width;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < E; i += (long)gridDim.x * 256) {
        float s = part[i];
        for (int j = 1; j < NS; ++j) s = __fadd_rn(s, part[(long)j * E + i]);
        out[(i / width) * ldo + i % width] = s;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static bool attn_shape_ok(int N, int heads, int Pq, int Pk, int D, int Dv) {
    if (N < 1 || heads < 1 || Pq < 1 || Pk < 1) return false;
    if (D < 4 || D > ATTN_MAX_D || D % 4 || Dv < 4 || Dv > ATTN_MAX_DV || Dv % 4) return false;
    const long lim = 1L << 31;
    return (long)N * heads < lim && (long)N * heads * Pq < lim && (long)N * Pq < lim && (long)N * Pk < lim;
}
static bool attn_rows_ok(const void* ptr, long ld, long width) {
    return ptr != nullptr && ld >= width && ld % 4 == 0 && ((uintptr_t)ptr & 15) == 0;
}
static inline long attn_up4(long n) { return (n + 3) & ~3L; }
static inline unsigned attn_grid(long items) { return (unsigned)(items < ATTN_MAX_BLOCKS ? (items < 1 ? 1 : items) : ATTN_MAX_BLOCKS); }
static inline long attn_cdiv(long a, long b) { return (a + b - 1) / b; }

// the slab rule of the key-owning kernels: a function of N, heads, Pq and Pk alone
static void attn_slabs(int N, int heads, int Pq, int Pk, int& NS, int& rows) {
    const long tiles = (long)N * heads * attn_cdiv(Pk, ATTN_BQ);
    long ns = attn_cdiv(ATTN_FILL, tiles);
    const long cap = attn_cdiv(Pq, ATTN_SLAB_MIN);
    if (ns > cap) ns = cap;
    if (ns > ATTN_MAX_SLABS) ns = ATTN_MAX_SLABS;
    if (ns < 1) ns = 1;
    rows = (int)(attn_cdiv(attn_cdiv(Pq, ns), ATTN_BK) * ATTN_BK);
    NS = (int)attn_cdiv(Pq, rows);
}

U2PL_API size_t u2pl_attn_fwd_ws_floats(int, int, int, int, int, int) { return 0; }

U2PL_API int u2pl_attn_fwd_f32(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float scale, int N, int heads,
                               int Pq, int Pk, int D, int Dv, float* o, long ldo, float* lse, float* ws, hipStream_t stream) {
    (void)ws;
    if (!attn_shape_ok(N, heads, Pq, Pk, D, Dv) || !attn_rows_ok(q, ldq, (long)heads * D) || !attn_rows_ok(k, ldk, (long)heads * D) ||
        !attn_rows_ok(v, ldv, (long)heads * Dv) || !attn_rows_ok(o, ldo, (long)heads * Dv) || lse == nullptr)
        return U2PL_EINVAL;
    AttnP p = {};
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.scale = scale;
    p.N = N, p.heads = heads, p.Pq = Pq, p.Pk = Pk, p.D = D, p.Dv = Dv;
    const long items = (long)N * heads * attn_cdiv(Dv, ATTN_DVC) * attn_cdiv(Pq, ATTN_BQ);
    U2PL_LAUNCH(k_attn_fwd, dim3(attn_grid(items)), dim3(256), 0, stream, q, k, v, o, lse, p);
    U2PL_LAUNCH_CHECK();
    return 0;
}

U2PL_API size_t u2pl_attn_bwd_ws_floats(int N, int heads, int Pq, int Pk, int D, int Dv) {
    if (!attn_shape_ok(N, heads, Pq, Pk, D, Dv)) return 0;
    int NS, rows;
    attn_slabs(N, heads, Pq, Pk, NS, rows);
    size_t n = (size_t)attn_up4((long)N * heads * Pq);
    if (NS > 1) n += (size_t)NS * N * Pk * heads * ((size_t)D + Dv);
    return n;
}

U2PL_API int u2pl_attn_bwd_f32(const float* g, long ldg, const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                               const float* o, long ldo, const float* lse, float scale, int N, int heads, int Pq, int Pk, int D, int Dv,
                               float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, float* ws, hipStream_t stream) {
    if (!attn_shape_ok(N, heads, Pq, Pk, D, Dv) || !attn_rows_ok(g, ldg, (long)heads * Dv) || !attn_rows_ok(q, ldq, (long)heads * D) ||
        !attn_rows_ok(k, ldk, (long)heads * D) || lse == nullptr || (!dq && !dk && !dv) || !attn_rows_ok(ws, 4, 4))
        return U2PL_EINVAL;
    if ((dq || dk) && (!attn_rows_ok(v, ldv, (long)heads * Dv) || !attn_rows_ok(o, ldo, (long)heads * Dv))) return U2PL_EINVAL;
    if (dq && !attn_rows_ok(dq, lddq, (long)heads * D)) return U2PL_EINVAL;
    if (dk && !attn_rows_ok(dk, lddk, (long)heads * D)) return U2PL_EINVAL;
    if (dv && !attn_rows_ok(dv, lddv, (long)heads * Dv)) return U2PL_EINVAL;
    AttnP p = {};
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.ldg = ldg, p.scale = scale;
    p.N = N, p.heads = heads, p.Pq = Pq, p.Pk = Pk, p.D = D, p.Dv = Dv;
    attn_slabs(N, heads, Pq, Pk, p.NS, p.rows);
    float* delta = ws;
    float* pk = ws + attn_up4((long)N * heads * Pq);
    float* pv = pk + (p.NS > 1 ? (long)p.NS * N * Pk * heads * D : 0);
    const long nhq = (long)N * heads * Pq;
    if (dq || dk) {
        U2PL_LAUNCH(k_attn_delta, dim3(attn_grid(attn_cdiv(nhq, 256))), dim3(256), 0, stream, g, o, delta, p);
        U2PL_LAUNCH_CHECK();
    }
    if (dq) {
        p.ldout = lddq;
        U2PL_LAUNCH(k_attn_dq, dim3(attn_grid((long)N * heads * attn_cdiv(Pq, ATTN_BQ))), dim3(256), 0, stream, g, q, k, v, lse, delta, dq,
                    p);
        U2PL_LAUNCH_CHECK();
    }
    const long kt = (long)N * heads * attn_cdiv(Pk, ATTN_BQ) * p.NS;
    if (dk) {
        p.ldout = lddk;
        U2PL_LAUNCH(k_attn_kgrad<true>, dim3(attn_grid(kt)), dim3(256), 0, stream, g, q, k, v, lse, delta, p.NS > 1 ? pk : dk, p);
        U2PL_LAUNCH_CHECK();
        if (p.NS > 1) {
            const long E = (long)N * Pk * heads * D;
            U2PL_LAUNCH(k_attn_finish, dim3(attn_grid(attn_cdiv(E, 256))), dim3(256), 0, stream, pk, p.NS, (long)N * Pk, heads * D, dk, lddk);
            U2PL_LAUNCH_CHECK();
        }
    }
    if (dv) {
        p.ldout = lddv;
        U2PL_LAUNCH(k_attn_kgrad<false>, dim3(attn_grid(kt * attn_cdiv(Dv, ATTN_DVC))), dim3(256), 0, stream, g, q, k, v, lse, delta,
                    p.NS > 1 ? pv : dv, p);
        U2PL_LAUNCH_CHECK();
        if (p.NS > 1) {
            const long E = (long)N * Pk * heads * Dv;
            U2PL_LAUNCH(k_attn_finish, dim3(attn_grid(attn_cdiv(E, 256))), dim3(256), 0, stream, pv, p.NS, (long)N * Pk, heads * Dv, dv, lddv);
            U2PL_LAUNCH_CHECK();
        }
    }
    return 0;
}
