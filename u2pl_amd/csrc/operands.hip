// The GEMM operands derived from the weights (the C counterpart of u2pl_amd/operands.py): the bf16 / fp16 piece planes that the
// pre-split GEMMs of igemm_ws.hip copy straight into their LDS tiles, the maxima behind the fp16 planes, and max |x| of an
// activation operand.  Layout: ws_planes.h.  Three ways to build planes:
//   * one weight, lazily on first use: u2pl_weight_split3_f32 (bf16) / u2pl_weight_split2h_f32 (fp16);
//   * every bf16 operand of a model from a job table: u2pl_weight_split3_multi_f32;
//   * every fp16 operand of a model from the weights alone: u2pl_weight_rebuild2h_f32.
// All of them write through the same few device functions below -- the plane address, the source segment, the job lookup, the
// split-and-store, the maxima tail -- so the format exists once.
#include "common.h"
#include "conv_geom.h"
#include "u2pl_hip.h"
#include "wino_t.h"
#include "ws_planes.h"

// ---------------------------------------------------------------------------------------------------------------
// the format, once
// ---------------------------------------------------------------------------------------------------------------
// element offset of the 16-byte segment s (8 k) of row n in chunk c, first of NP piece planes (the next piece: + Np * 32)
template <int NP>
__device__ __forceinline__ long ws_plane_off(int c, int n, int s, int Np) {
    return (((long)c * NP) * Np + n) * 32 + ((s ^ ((n >> 2) & 3)) << 3);
}
// the eight source floats k = sg * 8 .. sg * 8 + 7 of row n (zeros for the padding rows n >= rows).  kind 0: src = [rows][K]
// row-major; kind 1: src = the convolution weight [Cout][RS][Cin] read as its transpose [rows = Cin][K = RS * Cout], (rs, co) =
// the tap and output channel of the segment's first k (k = rs * Cout + co)
__device__ __forceinline__ void ws_src8(const float* __restrict__ src, int kind, int rows, int K, int RS, unsigned Cout, int n, int sg,
                                        unsigned rs, unsigned co, float (&e)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) e[q] = 0.f;
    if (n < rows) {
        if (kind == 0) {
            const float4* p = (const float4*)(src + (long)n * K + sg * 8);
            const float4 v0 = p[0], v1 = p[1];
            e[0] = v0.x; e[1] = v0.y; e[2] = v0.z; e[3] = v0.w;
            e[4] = v1.x; e[5] = v1.y; e[6] = v1.z; e[7] = v1.w;
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                e[q] = src[((long)co * RS + rs) * rows + n];
                if (++co == Cout) { co = 0; ++rs; }
            }
        }
    }
}
// highest job whose `begin` field is <= i (jobs of length 0 share their begin with the next job and are never the highest)
template <class F>
__device__ __forceinline__ int rb_find(int n, long i, F&& begin) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (begin(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// eight values v[0 .. 7] -> NP pieces of 16 bytes each, pl elements apart.  NP == 3: bf16 pieces (sc unused); NP == 2: fp16 pieces of v * sc
template <int NP>
__device__ __forceinline__ void ws_split_store(unsigned short* out, long pl, const float (&v)[8], float sc) {
    static_assert(NP == 2 || NP == 3, "pieces per operand");
    if constexpr (NP == 3) {
        uint2 a0, a1, a2, b0, b1, b2;
        split3_bf16(make_float4(v[0], v[1], v[2], v[3]), a0, a1, a2);
        split3_bf16(make_float4(v[4], v[5], v[6], v[7]), b0, b1, b2);
        *(uint4*)out = make_uint4(a0.x, a0.y, b0.x, b0.y);
        *(uint4*)(out + pl) = make_uint4(a1.x, a1.y, b1.x, b1.y);
        *(uint4*)(out + 2 * pl) = make_uint4(a2.x, a2.y, b2.x, b2.y);
    } else {
        uint2 a0, a1, b0, b1;
        split2_f16(make_float4(v[0], v[1], v[2], v[3]), sc, a0, a1);
        split2_f16(make_float4(v[4], v[5], v[6], v[7]), sc, b0, b1);
        *(uint4*)out = make_uint4(a0.x, a0.y, b0.x, b0.y);
        *(uint4*)(out + pl) = make_uint4(a1.x, a1.y, b1.x, b1.y);
    }
}
// the maxima behind the fp16 planes of `batch` matrices: one uint32 per matrix (the fp32 bit pattern of its max |w|: the GEMM
// derives the power-of-two scale from it with split2_exp_bits, exactly as the split does); cleared with the whole 16-byte-rounded
// tail (no uninitialised bytes) before the maxima are accumulated with atomicMax (order-independent, deterministic)
__device__ __forceinline__ unsigned* ws2_tail(unsigned short* out, int Np, int K, int batch) {
    return (unsigned*)((char*)out + ws2_plane_bytes(Np, K, batch));
}
__device__ __forceinline__ void ws2_tail_clear(unsigned* tail, int batch) {
    const int n = (batch + 3) & ~3;
    for (int z = 0; z != n; ++z) tail[z] = 0u;
}

// ---------------------------------------------------------------------------------------------------------------
// planes of `batch` matrices from one source: the one-weight calls (the lazy path) and the bf16 job table.
// A job covers the 16-byte output segments [seg_begin, seg_begin + batch * Np * K / 8); kind as in ws_src8 (the matrices of a batch
// rows * K floats apart).  kind 0: sg fastest; kind 1: n fastest (neighbouring lanes read neighbouring input channels).
// ---------------------------------------------------------------------------------------------------------------
struct SplitJob { const float* src; unsigned short* out; long seg_begin; int rows, Np, K, kind, RS, batch; };
// segment r of job j -> matrix z, row n, segment sg
struct SegPos { int z, n, sg; };
__device__ __forceinline__ SegPos split_job_decode(const SplitJob& j, long r) {
    const int nseg = j.K / 8;
    const long per = (long)j.Np * nseg;
    const int z = (int)(r / per);
    r -= (long)z * per;
    if (j.kind == 0) return {z, (int)(r / nseg), (int)(r % nseg)};
    return {z, (int)(r % j.Np), (int)(r / j.Np)};
}
// NP == 2: scaled by the maximum that lies behind the planes
template <int NP>
__device__ __forceinline__ void split_job_segment(const SplitJob& j, long r) {
    const SegPos p = split_job_decode(j, r);
    const int z = p.z, n = p.n, sg = p.sg;
    const unsigned Cout = j.kind == 1 ? (unsigned)(j.K / j.RS) : 1u;
    const unsigned rs = j.kind == 1 ? (unsigned)(sg * 8) / Cout : 0u, co = j.kind == 1 ? (unsigned)(sg * 8) - rs * Cout : 0u;
    float v[8];
    ws_src8(j.src + (long)z * j.rows * j.K, j.kind, j.rows, j.K, j.RS, Cout, n, sg, rs, co, v);
    float sc = 1.f;
    if constexpr (NP == 2) sc = split2_scale(split2_exp_bits(ws2_tail(j.out, j.Np, j.K, j.batch)[z]));
    const long pl = (long)j.Np * 32;
    ws_split_store<NP>(j.out + (long)z * (j.K / 32) * NP * pl + ws_plane_off<NP>(sg >> 2, n, sg & 3, j.Np), pl, v, sc);
}

// ---- bf16 planes: out [K/32][3][Np][32] per matrix ----
__global__ void k_weight_split3(const SplitJob j, long total) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) split_job_segment<3>(j, i);
}
// every bf16 split of a model in ONE launch (operands.presplit under U2PL_CONV_H=0, after the optimizer / EMA update)
__global__ void k_weight_split3_multi(const SplitJob* __restrict__ jobs, int njobs, long total) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const SplitJob j = jobs[rb_find(njobs, i, [&](int m) { return jobs[m].seg_begin; })];
        split_job_segment<3>(j, i - j.seg_begin);
    }
}
// jobs: device array of njobs SplitJob (48 bytes each: src, out, seg_begin, rows, Np = u2pl_weight_split3_pad_rows(rows), K,
// kind, RS, batch); total = sum over jobs of batch * Np * K / 8
U2PL_API int u2pl_weight_split3_multi_f32(const void* jobs, int njobs, long total, hipStream_t stream) {
    if (njobs <= 0 || total <= 0) return njobs == 0 ? 0 : U2PL_EINVAL;
    U2PL_LAUNCH(k_weight_split3_multi, dim3(grid_for(total, 256, 4096)), dim3(256), 0, stream, (const SplitJob*)jobs, njobs, total);
    U2PL_LAUNCH_CHECK();
    return 0;
}
U2PL_API int u2pl_weight_split3_pad_rows(int rows) { return ws_pad_rows(rows); }

U2PL_API size_t u2pl_weight_split3_bytes(int rows, int K, int batch) {
    return (size_t)batch * (K / 32) * 3 * ws_pad_rows(rows) * WS_ROW_B;
}
// the job of a one-weight call: `batch` row-major matrices [rows][K], rows * K floats apart.  It travels in the kernel arguments
// (no upload, nothing that could outlive the caller's stack)
static int split_job_one(const float* w, long zw, int rows, int K, int batch, void* out, SplitJob& j, long& total) {
    if (rows <= 0 || K <= 0 || (K % 32) || batch <= 0) return U2PL_EINVAL;
    if (batch > 1 && zw != (long)rows * K) return U2PL_EINVAL;
    const int Np = ws_pad_rows(rows);
    j = {w, (unsigned short*)out, 0, rows, Np, K, 0, 1, batch};
    total = (long)batch * Np * (K / 8);
    return 0;
}
// split planes of `batch` row-major fp32 matrices [rows][K] (zw = rows * K floats apart; the split copies are
// u2pl_weight_split3_bytes(rows, K, 1) bytes apart).  K % 32 == 0.
U2PL_API int u2pl_weight_split3_f32(const float* w, long zw, int rows, int K, int batch, void* out, hipStream_t stream) {
    SplitJob j;
    long total;
    if (int rc = split_job_one(w, zw, rows, K, batch, out, j, total)) return rc;
    U2PL_LAUNCH(k_weight_split3, dim3(grid_for(total, 256, 4096)), dim3(256), 0, stream, j, total);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---- fp16 planes (conv_geom.h "split-fp16"): out [K/32][2][Np][32] per matrix, then the maxima (ws2_tail).  Three launches: the
// maxima are cleared, computed, and consumed by the split ----
__global__ void k_weight_amax_clear(const SplitJob j) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ws2_tail_clear(ws2_tail(j.out, j.Np, j.K, j.batch), j.batch);
}
// block b covers the contiguous segments [b * WS_AMAX_SPAN, (b + 1) * WS_AMAX_SPAN): a thread keeps a running maximum for the
// matrix it is in and publishes when it crosses into another (rare) and at its end -- per wave one atomic where the lanes agree on
// the matrix.  (One atomic per wave and segment-strided blocks: 590 K same-line atomics per rebuild, 27 ms -- measured.)
#define WS_AMAX_SPAN 8192
__global__ __launch_bounds__(256) void k_weight_absmax(const SplitJob j, long total) {
    const long begin = (long)blockIdx.x * WS_AMAX_SPAN, end = begin + WS_AMAX_SPAN < total ? begin + WS_AMAX_SPAN : total;
    unsigned* slot = nullptr;
    unsigned m = 0u;
    for (long i = begin + threadIdx.x; i < end; i += 256) {
        const SegPos p = split_job_decode(j, i);
        unsigned* sl = ws2_tail(j.out, j.Np, j.K, j.batch) + p.z;
        if (sl != slot) {
            if (slot && m) atomicMax(slot, m);
            slot = sl;
            m = 0u;
        }
        float v[8];
        ws_src8(j.src + (long)p.z * j.rows * j.K, 0, j.rows, j.K, 1, 1u, p.n, p.sg, 0u, 0u, v);
#pragma unroll
        for (int q = 0; q < 8; ++q) m = amax_bits(m, v[q]);
    }
    // (all lanes arrive here; lanes that never entered the loop hold slot == nullptr)
    const unsigned long long key = (unsigned long long)slot;
    const unsigned long long first = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key) |
                                     ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32)) << 32);
    if (__all(key == first)) {
        m = wave_max_u(m);
        if ((threadIdx.x & 63) == 0 && slot && m) atomicMax(slot, m);
    } else if (slot && m) {
        atomicMax(slot, m);
    }
}
__global__ __launch_bounds__(256) void k_weight_split2h(const SplitJob j, long total) {
    const long begin = (long)blockIdx.x * WS_AMAX_SPAN, end = begin + WS_AMAX_SPAN < total ? begin + WS_AMAX_SPAN : total;
    for (long i = begin + threadIdx.x; i < end; i += 256) split_job_segment<2>(j, i);
}
U2PL_API size_t u2pl_weight_split2h_bytes(int rows, int K, int batch) {
    return ws2_plane_bytes(ws_pad_rows(rows), K, batch) + (((size_t)batch * 4 + 15) & ~(size_t)15);
}
// one weight (batch matrices [rows][K], zw = rows * K floats apart): clears the maxima, computes them, writes the planes
U2PL_API int u2pl_weight_split2h_f32(const float* w, long zw, int rows, int K, int batch, void* out, hipStream_t stream) {
    SplitJob j;
    long total;
    if (int rc = split_job_one(w, zw, rows, K, batch, out, j, total)) return rc;
    const dim3 grid((unsigned)cdiv(total, WS_AMAX_SPAN));
    U2PL_LAUNCH(k_weight_amax_clear, dim3(1), dim3(256), 0, stream, j);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_weight_absmax, grid, dim3(256), 0, stream, j, total);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_weight_split2h, grid, dim3(256), 0, stream, j, total);
    U2PL_LAUNCH_CHECK();
    return 0;
}
// ---------------------------------------------------------------------------------------------------------------
// The once-per-step rebuild of every split-fp16 operand of a model (operands.presplit): the planes and maxima the calls above
// produce weight by weight, bit for bit, from the WEIGHTS alone -- no fp32 scratch:
//   * kinds 0 / 1 (the weight as it lies / read as its transpose, one matrix per job): max |w| is the same number for every
//     operand of a weight, so it is computed ONCE per weight, in one linear pass over the source (amax_begin: the weight's place in
//     that pass, in float4; the further jobs of the same weight have length 0 there) and published to amax_dst -- the word
//     behind the FIRST job's planes.  Every job of the weight scales by *amax_dst and leaves a copy behind its own planes.
//   * kinds 2 / 3 (Winograd-domain filters of a 3x3 weight [O][3][3][C]: U[z][O][C] = G g G^T, / of the 180-degree-rotated taps,
//     U'[z][C][O]; (mt + 2)^2 matrices per job): both passes recompute the components in registers with wino_filter_row
//     (wino_t.h: the operations of wino_weight_one) instead of reading a U that a transform launch wrote: per filter 36 B of
//     taps read twice against 144 B written and 288 B read.  A block works on ONE job (mblk_begin / pblk_begin: the job's first
//     block in the maxima / pieces grid): mt, the orientation and the 36 scales are uniform.
// Positions are decoded once per block span (32-bit) and stepped: no division in the loops.
// Four launches: (1) the maxima words are cleared, (2) the maxima of every kind, (3) the pieces of kinds 0 / 1, (4) the pieces of
// kinds 2 / 3.  (3) and (4) stay apart: the Winograd pieces kernel holds a thread's 72 taps and a row of 48 components in
// registers and runs at a quarter of the waves per SIMD a streaming copy wants; in one kernel the plain planes would be
// written at that occupancy.  (1) cannot fold into (2): a block's atomicMax must not meet another block's clear.
// ---------------------------------------------------------------------------------------------------------------
struct RebuildJob {       // 72 bytes; mirrored by operands.py's numpy dtype
    const float* src;
    unsigned short* out;
    long seg_begin;       // kinds 0 / 1: the job's first 16-byte output segment in launch (3) (prefix sum of Np * K / 8)
    long amax_begin;      // kinds 0 / 1: the weight's first float4 in the maxima pass (prefix sum of rows * K / 4 over FIRST jobs)
    unsigned* amax_dst;   // kinds 0 / 1: the word behind the planes of the weight's first job
    int rows, Np, K, kind, RS, mt;
    int mblk_begin, pblk_begin;        // kinds 2 / 3: first block in the maxima / pieces grid
};
#define RB_WINO_MSPAN 2048             // Winograd maxima: (o, 4 channels) units per block -- 8192 filters, 288 KB of taps
#define RB_WINO_PSPAN 1024             // Winograd pieces: (row, 8 k) units per block -- 1.1 MB of planes at mt = 4
__host__ __device__ static inline int rb_batch(int kind, int mt) { return kind >= 2 ? (mt + 2) * (mt + 2) : 1; }
__device__ __forceinline__ unsigned* rb_tail(const RebuildJob& j) { return ws2_tail(j.out, j.Np, j.K, rb_batch(j.kind, j.mt)); }
__global__ void k_rebuild_clear(const RebuildJob* __restrict__ jobs, int njobs) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= njobs) return;
    const RebuildJob j = jobs[t];
    ws2_tail_clear(rb_tail(j), rb_batch(j.kind, j.mt));
}
// maxima of kinds 0 / 1: block b reads the float4 [b * WS_AMAX_SPAN, (b + 1) * WS_AMAX_SPAN) of the weights laid end to end, weight by
// weight (block-uniform), four independent 16-byte loads per thread and trip; one atomic per wave and weight
__device__ __forceinline__ void rb_amax_flat(const RebuildJob* __restrict__ jobs, int njobs, long total, int blk) {
    const long begin = (long)blk * WS_AMAX_SPAN, end = begin + WS_AMAX_SPAN < total ? begin + WS_AMAX_SPAN : total;
    int ji = rb_find(njobs, begin, [&](int m) { return jobs[m].amax_begin; });
    long pos = begin;
    while (pos < end) {
        const long jb = jobs[ji].amax_begin;
        long je = ji + 1 < njobs ? jobs[ji + 1].amax_begin : total;
        if (je <= pos) { ++ji; continue; }         // (a further job of a weight already counted)
        je = je < end ? je : end;
        const float4* __restrict__ src = (const float4*)jobs[ji].src - jb;
        unsigned m = 0u;
        for (long i = pos + threadIdx.x; i < je; i += 1024) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 v0 = src[i], v1 = i + 256 < je ? src[i + 256] : z, v2 = i + 512 < je ? src[i + 512] : z,
                         v3 = i + 768 < je ? src[i + 768] : z;
            m = amax_bits4(amax_bits4(amax_bits4(amax_bits4(m, v0), v1), v2), v3);
        }
        m = wave_max_u(m);
        if ((threadIdx.x & 63) == 0 && m) atomicMax(jobs[ji].amax_dst, m);
        pos = je;
        ++ji;
    }
}
// maxima of kinds 2 / 3: a thread takes (o, 4 channels) units -- nine float4 loads, the whole weight read linearly --, keeps the
// running maxima of the A * A components in registers across its filters; per block: wave reduce, LDS, ONE atomic per component
template <int MT>
__device__ __forceinline__ void rb_amax_wino(const RebuildJob& j, int lb, unsigned (*s_m)[36]) {
    constexpr int A = WinoT<MT>::A;
    const int O = j.kind == 3 ? j.K : j.rows, C = j.kind == 3 ? j.rows : j.K, C4 = C >> 2;
    const unsigned total = (unsigned)O * (unsigned)C4;
    const bool tr = j.kind == 3;
    unsigned m[A * A];
#pragma unroll
    for (int z = 0; z < A * A; ++z) m[z] = 0u;
    const unsigned u0 = (unsigned)lb * RB_WINO_MSPAN + threadIdx.x;
    for (int it = 0; it < RB_WINO_MSPAN / 256; ++it) {
        const unsigned u = u0 + it * 256;
        if (u >= total) break;
        const unsigned o = u / (unsigned)C4, c4 = u - o * (unsigned)C4;
        const float* __restrict__ p = j.src + (long)o * 9 * C + c4 * 4;
        float4 tp[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) tp[t] = *(const float4*)(p + (long)t * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            auto tap = [&](int r, int s) {
                const float4& v = tp[tr ? 8 - (r * 3 + s) : r * 3 + s];       // (transposed: taps rotated by 180 degrees)
                return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
            };
            wino_filter_rows<MT>(tap, [&](int i, const float (&r)[A]) {
#pragma unroll
                for (int q = 0; q < A; ++q) m[i * A + q] = amax_bits(m[i * A + q], r[q]);
            });
        }
    }
#pragma unroll
    for (int z = 0; z < A * A; ++z) {
        const unsigned w = wave_max_u(m[z]);
        if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6][z] = w;
    }
    __syncthreads();
    if (threadIdx.x < A * A) {
        const unsigned a = s_m[0][threadIdx.x], b = s_m[1][threadIdx.x], c = s_m[2][threadIdx.x], d = s_m[3][threadIdx.x];
        const unsigned ab = a > b ? a : b, cd = c > d ? c : d, w = ab > cd ? ab : cd;
        if (w) atomicMax(rb_tail(j) + threadIdx.x, w);
    }
}
__global__ __launch_bounds__(256) void k_rebuild_amax(const RebuildJob* __restrict__ jobs, int n_flat, int n_wino, long amax_total,
                                                      int flat_blocks) {
    __shared__ unsigned s_m[4][36];
    if ((int)blockIdx.x < flat_blocks) {
        rb_amax_flat(jobs, n_flat, amax_total, blockIdx.x);
        return;
    }
    const int b = (int)blockIdx.x - flat_blocks;
    const RebuildJob* __restrict__ wj = jobs + n_flat;
    const int ji = rb_find(n_wino, b, [&](int m) { return (long)wj[m].mblk_begin; });
    const RebuildJob j = wj[ji];
    if (j.mt == 4) rb_amax_wino<4>(j, b - j.mblk_begin, s_m);
    else rb_amax_wino<2>(j, b - j.mblk_begin, s_m);
}
// pieces of kinds 0 / 1: block b writes the 16-byte segments [b * WS_AMAX_SPAN, (b + 1) * WS_AMAX_SPAN) of the jobs laid end to end; a
// thread decodes (row n, segment sg) when it enters a job and steps them by 256 segments afterwards.
// kind 0: sg fastest (a row's K floats are contiguous); kind 1: n fastest (neighbouring lanes read neighbouring input channels)
__global__ __launch_bounds__(256) void k_rebuild_pieces_flat(const RebuildJob* __restrict__ jobs, int njobs, long total) {
    const long begin = (long)blockIdx.x * WS_AMAX_SPAN, end = begin + WS_AMAX_SPAN < total ? begin + WS_AMAX_SPAN : total;
    long i = begin + threadIdx.x;
    if (i >= end) return;
    int ji = rb_find(njobs, begin, [&](int m) { return jobs[m].seg_begin; });
    for (;;) {
        // (enter the job of segment i)
        while (ji + 1 < njobs && jobs[ji + 1].seg_begin <= i) ++ji;
        const RebuildJob j = jobs[ji];
        const long jend_all = ji + 1 < njobs ? jobs[ji + 1].seg_begin : total;
        const long jend = jend_all < end ? jend_all : end;
        const unsigned fast = j.kind == 0 ? (unsigned)(j.K >> 3) : (unsigned)j.Np;        // extent of the fast index
        const unsigned r = (unsigned)(i - j.seg_begin);
        unsigned slow = r / fast, fst = r - slow * fast;
        const unsigned dq = 256u / fast, dr = 256u - dq * fast;
        const unsigned am = *j.amax_dst;
        const float sc = split2_scale(split2_exp_bits(am));
        if (r == 0) *rb_tail(j) = am;                   // (the job's own copy of the weight's maximum; its first job rewrites the same value)
        const long pl = (long)j.Np * 32;
        // kind 1: (tap rs, output channel co) of the segment's first k, stepped with the segment (sg advances by dq, + 1 on a wrap)
        const unsigned Cout = j.kind == 1 ? (unsigned)(j.K / j.RS) : 1u;
        unsigned rs0 = j.kind == 1 ? (slow * 8u) / Cout : 0u, co0 = j.kind == 1 ? slow * 8u - rs0 * Cout : 0u;
        const unsigned dk_q = (8u * dq) / Cout, dk_r = 8u * dq - dk_q * Cout;
        for (; i < jend; i += 256) {
            const int n = j.kind == 0 ? (int)slow : (int)fst, sg = j.kind == 0 ? (int)fst : (int)slow;
            float v[8];
            ws_src8(j.src, j.kind, j.rows, j.K, j.RS, Cout, n, sg, rs0, co0, v);
            ws_split_store<2>(j.out + ws_plane_off<2>(sg >> 2, n, sg & 3, j.Np), pl, v, sc);
            slow += dq;
            fst += dr;
            rs0 += dk_q;
            co0 += dk_r;
            if (fst >= fast) { fst -= fast; ++slow; co0 += 8u; }
            while (co0 >= Cout) { co0 -= Cout; ++rs0; }
        }
        if (i >= end) return;
    }
}
// pieces of kinds 2 / 3: unit u of a job = (32-deep chunk c, row n, 16-byte segment s) with s fastest, then n: a wave writes 16 whole
// 64-byte rows (1 KB contiguous) per store; the thread loads the nine taps of its eight filters (kind 2: eight consecutive channels
// of filter n -- two float4 per tap; kind 3: the taps of filters k0 .. k0 + 7 at channel n, rotated) and produces the A * A components a
// G row at a time: A components of eight filters are split and stored before the next row is computed.
template <int MT>
__device__ __forceinline__ void rb_pieces_wino(const RebuildJob& j, int lb) {
    constexpr int A = WinoT<MT>::A;
    const bool tr = j.kind == 3;
    const int C = tr ? j.rows : j.K;
    const unsigned total = (unsigned)j.Np * (unsigned)(j.K >> 3);
    const unsigned* __restrict__ amax = rb_tail(j);
    const long pl = (long)j.Np * 32, zs = (long)(j.K / 32) * 2 * pl;       // a piece plane of a chunk / a component's planes, fp16 elements
    unsigned u = (unsigned)lb * RB_WINO_PSPAN + threadIdx.x;
    const int s_ = (int)(u & 3);
    int c = (int)((u >> 2) / (unsigned)j.Np), n = (int)((u >> 2) - (unsigned)c * (unsigned)j.Np);
    for (int it = 0; it < RB_WINO_PSPAN / 256 && u < total; ++it, u += 256) {
        const int k0 = c * 32 + s_ * 8;
        const bool live = n < j.rows;
        float tp[9][8];
        if (!tr) {
            const float* __restrict__ p = j.src + (long)(live ? n : 0) * 9 * C + k0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 lo = *(const float4*)(p + (long)t * C), hi = *(const float4*)(p + (long)t * C + 4);
                tp[t][0] = lo.x; tp[t][1] = lo.y; tp[t][2] = lo.z; tp[t][3] = lo.w;
                tp[t][4] = hi.x; tp[t][5] = hi.y; tp[t][6] = hi.z; tp[t][7] = hi.w;
            }
        } else {
            const float* __restrict__ p = j.src + (long)k0 * 9 * C + (live ? n : 0);
#pragma unroll
            for (int q = 0; q < 8; ++q)
#pragma unroll
                for (int t = 0; t < 9; ++t) tp[8 - t][q] = p[((long)q * 9 + t) * C];       // (rotated by 180 degrees)
        }
        unsigned short* __restrict__ out = j.out + ws_plane_off<2>(c, n, s_, j.Np);
        static_for<0, A>([&](auto i_c) __attribute__((always_inline)) {
            constexpr int I = decltype(i_c)::value;
            float comp[A][8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float r[A];
                wino_filter_row<MT, I>([&](int r_, int s) { return tp[r_ * 3 + s][q]; }, r);
#pragma unroll
                for (int jj = 0; jj < A; ++jj) comp[jj][q] = live ? r[jj] : 0.f;       // (padding rows: +0, as the split of no source writes)
            }
#pragma unroll
            for (int jj = 0; jj < A; ++jj) {
                const int z = I * A + jj;
                const float sc = split2_scale(split2_exp_bits(amax[z]));
                ws_split_store<2>(out + z * zs, pl, comp[jj], sc);
            }
        });
        n += 64;
        if (n >= j.Np) { n -= j.Np; ++c; }
    }
}
__global__ __launch_bounds__(256) void k_rebuild_pieces_wino(const RebuildJob* __restrict__ wj, int n_wino) {
    const int b = (int)blockIdx.x;
    const int ji = rb_find(n_wino, b, [&](int m) { return (long)wj[m].pblk_begin; });
    const RebuildJob j = wj[ji];
    if (j.mt == 4) rb_pieces_wino<4>(j, b - j.pblk_begin);
    else rb_pieces_wino<2>(j, b - j.pblk_begin);
}
U2PL_API int u2pl_weight_rebuild2h_job_bytes(void) { return (int)sizeof(RebuildJob); }
// which: 0 -> float4 per block of the kinds 0 / 1 maxima pass and 16-byte segments per block of their pieces pass; 1 -> (o, 4 channels)
// units per block of the Winograd maxima pass; 2 -> (row, 8 k) units per block of the Winograd pieces pass
U2PL_API int u2pl_weight_rebuild2h_span(int which) { return which == 0 ? WS_AMAX_SPAN : which == 1 ? RB_WINO_MSPAN : which == 2 ? RB_WINO_PSPAN : 0; }
U2PL_API int u2pl_weight_rebuild2h_f32(const void* jobs, int n_flat, int n_wino, long seg_total, long amax_total, int wino_mblocks,
                                       int wino_pblocks, hipStream_t stream) {
    if (n_flat < 0 || n_wino < 0 || seg_total < 0 || amax_total < 0 || wino_mblocks < 0 || wino_pblocks < 0) return U2PL_EINVAL;
    if ((n_flat == 0) != (seg_total == 0) || (n_flat == 0) != (amax_total == 0)) return U2PL_EINVAL;
    if ((n_wino == 0) != (wino_mblocks == 0) || (n_wino == 0) != (wino_pblocks == 0)) return U2PL_EINVAL;
    if (n_flat + n_wino == 0) return 0;
    const RebuildJob* rj = (const RebuildJob*)jobs;
    const int flat_blocks = cdiv(amax_total, WS_AMAX_SPAN);
    U2PL_LAUNCH(k_rebuild_clear, dim3(cdiv(n_flat + n_wino, 256)), dim3(256), 0, stream, rj, n_flat + n_wino);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_rebuild_amax, dim3((unsigned)(flat_blocks + wino_mblocks)), dim3(256), 0, stream, rj, n_flat, n_wino, amax_total, flat_blocks);
    U2PL_LAUNCH_CHECK();
    if (n_flat) {
        U2PL_LAUNCH(k_rebuild_pieces_flat, dim3((unsigned)cdiv(seg_total, WS_AMAX_SPAN)), dim3(256), 0, stream, rj, n_flat, seg_total);
        U2PL_LAUNCH_CHECK();
    }
    if (n_wino) {
        U2PL_LAUNCH(k_rebuild_pieces_wino, dim3((unsigned)wino_pblocks), dim3(256), 0, stream, rj + n_flat, n_wino);
        U2PL_LAUNCH_CHECK();
    }
    return 0;
}
// max |x| of an activation operand [M][C] (row pitch ld floats) -> the amax object `out` (U2PL_AMAX_WORDS floats, common.h; NaN if
// any element is NaN); clear != 0: zeroed here first.  The A operand's scale of the *_wsh_* entry points.
__global__ void k_absmax_rows(const float* __restrict__ x, long ld, long M, int C4, unsigned* __restrict__ out) {
    const long total = M * C4;
    unsigned m = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C4;
        const int c = (int)(i - r * C4);
        m = amax_bits4(m, *(const float4*)(x + r * ld + c * 4));
    }
    amax_wave_publish(m, out);
}
U2PL_API int u2pl_amax_words(void) { return U2PL_AMAX_WORDS; }
U2PL_API int u2pl_absmax_f32(const float* x, long ld, long M, int C, float* out, int clear, hipStream_t stream) {
    if (M < 0 || C <= 0 || (C & 3) || (ld & 3)) return U2PL_EINVAL;
    if (clear) {            // (clear == 0: the caller hands a zeroed slot -- one fill for a whole pool of them)
        hipError_t e = hipMemsetAsync(out, 0, (size_t)U2PL_AMAX_WORDS * 4, stream);
        if (e != hipSuccess) return (int)e;
    }
    if (M == 0) return 0;
    U2PL_LAUNCH(k_absmax_rows, dim3(grid_for(M * (C / 4), 512, 2048)), dim3(512), 0, stream, x, ld, M, C / 4, (unsigned*)out);
    U2PL_LAUNCH_CHECK();
    return 0;
}
