// Contrastive path for MORE THAN 32 CLASSES (up to U2PL_WIDE_MAXC = 255: label value 255 is the ignore value).
// contrast.hip keeps a pixel's multi-hot label in one 32-bit word and sizes everything after it by MAXC = 32; here the
// masks are WORD PLANES: lbits / abits / lowbits / nbits are u32 [W][P] with W = ceil(C / 32), plane g holds classes
// 32 g .. 32 g + 31 (a plane is what the 32-class kernels consume).  Lists, counts and prototypes stay class-indexed.
// The pixel lists are stored FLAT: one int32 buffer that holds the lists of all (kind, class) pairs back to back, in
// (kind, class) order, each list in row-major pixel order (torch boolean-mask order); offsets int64 [3][C] gives every
// list's first element.  (A [3][C][P] array is 268 MB at C = 150 and 769^2 crops; the flat buffer is the sum of the list
// lengths.)  The caller reads the list lengths back -- the step's one host synchronisation, which it needs anyway for the
// random-index bounds -- and allocates the flat buffer from them, so the list write follows that read.
// Reference: u2pl/utils/loss_helper.py:80-154 (masks, lists, prototypes), u2pl/utils/utils.py:27-47 (the bank).
// Everything here is integer or ordered double-precision arithmetic: the same bits on every run.
#include <stdint.h>
#include "common.h"
#include "class_lists.h"
#include "u2pl_hip.h"

#define WIDE_MAXC 255
#define WIDE_LDS_BUDGET (48 * 1024)   // bytes of staged probability rows + counters a classify block may hold

static inline int wide_words(int C) { return (C + 31) / 32; }
// pixels per block of the classify / write kernels (one per thread), by the class count: the largest of 256 / 128 / 64
// whose probability rows (PIX * C floats) and 3 C counters fit the LDS budget, (PIX + 3) * C * 4 <= 49152: 256 pixels up
// to C = 47, 128 up to 93, 64 up to 183; C >= 184 does not fit at 64 pixels and reads its rows from global memory
// (staged == 0; u2pl_contra_wide_staged reports it)
static inline int wide_pix(int C, int* staged) {
    for (int pix = 256; pix >= 64; pix >>= 1)
        if (((long)pix * C + 3L * C) * 4 <= WIDE_LDS_BUDGET) {
            if (staged) *staged = 1;
            return pix;
        }
    if (staged) *staged = 0;
    return 64;
}
U2PL_API int u2pl_wide_words(int C) { return C > 0 && C <= WIDE_MAXC ? wide_words(C) : 0; }
U2PL_API int u2pl_contra_wide_block_pixels(int C) { return C > 0 && C <= WIDE_MAXC ? wide_pix(C, nullptr) : 0; }
U2PL_API int u2pl_contra_wide_staged(int C) {
    int staged = 0;
    if (C > 0 && C <= WIDE_MAXC) wide_pix(C, &staged);
    return staged;
}
U2PL_API size_t u2pl_contra_wide_workspace_bytes(long P, int C) {
    if (P <= 0 || C <= 0 || C > WIDE_MAXC) return 0;
    return (size_t)cdiv(P, wide_pix(C, nullptr)) * 3 * C * sizeof(unsigned);
}

// ---------------------------------------------------------------------------
// Phase 1a (loss_helper.py:103-141), the arithmetic of k_contra_classify_rows: per pixel, for every SET label bit i
// (whichever plane it lies in) the rank of prob_i in the pixel's whole row of C probabilities (descending; ties towards the
// lower class index: pj == pi && j < i), then
//   abits  : (prob_i > thr_p) & label_i & low_mask        lowbits: label_i & low_mask
//   nbits  : (prob_i < thr_n) & label_i & high_mask & rank_i in [low_rank, high_rank)   (unlabeled images only, Q2)
// and per block of PIX pixels the member counts of every (kind, class) list: blk[(kind * C + c) * nblk + b].
// STAGED: the probabilities are contiguous [pixel][C] rows, a block's rows are one contiguous span staged into LDS with
// 16-byte loads; otherwise a thread reads its own row through the strides.
// ---------------------------------------------------------------------------
template <bool STAGED>
__global__ __launch_bounds__(256) void k_wide_classify(
    const float* __restrict__ prob, long sn, long sc, long sp, const unsigned* __restrict__ lbits,
    const float* __restrict__ low_mask, const float* __restrict__ high_mask, int N2, int num_labeled, int C, int W, long hw,
    float thr_p, float thr_n, int low_rank, int high_rank, unsigned* __restrict__ abits, unsigned* __restrict__ lowbits,
    unsigned* __restrict__ nbits, unsigned* __restrict__ blk, int nblk) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int PIX = blockDim.x, t = threadIdx.x;
    unsigned* cnt = (unsigned*)(sm + (STAGED ? (long)PIX * C : 0));      // [3][C]
    for (int i = t; i < 3 * C; i += PIX) cnt[i] = 0;
    const long total = (long)N2 * hw;
    const long p0 = blockIdx.x * (long)PIX, p = p0 + t;
    if (STAGED) {
        const long npx = min((long)PIX, total - p0);
        const int nfl = (int)(npx * C);
        const float* src = prob + p0 * C;      // 16-byte aligned: p0 is a multiple of 64 (host checks the base)
        for (int i = t * 4; i < nfl; i += PIX * 4) {
            if (i + 3 < nfl) *(float4*)(sm + i) = *(const float4*)(src + i);
            else for (int k = i; k < nfl; ++k) sm[k] = src[k];
        }
    }
    __syncthreads();
    if (p < total) {
        const long n = p / hw, q = p % hw;
        const bool lo = low_mask[p] != 0.f, hi = high_mask[p] != 0.f;
        const float* b = STAGED ? sm + (long)t * C : prob + n * sn + q * sp;
        const long st = STAGED ? 1 : sc;
        const bool unlabeled = n >= num_labeled;
        for (int g = 0; g < W; ++g) {
            const int left = C - 32 * g;           // classes of this plane
            const unsigned lb = lbits[(long)g * total + p] & (left >= 32 ? 0xffffffffu : (1u << left) - 1u);
            unsigned a = 0, l = 0, ng = 0;
            for (unsigned x = lb; x; x &= x - 1u) {
                const int bit = __ffs(x) - 1, i = 32 * g + bit;
                const float pi = b[i * st];
                int rank = 0;
                for (int j = 0; j < C; ++j) {
                    const float pj = b[j * st];
                    rank += (pj > pi) || (pj == pi && j < i);
                }
                const bool cmask = unlabeled && rank >= low_rank && rank < high_rank;
                if (lo) {
                    l |= 1u << bit;
                    atomicAdd(&cnt[1 * C + i], 1u);
                    if (pi > thr_p) { a |= 1u << bit; atomicAdd(&cnt[0 * C + i], 1u); }
                }
                if (hi && pi < thr_n && cmask) { ng |= 1u << bit; atomicAdd(&cnt[2 * C + i], 1u); }
            }
            abits[(long)g * total + p] = a;
            lowbits[(long)g * total + p] = l;
            nbits[(long)g * total + p] = ng;
        }
    }
    __syncthreads();
    for (int i = t; i < 3 * C; i += PIX) blk[(long)i * nblk + blockIdx.x] = cnt[i];
}

// offsets[kind][c] = first element of list (kind, c) in the flat buffer: the running sum of the 3 C list lengths in
// (kind, class) order (<= 765 terms: one thread)
__global__ void k_wide_offsets(const unsigned* __restrict__ counts, int n, long long* __restrict__ offsets) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < n; ++i) { offsets[i] = run; run += counts[i]; }
    }
}

U2PL_API int u2pl_contra_classify_wide(const float* prob, long sn, long sc, long sp, const unsigned* lbits,
                                       const float* low_mask, const float* high_mask, int N2, int num_labeled, int C,
                                       int h, int w, float thr_p, float thr_n, int low_rank, int high_rank,
                                       unsigned* abits, unsigned* lowbits, unsigned* nbits, void* workspace,
                                       unsigned* counts, long long* offsets, hipStream_t stream) {
    const long total = (long)N2 * h * w;
    if (C <= 0 || C > WIDE_MAXC || total <= 0 || total >= (1L << 31) || !workspace || !counts || !offsets) return U2PL_EINVAL;
    int staged = 0;
    const int pix = wide_pix(C, &staged), W = wide_words(C);
    const int nblk = cdiv(total, pix);
    unsigned* blk = (unsigned*)workspace;
    const bool rows = sc == 1 && sp == C && sn == (long)h * w * C && ((uintptr_t)prob & 15) == 0;
    if (staged && rows)
        U2PL_LAUNCH(k_wide_classify<true>, dim3(nblk), dim3(pix), ((size_t)pix * C + 3 * C) * sizeof(float), stream, prob, sn,
                    sc, sp, lbits, low_mask, high_mask, N2, num_labeled, C, W, (long)h * w, thr_p, thr_n, low_rank,
                    high_rank, abits, lowbits, nbits, blk, nblk);
    else
        U2PL_LAUNCH(k_wide_classify<false>, dim3(nblk), dim3(pix), (size_t)3 * C * sizeof(float), stream, prob, sn, sc, sp,
                    lbits, low_mask, high_mask, N2, num_labeled, C, W, (long)h * w, thr_p, thr_n, low_rank, high_rank,
                    abits, lowbits, nbits, blk, nblk);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_compact_scan, dim3(3 * C), dim3(256), 0, stream, blk, nblk, counts);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_wide_offsets, dim3(1), dim3(64), 0, stream, counts, 3 * C, offsets);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// Phase 1b: ordered compaction into the flat buffer (k_compact_write's scheme, one plane per grid.y, all three kinds --
// the low-valid list is what the prototypes sum over).  A block's offset inside list (kind, c) is the scanned per-block
// count, inside the block the waves' ballots: integer only, row-major pixel order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wide_write(const unsigned* __restrict__ b0, const unsigned* __restrict__ b1,
                                                    const unsigned* __restrict__ b2, long P, const unsigned* __restrict__ blk,
                                                    int nblk, int C, const long long* __restrict__ offsets,
                                                    int* __restrict__ idx, long idx_len) {
    __shared__ long long wcnt[4][3 * 32];    // per-wave counts -> exclusive positions in the flat buffer
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, nw = blockDim.x >> 6, g = blockIdx.y;
    const long p = blockIdx.x * (long)blockDim.x + t;
    unsigned v[3];
    v[0] = p < P ? b0[(long)g * P + p] : 0;
    v[1] = p < P ? b1[(long)g * P + p] : 0;
    v[2] = p < P ? b2[(long)g * P + p] : 0;
    for (int i = t; i < 4 * 3 * 32; i += blockDim.x) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    unsigned pres[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pres[k] = wave_or_uniform(v[k]);
        for (unsigned x = pres[k]; x; x &= x - 1u) {
            const int c = __ffs(x) - 1;
            const unsigned long long m = __ballot((v[k] >> c) & 1u);
            if (lane == 0) wcnt[wave][k * 32 + c] = __popcll(m);
        }
    }
    __syncthreads();
    for (int i = t; i < 3 * 32; i += blockDim.x) {
        const int k = i >> 5, cls = 32 * g + (i & 31);
        if (cls < C) {
            long long run = offsets[k * C + cls] + (long long)blk[((long)k * C + cls) * nblk + blockIdx.x];
            for (int w2 = 0; w2 < nw; ++w2) {
                const long long tmp = wcnt[w2][i];
                wcnt[w2][i] = run;
                run += tmp;
            }
        }
    }
    __syncthreads();
    const unsigned long long lt = lanemask_lt();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (unsigned x = pres[k]; x; x &= x - 1u) {
            const int c = __ffs(x) - 1;
            const bool on = (v[k] >> c) & 1u;
            const unsigned long long m = __ballot(on);
            if (on) {
                const long long pos = wcnt[wave][k * 32 + c] + __popcll(m & lt);
                if (pos < idx_len) idx[pos] = (int)p;      // (always true for bit planes the counts were taken from)
            }
        }
}
// workspace: what u2pl_contra_classify_wide left (the scanned per-block counts); offsets: the same call's; idx: int32
// [idx_len], idx_len >= the sum of all 3 C list lengths
U2PL_API int u2pl_compact_lists_wide(const unsigned* abits, const unsigned* lowbits, const unsigned* nbits, long P, int C,
                                     const void* workspace, const long long* offsets, int* idx, long idx_len,
                                     hipStream_t stream) {
    if (C <= 0 || C > WIDE_MAXC || P <= 0 || P >= (1L << 31) || !workspace || !offsets) return U2PL_EINVAL;
    if (idx_len <= 0) return 0;
    if (!idx) return U2PL_EINVAL;
    const int pix = wide_pix(C, nullptr), nblk = cdiv(P, pix);
    U2PL_LAUNCH(k_wide_write, dim3(nblk, wide_words(C)), dim3(pix), 0, stream, abits, lowbits, nbits, P,
                (const unsigned*)workspace, nblk, C, offsets, idx, idx_len);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------
// Phase 1c: class prototypes = mean of the rep_teacher rows over the class's low-valid list (loss_helper.py:119-123).
// grid (C, D / 64), 1024 threads = 64 channels x 16 row groups: group r adds members r, r + 16, ... in list order in
// double precision, the 16 sums are added in a fixed order and the mean is rounded once.  A class without members: NaN
// (torch.mean of an empty selection).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_wide_proto(const float* __restrict__ rows, long ld, int D, const int* __restrict__ idx,
                                                     const long long* __restrict__ offsets, const unsigned* __restrict__ counts,
                                                     int C, float* __restrict__ proto) {
    __shared__ double sh[16][64];
    const int c = blockIdx.x, cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int d = blockIdx.y * 64 + cl;
    const unsigned n = counts[1 * C + c];
    double acc = 0.0;
    if (d < D && n) {
        const int* list = idx + offsets[1 * C + c];
        for (unsigned i = rg; i < n; i += 16) acc += (double)rows[(long)list[i] * ld + d];
    }
    sh[rg][cl] = acc;
    __syncthreads();
    if (rg == 0 && d < D) {
        double tsum = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) tsum += sh[q][cl];
        proto[(long)c * D + d] = n ? (float)(tsum / (double)n) : __uint_as_float(0x7fc00000u);
    }
}
U2PL_API int u2pl_class_prototypes_wide(const float* rows, long ld, int D, const int* idx, const long long* offsets,
                                        const unsigned* counts, int C, float* proto, hipStream_t stream) {
    if (C <= 0 || C > WIDE_MAXC || D <= 0 || !rows || !offsets || !counts || !proto) return U2PL_EINVAL;
    U2PL_LAUNCH(k_wide_proto, dim3(C, cdiv(D, 64)), dim3(1024), 0, stream, rows, ld, D, idx, offsets, counts, C, proto);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// The device-resident bank (class_lists.h) for up to 255 classes, lists in the flat buffer: class c's list starts at
// idx + list_off_dev[c].
U2PL_API int u2pl_bank_init_wide(long long* state, int C, const long long* caps_host, hipStream_t stream) {
    return bank_init(state, C, WIDE_MAXC, caps_host, stream);
}
U2PL_API int u2pl_bank_enqueue_wide_f32(long long* state, float* storage, int D, const float* rows, long ld, const int* idx,
                                        const long long* list_off_dev, const long long* row_start_dev,
                                        const unsigned* counts_dev, int C, hipStream_t stream) {
    if (D % 4 || C <= 0 || C > WIDE_MAXC || !state || !storage || !rows || !counts_dev || (idx && !list_off_dev)) return U2PL_EINVAL;
    return bank_enqueue(state, storage, D, rows, ld, idx, 0, list_off_dev, row_start_dev, counts_dev, C, 64, 256, stream);
}
