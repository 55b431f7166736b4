// Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018: Algorithm 1 on the softmax errors of section 3) and the
// segmented stable radix sort it needs -- the library's first full sort (csrc/select.hip selects order statistics and
// never orders).  DESIGN section 3.17.
//
// Stages, each an entry point of its own (include/u2pl_hip.h), run per CHUNK of classes so that the sort buffers stay
// bounded at 150 .. 255 classes:
//   1 errors    k_lv_errors + k_lv_counts   one pass over the logits: a 30-bit sortable key and a payload (pixel index, the
//                                           foreground bit in bit 31) per (class of the chunk, pixel); per-class foreground
//                                           counts G and the valid count, as per-block integer partials summed by a second launch
//   2 sort      u2pl_segsort_u32            least-significant-digit radix sort, one segment per class, 8-bit digits:
//                                           k_ss_hist -> k_ss_rowscan -> k_ss_scatter per pass, ping-pong buffers
//   3 gradient  k_lv_tilefg -> k_ss_rowscan -> k_lv_grad   reduce-then-scan of the foreground bit along the sorted order,
//                                           the closed-form Lovasz gradient, slab partials of m * g, g stored through the
//                                           permutation into the [C][P] plane the backward reads
//   4 finish    k_lv_finish                 slabs summed in order (double), class count, loss -> out3 = {loss, 1/n, n}
//   5 backward  k_lv_bwd                    per pixel: softmax again, g[:, i] through the softmax Jacobian -> dz
//
// KEY.  m = |[y == c] - p_c| lies in [0, 1], so its bit pattern is monotone as an unsigned and at most 0x3F800000.  The
// sort is ascending on  key = 0x3F800000 - bits(m)  (descending m), which keeps 30 significant bits; an ignored pixel gets
// LV_IGN_KEY = 0x3FFFFFFF, strictly above the key 0x3F800000 of a valid pixel with m == 0.  The sort is stable and the
// errors stage emits pixels in ascending index, so ties come out in ascending flat pixel index: the order of the contract.
//
// DIGIT WIDTH.  30 bits = 8 + 8 + 8 + 6: four passes.  10-bit digits would make it three, but the per-tile histogram table and
// the scan between the launches grow fourfold (1024 counters per 2048-element tile: 2 bytes of table per element and pass against
// the 16 bytes of keys and payloads a pass moves), and the wave-level digit match below costs one ballot per digit bit.
//
// ORDER WITHOUT WAITING.  A wave owns a TILE of SS_TILE consecutive elements and walks it 64 at a time; the lanes that share a
// digit find each other with one ballot per digit bit, the rank inside the round is a popcount of the lanes below, and a
// per-wave LDS counter carries the rank from round to round.  No lane ever waits for another wave: the prefix over the tiles
// is a launch of its own (k_ss_rowscan, one wave per row, 64 tiles per step): no decoupled look-back, no spin flags.
// No atomics anywhere; every output word is written exactly once, so workspaces may arrive NaN-filled.
//
// SUMS.  Per lane a sequential fp32 sum of m * g over the rounds of its tile, a fixed butterfly over the 64 lanes -> one fp32
// slab per (class, tile); k_lv_finish adds the slabs of a class in double (lane l takes tiles l, l + 64, ..., then the same
// butterfly), the classes upward in double.  The same bits on every run.
#include "common.h"
#include "u2pl_hip.h"

#define SS_TILE 2048          // elements per wave tile (32 rounds of 64)
#define SS_WAVES 4            // waves (tiles) per block
#define SS_BINS 256           // 8-bit digits
#define LV_ONE_BITS 0x3F800000u
#define LV_IGN_KEY 0x3FFFFFFFu
#define LV_ALIGN 256

// ------------------------------------------------------------------------------------------------ wave helpers
// per-wave LDS counters: read by every lane, then written by one lane per digit, round after round.  A wave's LDS instructions
// execute in program order, so no barrier is needed between them; volatile keeps the compiler from caching or reordering the
// accesses, and the explicit address space keeps them ds_read / ds_write (a volatile generic pointer compiles to flat accesses)
typedef volatile __attribute__((address_space(3))) unsigned lds_u32;
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// the lanes (among the active ones) whose 8-bit digit equals this lane's: one ballot per digit bit
__device__ __forceinline__ unsigned long long match_digit(unsigned d, bool active) {
    unsigned long long m = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(active && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}
__device__ __forceinline__ unsigned wave_incl_scan_u(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ int seg_length(const int* __restrict__ seg_len, int seg, int n) {
    if (!seg_len) return n;
    const int l = seg_len[seg];
    return l < 0 ? 0 : (l > n ? n : l);
}

// ------------------------------------------------------------------------------------------------ segmented radix sort
// hist[(seg * 256 + digit) * tiles + tile] = elements of the tile with that digit (0 for a tile past the segment's length)
__global__ __launch_bounds__(256) void k_ss_hist(const unsigned* __restrict__ keys, long stride,
                                                 const int* __restrict__ seg_len, int n, int shift, unsigned mask,
                                                 int tiles, unsigned* __restrict__ hist) {
    __shared__ unsigned s_cnt[SS_WAVES][SS_BINS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * SS_WAVES + w, seg = blockIdx.y;
    if (tile >= tiles) return;                       // whole wave; the kernel has no block-wide barrier
    const int len = seg_length(seg_len, seg, n);
    lds_u32* c = (lds_u32*)&s_cnt[w][0];
#pragma unroll
    for (int k = 0; k < SS_BINS / 64; ++k) c[lane + 64 * k] = 0u;
    __builtin_amdgcn_wave_barrier();
    const unsigned* __restrict__ k = keys + (long)seg * stride;
    const long base = (long)tile * SS_TILE;
    for (int r = 0; r < SS_TILE / 64; ++r) {
        const long i = base + r * 64 + lane;
        if (base + r * 64 >= len) break;             // wave-uniform
        const bool act = i < len;
        const unsigned d = act ? ((k[i] >> shift) & mask) : 0u;
        const unsigned long long m = match_digit(d, act);
        const unsigned old = act ? c[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (act && (m & lanes_below(lane)) == 0ull) c[d] = old + (unsigned)__popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int q = 0; q < SS_BINS / 64; ++q) {
        const int d = lane + 64 * q;
        hist[((long)seg * SS_BINS + d) * tiles + tile] = c[d];
    }
}

// rows[row][0 .. len) -> its exclusive prefix sums in place, tot[row] = the row's sum.  One wave per row, 64 entries a step.
__global__ __launch_bounds__(256) void k_ss_rowscan(unsigned* __restrict__ rows, long nrows, int len,
                                                    unsigned* __restrict__ tot) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * SS_WAVES + w;
    if (row >= nrows) return;
    unsigned* __restrict__ p = rows + row * len;
    unsigned carry = 0u;
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        const unsigned v = t < len ? p[t] : 0u;
        const unsigned inc = wave_incl_scan_u(v, lane);
        if (t < len) p[t] = carry + inc - v;
        carry += (unsigned)__shfl((int)inc, 63, 64);
    }
    if (lane == 0) tot[row] = carry;
}

// stable scatter of one tile: destination = segment base + (elements of the segment with a smaller digit) + (elements with this
// digit in earlier tiles) + (elements with this digit earlier in this tile)
__global__ __launch_bounds__(256) void k_ss_scatter(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                    unsigned* __restrict__ kout, unsigned* __restrict__ vout, long stride,
                                                    const int* __restrict__ seg_len, int n, int shift, unsigned mask,
                                                    int tiles, const unsigned* __restrict__ hist,
                                                    const unsigned* __restrict__ tot) {
    __shared__ unsigned s_cnt[SS_WAVES][SS_BINS];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * SS_WAVES + w, seg = blockIdx.y;
    if (tile >= tiles) return;
    const int len = seg_length(seg_len, seg, n);
    const long base = (long)tile * SS_TILE;
    if (base >= len) return;
    lds_u32* c = (lds_u32*)&s_cnt[w][0];
    {   // exclusive prefix of the 256 digit totals: lane l owns digits 4 l .. 4 l + 3
        const unsigned* __restrict__ t = tot + (long)seg * SS_BINS + 4 * lane;
        const unsigned t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
        const unsigned sum = t0 + t1 + t2 + t3;
        unsigned ex = wave_incl_scan_u(sum, lane) - sum;
        const unsigned* __restrict__ h = hist + ((long)seg * SS_BINS + 4 * lane) * tiles + tile;
        c[4 * lane + 0] = ex + h[0];
        ex += t0;
        c[4 * lane + 1] = ex + h[tiles];
        ex += t1;
        c[4 * lane + 2] = ex + h[2L * tiles];
        ex += t2;
        c[4 * lane + 3] = ex + h[3L * tiles];
    }
    __builtin_amdgcn_wave_barrier();
    const long so = (long)seg * stride;
    for (int r = 0; r < SS_TILE / 64; ++r) {
        const long i = base + r * 64 + lane;
        if (base + r * 64 >= len) break;
        const bool act = i < len;
        const unsigned key = act ? kin[so + i] : 0u;
        const unsigned val = act ? vin[so + i] : 0u;
        const unsigned d = (key >> shift) & mask;
        const unsigned long long m = match_digit(d, act);
        const unsigned rank = (unsigned)__popcll(m & lanes_below(lane));
        const unsigned old = act ? c[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (act) {
            const unsigned pos = old + rank;
            if (pos < (unsigned)len) {               // always true for a consistent histogram; keeps a store inside the segment
                kout[so + pos] = key;
                vout[so + pos] = val;
            }
            if (rank == 0u) c[d] = old + (unsigned)__popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

static inline int ss_tiles(long n) { return (int)((n + SS_TILE - 1) / SS_TILE); }
static inline int ss_passes(int bits) { return (bits + 7) / 8; }
static inline size_t lv_up(size_t b) { return (b + LV_ALIGN - 1) / LV_ALIGN * LV_ALIGN; }

U2PL_API int u2pl_segsort_passes(int bits) { return bits < 1 || bits > 32 ? 0 : ss_passes(bits); }
U2PL_API int u2pl_segsort_tile(void) { return SS_TILE; }
U2PL_API size_t u2pl_segsort_ws_bytes(int nseg, long n) {
    if (nseg < 1 || nseg > 65535 || n < 1 || n >= (1L << 31)) return 0;
    return lv_up((size_t)nseg * SS_BINS * ss_tiles(n) * sizeof(unsigned)) + lv_up((size_t)nseg * SS_BINS * sizeof(unsigned));
}

static int segsort_run(unsigned* k0, unsigned* v0, unsigned* k1, unsigned* v1, void* ws, int nseg, long n, long stride,
                       const int* seg_len, int bits, hipStream_t stream) {
    const int tiles = ss_tiles(n), passes = ss_passes(bits);
    unsigned* hist = (unsigned*)ws;
    unsigned* tot = (unsigned*)((char*)ws + lv_up((size_t)nseg * SS_BINS * tiles * sizeof(unsigned)));
    const dim3 grid(cdiv(tiles, SS_WAVES), nseg);
    const long rows = (long)nseg * SS_BINS;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p, width = bits - shift < 8 ? bits - shift : 8;
        const unsigned mask = (1u << width) - 1u;
        U2PL_LAUNCH(k_ss_hist, grid, dim3(256), 0, stream, (const unsigned*)k0, stride, seg_len, (int)n, shift, mask, tiles, hist);
        U2PL_LAUNCH_CHECK();
        U2PL_LAUNCH(k_ss_rowscan, dim3(cdiv(rows, SS_WAVES)), dim3(256), 0, stream, hist, rows, tiles, tot);
        U2PL_LAUNCH_CHECK();
        U2PL_LAUNCH(k_ss_scatter, grid, dim3(256), 0, stream, (const unsigned*)k0, (const unsigned*)v0, k1, v1, stride, seg_len,
                    (int)n, shift, mask, tiles, (const unsigned*)hist, (const unsigned*)tot);
        U2PL_LAUNCH_CHECK();
        unsigned* t = k0; k0 = k1; k1 = t;
        t = v0; v0 = v1; v1 = t;
    }
    return 0;
}

U2PL_API int u2pl_segsort_u32(unsigned* keys, unsigned* vals, unsigned* keys_alt, unsigned* vals_alt, void* ws, int nseg,
                              long n, const int* seg_len_dev, int bits, hipStream_t stream) {
    if (!keys || !vals || !keys_alt || !vals_alt || !ws) return U2PL_EINVAL;
    if (nseg < 1 || nseg > 65535 || n < 1 || n >= (1L << 31) || bits < 1 || bits > 32) return U2PL_EINVAL;
    return segsort_run(keys, vals, keys_alt, vals_alt, ws, nseg, n, n, seg_len_dev, bits, stream);
}

// ------------------------------------------------------------------------------------------------ Lovasz workspace
struct LvLayout {
    int cap, tiles, nblk, nchunks;
    size_t keys0, vals0, keys1, vals1, sortws, tilefg, tiletot, part, counts, slabs, total;
};
static bool lv_layout(long P, int C, int class_chunk, LvLayout* L) {
    if (C < 2 || C > 255 || P <= 0 || P >= (1L << 31) || class_chunk < 1) return false;
    L->cap = class_chunk < C ? class_chunk : C;
    L->nchunks = (C + L->cap - 1) / L->cap;
    L->tiles = ss_tiles(P);
    L->nblk = (int)((P + 255) / 256);
    size_t o = 0;
    const size_t plane = lv_up((size_t)L->cap * P * sizeof(unsigned));
    L->keys0 = o; o += plane;
    L->vals0 = o; o += plane;
    L->keys1 = o; o += plane;
    L->vals1 = o; o += plane;
    L->sortws = o; o += u2pl_segsort_ws_bytes(L->cap, P);
    L->tilefg = o; o += lv_up((size_t)L->cap * L->tiles * sizeof(unsigned));
    L->tiletot = o; o += lv_up((size_t)L->cap * sizeof(unsigned));
    L->part = o; o += lv_up((size_t)(L->cap + 1) * L->nblk * sizeof(unsigned));
    L->counts = o; o += lv_up((size_t)(C + 1) * sizeof(unsigned));
    L->slabs = o; o += lv_up((size_t)C * L->tiles * sizeof(float));
    L->total = o;
    return true;
}

U2PL_API size_t u2pl_lovasz_workspace_bytes(long P, int C, int class_chunk) {
    LvLayout L;
    return lv_layout(P, C, class_chunk, &L) ? L.total : 0;
}
U2PL_API int u2pl_lovasz_default_chunk(void) { return 32; }

U2PL_API int u2pl_lovasz_plan(long P, int C, int class_chunk, long long* out) {
    LvLayout L;
    if (!out || !lv_layout(P, C, class_chunk, &L)) return U2PL_EINVAL;
    out[0] = L.nchunks;
    out[1] = L.cap;
    out[2] = SS_TILE;
    out[3] = L.tiles;                                  // tiles per segment: sort and gradient stages alike
    out[4] = L.nblk;                                   // errors: blocks of 256 pixels
    out[5] = L.cap + 1;                                // errors: blocks of the count reduction (one per class + the valid count)
    out[6] = ss_passes(30);                            // sort passes
    out[7] = cdiv(L.tiles, SS_WAVES);                  // sort / gradient: grid.x (grid.y = classes of the chunk)
    out[8] = cdiv((long)L.cap * SS_BINS, SS_WAVES);    // sort: blocks of the row scan
    out[9] = cdiv(L.cap, SS_WAVES);                    // gradient: blocks of the row scan
    out[10] = (long long)L.keys0;
    out[11] = (long long)L.vals0;
    out[12] = (long long)L.keys1;
    out[13] = (long long)L.vals1;
    out[14] = (long long)L.sortws;
    out[15] = (long long)L.tilefg;
    out[16] = (long long)L.part;
    out[17] = (long long)L.counts;
    out[18] = (long long)L.slabs;
    out[19] = (long long)L.total;
    return 0;
}

// ------------------------------------------------------------------------------------------------ stage 1: errors
__global__ __launch_bounds__(256) void k_lv_errors(const float* __restrict__ z, const long long* __restrict__ target,
                                                   int ignore, int C, long HW, long P, int c0, int cc,
                                                   unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                   unsigned* __restrict__ part, int nblk) {
    __shared__ unsigned s_cnt[SS_WAVES][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const bool act = p < P;
    long long t = ignore;
    if (act) t = target[p];
    const bool valid = act && t != ignore;
    const float* __restrict__ b = z;
    float mx = 0.f, s = 1.f;
    if (valid) {
        const long n = p / HW, q = p % HW;
        b = z + n * C * HW + q;
        mx = b[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, b[(long)c * HW]);
        s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(b[(long)c * HW] - mx);
    }
    for (int cl = 0; cl < cc; ++cl) {
        const int c = c0 + cl;
        const bool fg = valid && t == c;
        unsigned key = LV_IGN_KEY;
        if (valid) {
            const float pr = expf(b[(long)c * HW] - mx) / s;
            const float m = fg ? 1.0f - pr : pr;
            key = LV_ONE_BITS - __float_as_uint(m);
        }
        if (act) {
            keys[(long)cl * P + p] = key;
            vals[(long)cl * P + p] = (unsigned)p | (fg ? 0x80000000u : 0u);
        }
        const unsigned long long bal = __ballot(fg);
        if (lane == 0) s_cnt[w][cl] = (unsigned)__popcll(bal);
    }
    {
        const unsigned long long bal = __ballot(valid);
        if (lane == 0) s_cnt[w][cc] = (unsigned)__popcll(bal);
    }
    __syncthreads();
    if ((int)threadIdx.x <= cc)
        part[(long)threadIdx.x * nblk + blockIdx.x] =
            (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
}

// counts[c0 + b] = G of class c0 + b (b < cc); counts[C] = valid pixels (block cc)
__global__ __launch_bounds__(256) void k_lv_counts(const unsigned* __restrict__ part, int nblk, int c0, int cc, int C,
                                                   unsigned* __restrict__ counts) {
    __shared__ unsigned s[SS_WAVES];
    const unsigned* __restrict__ row = part + (long)blockIdx.x * nblk;
    unsigned v = 0u;
    for (int i = threadIdx.x; i < nblk; i += 256) v += row[i];
    v = wave_sum_u(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) counts[(int)blockIdx.x < cc ? c0 + (int)blockIdx.x : C] = (s[0] + s[1]) + (s[2] + s[3]);
}

U2PL_API int u2pl_lovasz_errors_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H,
                                    int W, int c0, void* ws, int class_chunk, hipStream_t stream) {
    LvLayout L;
    if (!logits_nchw || !target || !ws || N < 1 || H < 1 || W < 1) return U2PL_EINVAL;
    const long P = (long)N * H * W;
    if (!lv_layout(P, C, class_chunk, &L) || c0 < 0 || c0 >= C || c0 % L.cap != 0) return U2PL_EINVAL;
    const int cc = C - c0 < L.cap ? C - c0 : L.cap;
    char* w8 = (char*)ws;
    U2PL_LAUNCH(k_lv_errors, dim3(L.nblk), dim3(256), 0, stream, logits_nchw, target, ignore, C, (long)H * W, P, c0, cc,
                (unsigned*)(w8 + L.keys0), (unsigned*)(w8 + L.vals0), (unsigned*)(w8 + L.part), L.nblk);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_lv_counts, dim3(cc + 1), dim3(256), 0, stream, (const unsigned*)(w8 + L.part), L.nblk, c0, cc, C,
                (unsigned*)(w8 + L.counts));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// stage 2 on the workspace's own buffers: the cc segments of the chunk, 30 key bits, result back in keys0 / vals0
U2PL_API int u2pl_lovasz_sort(long P, int C, int c0, void* ws, int class_chunk, hipStream_t stream) {
    LvLayout L;
    if (!ws || !lv_layout(P, C, class_chunk, &L) || c0 < 0 || c0 >= C || c0 % L.cap != 0) return U2PL_EINVAL;
    const int cc = C - c0 < L.cap ? C - c0 : L.cap;
    char* w8 = (char*)ws;
    return segsort_run((unsigned*)(w8 + L.keys0), (unsigned*)(w8 + L.vals0), (unsigned*)(w8 + L.keys1),
                       (unsigned*)(w8 + L.vals1), w8 + L.sortws, cc, P, P, nullptr, 30, stream);
}

// ------------------------------------------------------------------------------------------------ stage 3: gradient
__global__ __launch_bounds__(256) void k_lv_tilefg(const unsigned* __restrict__ vals, long P, int tiles,
                                                   unsigned* __restrict__ tilefg) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * SS_WAVES + w, cl = blockIdx.y;
    if (tile >= tiles) return;
    const unsigned* __restrict__ v = vals + (long)cl * P;
    const long base = (long)tile * SS_TILE;
    unsigned cnt = 0u;
    for (int r = 0; r < SS_TILE / 64; ++r) {
        const long i = base + r * 64 + lane;
        if (base + r * 64 >= P) break;
        const bool fg = i < P && (v[i] >> 31);
        cnt += (unsigned)__popcll(__ballot(fg));
    }
    if (lane == 0) tilefg[(long)cl * tiles + tile] = cnt;
}

// position j (1-based) of the sorted order of class c, F = foreground among the first j, G = foreground of the class:
//   I = G - F, U = G + (j - F);  foreground: g = 1 / U;  background, G > 0: g = I / ((U - 1) U);  G == 0: g_1 = 1, else 0
// (the closed form of J_j - J_{j-1}: a difference of two numbers near 1 would lose every bit in the tail of a long list)
__global__ __launch_bounds__(256) void k_lv_grad(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                 long P, int tiles, const unsigned* __restrict__ tilefg,
                                                 const unsigned* __restrict__ counts, int c0, int present_only,
                                                 float* __restrict__ gplane, float* __restrict__ slabs) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * SS_WAVES + w, cl = blockIdx.y;
    if (tile >= tiles) return;
    const int c = c0 + cl;
    const unsigned G = counts[c];
    const bool live = G > 0u || !present_only;
    const unsigned* __restrict__ k = keys + (long)cl * P;
    const unsigned* __restrict__ v = vals + (long)cl * P;
    float* __restrict__ gp = gplane + (long)c * P;
    const long base = (long)tile * SS_TILE;
    unsigned carry = tilefg[(long)cl * tiles + tile];
    float acc = 0.f;
    for (int r = 0; r < SS_TILE / 64; ++r) {
        const long i = base + r * 64 + lane;
        if (base + r * 64 >= P) break;
        const bool act = i < P;
        const unsigned key = act ? k[i] : LV_IGN_KEY;
        const unsigned val = act ? v[i] : 0u;
        const bool valid = key != LV_IGN_KEY;
        const bool fg = valid && (val >> 31);
        const unsigned long long bal = __ballot(fg);
        const unsigned F = carry + (unsigned)__popcll(bal & (lanes_below(lane) | (1ull << lane)));
        carry += (unsigned)__popcll(bal);
        if (act) {
            float g = 0.f;
            if (valid && live) {
                const long long j = i + 1;
                const long long U = (long long)G + (j - (long long)F);
                if (fg) g = (float)(1.0 / (double)U);
                else if (G > 0u) g = (float)((double)((long long)G - (long long)F) / ((double)(U - 1) * (double)U));
                else g = j == 1 ? 1.0f : 0.0f;
                acc += __uint_as_float(LV_ONE_BITS - key) * g;
            }
            const long pix = val & 0x7fffffffu;
            if (pix < P) gp[pix] = g;                // always true for a payload of stage 1; keeps the store inside the plane
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) slabs[(long)c * tiles + tile] = acc;
}

U2PL_API int u2pl_lovasz_grad_f32(long P, int C, int c0, int present_only, void* ws, int class_chunk, float* gplane,
                                  hipStream_t stream) {
    LvLayout L;
    if (!ws || !gplane || !lv_layout(P, C, class_chunk, &L) || c0 < 0 || c0 >= C || c0 % L.cap != 0) return U2PL_EINVAL;
    const int cc = C - c0 < L.cap ? C - c0 : L.cap;
    char* w8 = (char*)ws;
    const dim3 grid(cdiv(L.tiles, SS_WAVES), cc);
    unsigned* tilefg = (unsigned*)(w8 + L.tilefg);
    U2PL_LAUNCH(k_lv_tilefg, grid, dim3(256), 0, stream, (const unsigned*)(w8 + L.vals0), P, L.tiles, tilefg);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_ss_rowscan, dim3(cdiv(cc, SS_WAVES)), dim3(256), 0, stream, tilefg, (long)cc, L.tiles,
                (unsigned*)(w8 + L.tiletot));
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_lv_grad, grid, dim3(256), 0, stream, (const unsigned*)(w8 + L.keys0), (const unsigned*)(w8 + L.vals0), P,
                L.tiles, (const unsigned*)tilefg, (const unsigned*)(w8 + L.counts), c0, present_only, gplane,
                (float*)(w8 + L.slabs));
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ stage 4: finish
// out3 = {loss, 1 / n_classes (0 when no class counts), n_classes}
__global__ __launch_bounds__(256) void k_lv_finish(const float* __restrict__ slabs, const unsigned* __restrict__ counts,
                                                   int C, int tiles, int present_only, float* __restrict__ out3) {
    __shared__ double s_loss[256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = w; c < C; c += SS_WAVES) {
        const float* __restrict__ row = slabs + (long)c * tiles;
        double a = 0.0;
        for (int t = lane; t < tiles; t += 64) a += (double)row[t];
        a = wave_sum_d(a);
        if (lane == 0) s_loss[c] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        int n = 0;
        for (int c = 0; c < C; ++c)
            if (!present_only || counts[c] > 0u) { sum += s_loss[c]; ++n; }
        out3[0] = n > 0 ? (float)(sum / (double)n) : 0.0f;
        out3[1] = n > 0 ? (float)(1.0 / (double)n) : 0.0f;
        out3[2] = (float)n;
    }
}

U2PL_API int u2pl_lovasz_finish_f32(long P, int C, int present_only, const void* ws, int class_chunk, float* out3,
                                    hipStream_t stream) {
    LvLayout L;
    if (!ws || !out3 || !lv_layout(P, C, class_chunk, &L)) return U2PL_EINVAL;
    const char* w8 = (const char*)ws;
    U2PL_LAUNCH(k_lv_finish, dim3(1), dim3(256), 0, stream, (const float*)(w8 + L.slabs), (const unsigned*)(w8 + L.counts),
                C, L.tiles, present_only, out3);
    U2PL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ stage 5: backward
// a_c = -/+ g[c][i] k  (minus where c == t), k = out3[1] gout gmul;  dz_c = p_c (a_c - sum_k a_k p_k);  0 on ignored pixels
__global__ __launch_bounds__(256) void k_lv_bwd(const float* __restrict__ z, const long long* __restrict__ target,
                                                int ignore, int C, long HW, long P, const float* __restrict__ gplane,
                                                const float* __restrict__ out3, const float* __restrict__ gout,
                                                float gmul, float* __restrict__ grad) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float kf = out3[1] * (gout ? *gout : 1.0f) * gmul;
    const long n = p / HW, q = p % HW;
    const float* __restrict__ b = z + n * C * HW + q;
    float* __restrict__ g = grad + n * C * HW + q;
    const long long t = target[p];
    if (t == ignore) {
        for (int c = 0; c < C; ++c) g[(long)c * HW] = 0.f;
        return;
    }
    float mx = b[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, b[(long)c * HW]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(b[(long)c * HW] - mx);
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
        const float pr = expf(b[(long)c * HW] - mx) / s;
        const float a = gplane[(long)c * P + p] * kf;
        dot += (c == t ? -a : a) * pr;
    }
    for (int c = 0; c < C; ++c) {
        const float pr = expf(b[(long)c * HW] - mx) / s;
        const float a = gplane[(long)c * P + p] * kf;
        g[(long)c * HW] = pr * ((c == t ? -a : a) - dot);
    }
}

U2PL_API int u2pl_lovasz_bwd_f32(const float* logits_nchw, const long long* target, int ignore, int N, int C, int H, int W,
                                 const float* gplane, const float* out3_dev, const float* gout_dev, float gmul, float* grad,
                                 hipStream_t stream) {
    if (!logits_nchw || !target || !gplane || !out3_dev || !grad || N < 1 || H < 1 || W < 1) return U2PL_EINVAL;
    const long P = (long)N * H * W;
    if (C < 2 || C > 255 || P >= (1L << 31)) return U2PL_EINVAL;
    U2PL_LAUNCH(k_lv_bwd, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, logits_nchw, target, ignore, C,
                (long)H * W, P, gplane, out3_dev, gout_dev, gmul, grad);
    U2PL_LAUNCH_CHECK();
    return 0;
}
