// What contrast.hip (up to 32 classes, one word of class bits per pixel) and contrast_wide.hip (up to 255, word planes)
// both need, defined once: the ballot helpers and the block scan of the ordered compaction, and the device-resident bank.
// (The two files are separate objects, so the kernels here are `static`: each object carries its own copy.)
#pragma once
#include "common.h"

// ---- ordered compaction ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long lanemask_lt() {
    unsigned lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}
__device__ __forceinline__ unsigned wave_or_uniform(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return __builtin_amdgcn_readfirstlane(v);
}
// exclusive scan over blocks: one 256-thread block per (kind, class) row of blk (contiguous); counts[row] = the list length
static __global__ __launch_bounds__(256) void k_compact_scan(unsigned* __restrict__ blk, int nblk, unsigned* __restrict__ counts) {
    __shared__ unsigned wsum[4];
    unsigned* row = blk + (long)blockIdx.x * nblk;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned carry = 0;
    for (int base = 0; base < nblk; base += 256) {
        const int b = base + t;
        const unsigned v = b < nblk ? row[b] : 0;
        unsigned x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            unsigned u = __shfl_up(x, o, 64);
            if (lane >= o) x += u;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned wb = 0;
        for (int w2 = 0; w2 < wave; ++w2) wb += wsum[w2];
        const unsigned tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (b < nblk) row[b] = carry + wb + x - v;
        carry += tot;
        __syncthreads();
    }
    if (t == 0) counts[blockIdx.x] = carry;
}

// ---------------------------------------------------------------------------
// The memory bank as a device-resident object driven from the C header alone (SURVEY 8b `u2pl_bank_t`): the ring
// bookkeeping of dequeue_and_enqueue (utils.py:27-47) lives in a small DEVICE state array, so an enqueue needs neither the
// list lengths nor the ring heads on the host and can be issued before the step's host synchronisation.
//   state: int64 [C][5] = {row offset of the class's ring inside `storage`, cap, head, len, ptr}
//   init     caps (host) -> offsets = prefix sums, head = len = ptr = 0
//   enqueue  class c appends counts[c] rows at its tail, only the last `cap` of them if there are more (utils.py:38-41),
//            then the state advances: len' = min(len + n, cap), head' = (tail + n - len') mod cap, ptr' = cap once full,
//            else (ptr + n) mod cap (utils.py:36-45).  The new rows are rows[list[j]], j < counts[c], with class c's list
//            at idx + list_off[c] (a flat list buffer; contrast_wide.hip) or, list_off NULL, at idx + c * idx_stride (a
//            [C][stride] array; contrast.hip); idx NULL: row j of a class-major block starting at row_start[c].
// A host that wants the lengths (the reference samples torch.randint(len) on the CPU) copies the state back, or mirrors
// the same arithmetic from the counts it reads anyway (u2pl_amd.hipops.DeviceMemoryBank does the latter).
// One implementation for both class limits: the entry points differ in their limit (32 / 255) and their grids.
// ---------------------------------------------------------------------------
#define BANK_MAXC 255
struct BankCaps { long long cap[BANK_MAXC]; };
static __global__ void k_bank_init(long long* __restrict__ state, int C, BankCaps caps) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        long long off = 0;
        for (int c = 0; c < C; ++c) {
            state[5 * c + 0] = off; state[5 * c + 1] = caps.cap[c]; state[5 * c + 2] = 0; state[5 * c + 3] = 0; state[5 * c + 4] = 0;
            off += caps.cap[c];
        }
    }
}
static __global__ void k_bank_enqueue(const long long* __restrict__ state, float* __restrict__ storage, int D,
                                      const float* __restrict__ rows, long ld, const int* __restrict__ idx, long idx_stride,
                                      const long long* __restrict__ list_off, const long long* __restrict__ row_start,
                                      const unsigned* __restrict__ counts) {
    const int c = blockIdx.y;
    const long n_new = counts[c];
    if (n_new <= 0) return;
    const long off = state[5 * c + 0], cap = state[5 * c + 1], head = state[5 * c + 2], len = state[5 * c + 3];
    const long tail = (head + len) % cap;
    const long skip = n_new > cap ? n_new - cap : 0;       // more new rows than slots: only the last `cap` are kept
    const int D4 = D >> 2;
    const long total = (n_new - skip) * D4;
    const int* list = idx ? idx + (list_off ? (long)list_off[c] : (long)c * idx_stride) : nullptr;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long j = skip + t / D4;
        const int dd = (int)(t % D4);
        const long src = list ? (long)list[j] : (row_start ? row_start[c] : 0) + j;
        long slot = tail + j;
        slot = slot >= cap ? slot % cap : slot;
        ((float4*)storage)[(off + slot) * D4 + dd] = *(const float4*)(rows + src * ld + 4 * dd);
    }
}
static __global__ void k_bank_advance(long long* __restrict__ state, const unsigned* __restrict__ counts, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long n = counts[c];
    const long cap = state[5 * c + 1], head = state[5 * c + 2], len = state[5 * c + 3], ptr = state[5 * c + 4];
    const long tail = (head + len) % cap;
    const long nl = len + n < cap ? len + n : cap;
    const long new_tail = (tail + n) % cap;
    state[5 * c + 3] = nl;
    state[5 * c + 2] = ((new_tail - nl) % cap + cap) % cap;
    state[5 * c + 4] = nl >= cap ? cap : (ptr + n) % cap;
}
// the launches behind u2pl_bank_init[_wide] / u2pl_bank_enqueue[_wide]_f32; the entry points check their own arguments
// (maxc: 32 / 255) and choose the grids (blocks per class of the enqueue, threads of the one advance block >= C)
static inline int bank_init(long long* state, int C, int maxc, const long long* caps_host, hipStream_t stream) {
    if (C <= 0 || C > maxc || !state || !caps_host) return U2PL_EINVAL;
    BankCaps caps = {};
    for (int c = 0; c < C; ++c) {
        if (caps_host[c] <= 0) return U2PL_EINVAL;
        caps.cap[c] = caps_host[c];
    }
    U2PL_LAUNCH(k_bank_init, dim3(1), dim3(64), 0, stream, state, C, caps);
    U2PL_LAUNCH_CHECK();
    return 0;
}
static inline int bank_enqueue(long long* state, float* storage, int D, const float* rows, long ld, const int* idx,
                               long idx_stride, const long long* list_off, const long long* row_start,
                               const unsigned* counts, int C, int blocks_per_class, int advance_threads, hipStream_t stream) {
    U2PL_LAUNCH(k_bank_enqueue, dim3(blocks_per_class, C), dim3(256), 0, stream, state, storage, D, rows, ld, idx, idx_stride,
                list_off, row_start, counts);
    U2PL_LAUNCH_CHECK();
    U2PL_LAUNCH(k_bank_advance, dim3(1), dim3(advance_threads), 0, stream, state, counts, C);
    U2PL_LAUNCH_CHECK();
    return 0;
}
