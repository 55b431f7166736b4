// The weight operand planes: what the code that WRITES them (operands.hip) and the GEMM that copies them into its LDS tile
// (igemm_ws.hip) agree on.  A matrix [rows][K] (K % 32 == 0) is stored chunk-major as [K/32][NP pieces][Np][32 k] 16-bit elements,
// the four 16-byte k segments of a row XOR-swizzled by (row >> 2) & 3 (ws_plane_off in operands.hip; the A-side image of
// igemm_ws.hip's alds[]).
#pragma once
#include <stddef.h>
#include <type_traits>

// compile-time loop: f(integral_constant<int, B>) ... f(integral_constant<int, E - 1>) as straight-line code (the pinned main
// loop must not depend on the loop unroller's size budget: a rolled slot loop sends the register arrays to scratch)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

#define WS_ROW_B 64                      // bytes of one piece row of a 32-deep chunk (32 bf16 / fp16)
// rows of a split matrix are padded (zero rows) to the widest tile that reads them: no read ever leaves the allocation
__host__ __device__ static inline int ws_pad_rows(int rows) { return rows <= 128 ? 128 : (rows + 255) & ~255; }
// bytes of the two fp16 piece planes of `batch` matrices; their maxima (one uint32 per matrix) lie right behind
__host__ __device__ static inline size_t ws2_plane_bytes(int Np, int K, int batch) { return (size_t)batch * (K / 32) * 2 * Np * WS_ROW_B; }
