// Winograd F(m x m, 3 x 3) transform matrices (m = 2, 4) as straight-line fp32 code, shared by the transform kernels of wino.hip
// and the operand rebuild of operands.hip (which recomputes G g G^T from the taps: same code, same bits under -ffp-contract=off).
#pragma once

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4mul(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
// a + s*b written as separate multiply and add (-ffp-contract=off keeps it that way)
__device__ __forceinline__ float4 f4axpy(float4 a, float s, float4 b) { return f4add(a, f4mul(s, b)); }

// B^T d for one 6-vector / 4-vector of float4 (applied to columns, then to rows)
template <int MT> struct WinoT;
template <> struct WinoT<4> {
    static constexpr int A = 6;
    __device__ static __forceinline__ void bt(const float4 (&d)[6], float4 (&r)[6]) {
        const float4 p = f4axpy(d[4], -4.f, d[2]);   // d4 - 4 d2
        const float4 q = f4axpy(d[3], -4.f, d[1]);   // d3 - 4 d1
        const float4 s = f4sub(d[4], d[2]);          // d4 - d2
        const float4 t = f4mul(2.f, f4sub(d[3], d[1]));
        r[0] = f4add(f4axpy(f4mul(4.f, d[0]), -5.f, d[2]), d[4]);
        r[1] = f4add(p, q);
        r[2] = f4sub(p, q);
        r[3] = f4add(s, t);
        r[4] = f4sub(s, t);
        r[5] = f4add(f4axpy(f4mul(4.f, d[1]), -5.f, d[3]), d[5]);
    }
    // A^T m : 6 -> 4
    __device__ static __forceinline__ void at(const float4 (&m)[6], float4 (&y)[4]) {
        const float4 s12 = f4add(m[1], m[2]), d12 = f4sub(m[1], m[2]);
        const float4 s34 = f4add(m[3], m[4]), d34 = f4sub(m[3], m[4]);
        y[0] = f4add(f4add(m[0], s12), s34);
        y[1] = f4axpy(d12, 2.f, d34);
        y[2] = f4axpy(s12, 4.f, s34);
        y[3] = f4add(f4axpy(d12, 8.f, d34), m[5]);
    }
    // A v : 4 -> 6 (transpose of the output transform: weight-gradient side)
    __device__ static __forceinline__ void av(const float4 (&v)[4], float4 (&r)[6]) {
        const float4 e = f4add(v[0], v[2]), o = f4add(v[1], v[3]);
        const float4 e4 = f4axpy(v[0], 4.f, v[2]), o4 = f4axpy(f4mul(2.f, v[1]), 8.f, v[3]);
        r[0] = v[0];
        r[1] = f4add(e, o);
        r[2] = f4sub(e, o);
        r[3] = f4add(e4, o4);
        r[4] = f4sub(e4, o4);
        r[5] = v[3];
    }
    // G^T v : 6 -> 3 (scalar)
    __device__ static __forceinline__ void gt(const float (&v)[6], float (&r)[3]) {
        const float s12 = v[1] + v[2], s34 = v[3] + v[4];
        r[0] = v[0] * 0.25f - s12 * (1.f / 6.f) + s34 * (1.f / 24.f);
        r[1] = (v[2] - v[1]) * (1.f / 6.f) + (v[3] - v[4]) * (1.f / 12.f);
        r[2] = (s34 - s12) * (1.f / 6.f) + v[5];
    }
    // G g : 3 -> 6 (scalar)
    __device__ static __forceinline__ void gg(const float (&g)[3], float (&r)[6]) {
        const float a = (g[0] + g[2]) * (-1.f / 6.f), b = g[1] * (1.f / 6.f);
        const float c = g[0] * (1.f / 24.f) + g[2] * (1.f / 6.f), e = g[1] * (1.f / 12.f);
        r[0] = g[0] * 0.25f;
        r[1] = a - b;
        r[2] = a + b;
        r[3] = c + e;
        r[4] = c - e;
        r[5] = g[2];
    }
};
template <> struct WinoT<2> {
    static constexpr int A = 4;
    __device__ static __forceinline__ void bt(const float4 (&d)[4], float4 (&r)[4]) {
        r[0] = f4sub(d[0], d[2]);
        r[1] = f4add(d[1], d[2]);
        r[2] = f4sub(d[2], d[1]);
        r[3] = f4sub(d[1], d[3]);
    }
    __device__ static __forceinline__ void at(const float4 (&m)[4], float4 (&y)[2]) {
        y[0] = f4add(f4add(m[0], m[1]), m[2]);
        y[1] = f4sub(f4sub(m[1], m[2]), m[3]);
    }
    __device__ static __forceinline__ void av(const float4 (&v)[2], float4 (&r)[4]) {
        r[0] = v[0];
        r[1] = f4add(v[0], v[1]);
        r[2] = f4sub(v[0], v[1]);
        r[3] = f4mul(-1.f, v[1]);
    }
    __device__ static __forceinline__ void gt(const float (&v)[4], float (&r)[3]) {
        r[0] = v[0] + 0.5f * (v[1] + v[2]);
        r[1] = 0.5f * (v[1] - v[2]);
        r[2] = 0.5f * (v[1] + v[2]) + v[3];
    }
    __device__ static __forceinline__ void gg(const float (&g)[3], float (&r)[4]) {
        r[0] = g[0];
        r[1] = 0.5f * ((g[0] + g[2]) + g[1]);
        r[2] = 0.5f * ((g[0] + g[2]) - g[1]);
        r[3] = g[2];
    }
};
// Row I of U = G g G^T of ONE filter, g(r, s) = tap(r, s): WinoT::gg on the three columns (only row I of each result is kept -- the
// rest is dead code to the compiler), then WinoT::gg on that row: the operations of wino_weight_one (wino.hip) for that row, in
// its order, so the operand rebuild of operands.hip, which recomputes the components from the taps a row at a time, gets the
// bits that kernel writes (no contraction: -ffp-contract=off).
template <int MT, int I, class Tap>
__device__ __forceinline__ void wino_filter_row(Tap&& tap, float (&r)[WinoT<MT>::A]) {
    constexpr int A = WinoT<MT>::A;
    float t[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        float col[3] = {tap(0, s), tap(1, s), tap(2, s)}, q[A];
        WinoT<MT>::gg(col, q);
        t[s] = q[I];
    }
    WinoT<MT>::gg(t, r);
}
// row(I, r) for I = 0 .. A - 1
template <int MT, int I = 0, class Tap, class Row>
__device__ __forceinline__ void wino_filter_rows(Tap&& tap, Row&& row) {
    if constexpr (I < WinoT<MT>::A) {
        float r[WinoT<MT>::A];
        wino_filter_row<MT, I>(tap, r);
        row(I, r);
        wino_filter_rows<MT, I + 1>(tap, row);
    }
}
