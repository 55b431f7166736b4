// Yardstick of tools/bench_bn_stream.py: a float4 streaming kernel with NR 16-byte read streams and NW 16-byte write streams per
// element and nothing else (one add per extra read), what a BatchNorm pass of the same streams could reach at best on this chip.
// Built as a small shared object by the tool:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC stream_yardstick.hip
// Each thread keeps 4 elements x NR loads in flight; the grid is one resident set of blocks (8 per CU).
#include <hip/hip_runtime.h>

struct Streams { const float4* r[4]; float4* w[2]; };

template <int NR, int NW>
__global__ __launch_bounds__(256) void k_stream(Streams s, long n4) {
    // a block takes chunks of 4 x 256 consecutive float4 (16 KB per stream), chunk blockIdx.x and then every gridDim.x-th: the
    // grid sweeps every stream front to back
    const long chunk = (long)gridDim.x * 1024;
    float4 keep = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i = blockIdx.x * 1024L + threadIdx.x; i < n4; i += chunk) {
        if (i + 768 < n4) {
            float4 v[4][NR];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < NR; ++k) v[u][k] = s.r[k][i + u * 256];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float4 a = v[u][0];
#pragma unroll
                for (int k = 1; k < NR; ++k) { a.x += v[u][k].x; a.y += v[u][k].y; a.z += v[u][k].z; a.w += v[u][k].w; }
#pragma unroll
                for (int k = 0; k < NW; ++k) s.w[k][i + u * 256] = a;
                if (NW == 0) { keep.x += a.x; keep.y += a.y; keep.z += a.z; keep.w += a.w; }
            }
        } else {
            for (long j = i; j < n4; j += 256) {
                float4 a = s.r[0][j];
#pragma unroll
                for (int k = 1; k < NR; ++k) { const float4 b = s.r[k][j]; a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
#pragma unroll
                for (int k = 0; k < NW; ++k) s.w[k][j] = a;
                if (NW == 0) { keep.x += a.x; keep.y += a.y; keep.z += a.z; keep.w += a.w; }
            }
        }
    }
    // a pure read: the sums must be live, and are never this value
    if (NW == 0 && keep.x == 123.456f && s.w[0]) s.w[0][0] = keep;
}

template <int NR, int NW>
static int launch(const Streams& s, long n4, hipStream_t st) {
    static int resident = 0;      // blocks of this instantiation that fit on the chip at once
    if (!resident) {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_stream<NR, NW>, 256, 0) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return 1002;
        resident = per_cu * cus;
    }
    long g = (n4 + 4 * 256 - 1) / (4 * 256);
    if (g > resident) g = resident;
    if (g < 1) g = 1;
    hipLaunchKernelGGL((k_stream<NR, NW>), dim3((unsigned)g), dim3(256), 0, st, s, n4);
    return (int)hipGetLastError();
}

// nr in 1..4 read streams, nw in 0..2 write streams, n4 float4 elements per stream
extern "C" __attribute__((visibility("default"))) int stream_yardstick(int nr, int nw, const void* r0, const void* r1, const void* r2,
                                                                       const void* r3, void* w0, void* w1, long n4, void* stream) {
    Streams s = {{(const float4*)r0, (const float4*)r1, (const float4*)r2, (const float4*)r3}, {(float4*)w0, (float4*)w1}};
    hipStream_t st = (hipStream_t)stream;
    switch (nr * 10 + nw) {
        case 10: return launch<1, 0>(s, n4, st);
        case 11: return launch<1, 1>(s, n4, st);
        case 20: return launch<2, 0>(s, n4, st);
        case 21: return launch<2, 1>(s, n4, st);
        case 22: return launch<2, 2>(s, n4, st);
        case 30: return launch<3, 0>(s, n4, st);
        case 31: return launch<3, 1>(s, n4, st);
        case 32: return launch<3, 2>(s, n4, st);
        case 42: return launch<4, 2>(s, n4, st);
        default: return 1001;
    }
}
