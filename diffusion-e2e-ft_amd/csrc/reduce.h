// reduce.h — the wave and block reduction pieces of the streaming kernels (wave64, blocks of whole waves), defined once.
// Every reduction built from them runs in a FIXED order: the xor butterfly inside a wave, the waves of a block left to right, and (in the kernels)
// the blocks' partials in index order.  No floating-point atomics: the same input gives the same bits on every run, rank and graph replay.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace e2eft {

// 64 lanes -> every lane holds the result.  Sums: float, double, uint32_t, int64_t, unsigned long long.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// min / max of unsigned integers (uint32_t, unsigned long long); the float overloads below drop NaNs like fminf / fmaxf
template <typename T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block (WAVES * 64 threads, all of them calling) sums of N columns: dst[i] = ((w0 + w1) + w2) + ... of column i, stored by thread i.
// One call per kernel (the LDS array is not fenced for a second use).
template <int N, int WAVES = 4> __device__ __forceinline__ void block_sums(double (&v)[N], double* dst) {
    static_assert(N <= WAVES * 64, "one thread per column");
    __shared__ double red[WAVES][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) red[wave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += red[w][threadIdx.x];
        dst[threadIdx.x] = t;
    }
}

// block (256 threads) min / max -> out[0], out[1] by thread 0
__device__ __forceinline__ void block_minmax(float mn, float mx, float* out) {
    __shared__ float red[2][4];
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = mn; red[1][wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        out[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

}  // namespace e2eft
