// Counter-based normals and the fixed-order workgroup fold, shared by mppi.hip (perturbed plans) and particles.hip (particle rollouts).
#pragma once
#include <hip/hip_runtime.h>

#define MPPI_THREADS 256

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
// ---------------------------------------------------------------------------
struct Philox4 { unsigned w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// 53 random bits -> a uniform strictly inside (0, 1) (but for one rounding to 1 in 2^53 draws, which Box-Muller maps to eps = 0)
__device__ __forceinline__ double mppi_uniform(unsigned hi, unsigned lo) {
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * 0x1p-53;
}

// fold 256 per-thread values in halves (fixed order); the total is returned to every thread.  `red` is free again after the call.
__device__ __forceinline__ double mppi_fold_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = MPPI_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}
__device__ __forceinline__ int mppi_fold_count(int v, int* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = MPPI_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    const int s = red[0];
    __syncthreads();
    return s;
}
