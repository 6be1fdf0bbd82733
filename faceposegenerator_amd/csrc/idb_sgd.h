// The arithmetic of the clipped SGD step, once, as device functions: the kernels of idb_sgd.hip (lists and tables of tensors) and
// the two of idb_head.hip (one tensor, the norm met again inside the step's launch) are made of these, so their bits agree.
// A tensor of n elements is cut into sgd_parts(n) parts; part b is elements 256 b + t + 256 parts i, t the thread, i = 0, 1, ...
#pragma once
#include "idb_f32mma.h"

namespace {

constexpr int SGD_PARTS = 1024;

__host__ __device__ __forceinline__ int sgd_parts(long long n) {
    const long long want = (n + 4095) / 4096;
    return want < SGD_PARTS ? (int)want : SGD_PARTS;
}

// the sum of squares of part blockIdx.x of g in double, then the fixed block sum; every thread gets it
__device__ __forceinline__ double sgd_sqsum_part(const float* g, long long n, int parts, double* lds4) {
    double s = 0.0;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += parts * 256LL) {
        const double v = (double)g[i];
        s += v * v;
    }
    return block_sum_d(s, lds4);
}

// a tensor's partials strided over the 256 threads and met in the fixed block sum
__device__ __forceinline__ double sgd_sum_parts(const double* part, int parts, double* lds4) {
    double s = 0.0;
    for (int i = threadIdx.x; i < parts; i += 256) s += part[i];
    return block_sum_d(s, lds4);
}

__device__ __forceinline__ double sgd_clip_coef(double max_norm, double norm) {
    const double q = max_norm / (norm + 1e-6);
    return q < 1.0 ? q : 1.0;
}

// part blockIdx.x of the step, evaluated in double per element; each fp32 state (the momentum buffer, the weight) is rounded once
__device__ __forceinline__ void sgd_step_part(float* w, const float* g, float* buf, long long n, int parts, double coef, double lr,
                                              double momentum, double wd, int first) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += parts * 256LL) {
        const double d = coef * (double)g[i] + wd * (double)w[i];
        const float b = (float)(first ? d : momentum * (double)buf[i] + d);
        buf[i] = b;
        w[i] = (float)((double)w[i] - lr * (double)b);
    }
}

}  // namespace
