// The embedding stage of the face-recognition backbone in training (ID-Booth's FR_training/backbones/iresnet.py: bn2 -> flatten ->
// dropout -> fc -> features, then the loop's F.normalize), forward and backward.  fp32 state, the three [b] x [hw ch] x [n] products on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32), every
// statistic and reduction in double in an order the shapes alone decide, no floating-point atomics.
//   x is NHWC [b][hw][ch]; with k = p ch + c the flattened row of sample i is x[i K + k], K = hw ch: the device order of fc.weight's
//   columns, of the keep-mask and of every [b][K] array here.
//   forward   stats     shifted sums of x per channel over slices of the b hw rows (the shift is row 0: a constant channel sums to 0)
//             bn2       the slices in ascending order: mean, 1 / sqrt(var + eps), the running statistics, and the fp32 affine
//                       sc = gamma invstd, sh = beta - mean gamma invstd that the products apply while loading
//             fc        z = d W^T, d = fma(x, sc, sh) * keep / (1 - p) formed in the A-operand load (never written), split over K
//             merge     the K slices in ascending order in double, plus the bias, rounded once
//             features  BatchNorm1d statistics over the batch per feature, running statistics
//             rows      one wave per sample: f, its norm, the unit row
//   backward  rows      g_f = (g - e <e, g>) / norm per sample (after the loop's second projection when `renormalised`)
//             features  BatchNorm1d backward per feature: g_z, d features.bias, d fc.bias
//             dgrad     g_d = g_z W with the mask applied in the epilogue: g_y, and per (row tile, column) sums of g_y and g_y xhat
//             bn2       those partials in ascending order: d bn2.weight, d bn2.bias, the two means
//             dx        gamma invstd (g_y - mean - xhat mean(g_y xhat)), optional
//             wgrad     dW = g_z^T d with d recomputed in the load path, all of the batch inside one workgroup
// The tile helpers are idb_f32mma.h's, instantiated at 4 column groups; the loop's clipped SGD step is idb_sgd.hip.
#include "idb_f32mma.h"
#include <math.h>

namespace {

constexpr int TAIL_MAX_B = 1024, TAIL_MAX_CH = 2048, TAIL_MAX_HW = 64, TAIL_MAX_N = 1024;
constexpr int TAIL_FILL = 256;     // workgroups that fill the machine
constexpr int TAIL_MAX_SLICES = 64;

template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <> __device__ __forceinline__ f32x4 load4<_Float16>(const _Float16* p) {
    const f16x4 v = *(const f16x4*)p;
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <> __device__ __forceinline__ f32x4 load4<__bf16>(const __bf16* p) {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// the dropped activation: fma(x, sc, sh), one rounding, times keep / (1 - p), one more (exact where 1 / (1 - p) is 1)
__device__ __forceinline__ f32x4 dropped4(f32x4 x, f32x4 sc, f32x4 sh, uint32_t keep4, float inv_keep) {
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = __builtin_fmaf(x[e], sc[e], sh[e]);
        d[e] = ((keep4 >> (8 * e)) & 0xffu) ? a * inv_keep : 0.f;
    }
    return d;
}

// ---- forward: bn2 statistics ------------------------------------------------------------------------------------------------------
// grid (ch / 64, slices): thread (g = t >> 6, c = t & 63) sums x - x[0][c] and its square over rows first + g, first + g + 4, ... of its
// slice in double; the four are added in order.  part: double [slices][2][ch].
template <typename T>
__global__ __launch_bounds__(256) void tail_stats_kernel(const T* __restrict__ x, int rows, int ch, int per, double* __restrict__ part) {
    __shared__ double l1[256], l2[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int first = blockIdx.y * per, last = min(rows, first + per);
    const double x0 = (double)(float)x[c];
    double s1 = 0.0, s2 = 0.0;
    for (int r = first + g; r < last; r += 4) {
        const double v = (double)(float)x[(long long)r * ch + c] - x0;
        s1 += v;
        s2 += v * v;
    }
    l1[threadIdx.x] = s1, l2[threadIdx.x] = s2;
    __syncthreads();
    if (g == 0) {
        const int t = threadIdx.x;
        part[((long long)blockIdx.y * 2 + 0) * ch + c] = ((l1[t] + l1[t + 64]) + l1[t + 128]) + l1[t + 192];
        part[((long long)blockIdx.y * 2 + 1) * ch + c] = ((l2[t] + l2[t + 64]) + l2[t + 128]) + l2[t + 192];
    }
}

// one thread per channel.  training: the slices in ascending order -> mean, biased variance, running statistics (the unbiased variance
// for running_var); else the running statistics as they are.  stat: double [2][ch] mean, invstd.  affine: fp32 [2][ch] sc, sh.
// flags[0]: a statistic is not finite.  flags[1]: a variance of exactly 0 with eps = 0.
template <typename T>
__global__ __launch_bounds__(64) void tail_bn2_kernel(const T* __restrict__ x, const double* __restrict__ part, int slices, int rows, int ch,
                                                      int training, double eps, double momentum, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                      double* __restrict__ stat, float* __restrict__ affine, int32_t* __restrict__ flags) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    double mean, var;
    if (training) {
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < slices; ++s) {
            s1 += part[((long long)s * 2 + 0) * ch + c];
            s2 += part[((long long)s * 2 + 1) * ch + c];
        }
        const double n = (double)rows, m = s1 / n;
        mean = (double)(float)x[c] + m;
        var = (s2 - s1 * m) / n;
        if (var < 0.0) var = 0.0;
        rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
        rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * (var * (n / (n - 1.0))));
    } else {
        mean = (double)rmean[c];
        var = (double)rvar[c];
    }
    const double invstd = 1.0 / sqrt(var + eps);
    stat[c] = mean;
    stat[ch + c] = invstd;
    const double sc = (double)gamma[c] * invstd;
    affine[c] = (float)sc;
    affine[ch + c] = (float)((double)beta[c] - mean * sc);
    if (!(fabs(mean) <= 1.7e308) || !(var <= 1.7e308)) flags[0] = 1;      // also true for NaN
    else if (var + eps == 0.0) flags[1] = 1;
}

// ---- forward: fc ------------------------------------------------------------------------------------------------------------------
// grid (column tiles of n, row tiles of b, K slices).  part: fp32 [slices][b][n].
template <typename T>
__global__ __launch_bounds__(256) void tail_fc_kernel(const T* __restrict__ x, const uint8_t* __restrict__ keep, const float* __restrict__ affine,
                                                      const float* __restrict__ w, int B, int ch, int K, int N, int per, float inv_keep,
                                                      float* __restrict__ part) {
    __shared__ float sA[TM * LDR], sB[TM * LDR];
    const int n0 = blockIdx.x * TM, m0 = blockIdx.y * TM;
    const int steps = K / TK, s0 = blockIdx.z * per, s1 = min(steps, s0 + per);
    const int kc = (threadIdx.x & 7) * 4, rr = threadIdx.x >> 3;
    f32x16 acc[4];
    zero_acc<4>(acc);
    f32x4 va[4], vb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + kc, c = k % ch;
        const f32x4 sc = *(const f32x4*)(affine + c), sh = *(const f32x4*)(affine + ch + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + rr + 32 * i, col = n0 + rr + 32 * i;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (row < B) {
                const long long o = (long long)row * K + k;
                a = dropped4(load4<T>(x + o), sc, sh, keep ? *(const uint32_t*)(keep + o) : 0x01010101u, inv_keep);
            }
            if (col < N) b = *(const f32x4*)(w + (long long)col * K + k);
            va[i] = a, vb[i] = b;
        }
    };
    fetch(s0 * TK);
    for (int s = s0; s < s1; ++s) {
        __syncthreads();
        stash_rows<4>(sA, va);
        stash_rows<4>(sB, vb);
        __syncthreads();
        if (s + 1 < s1) fetch((s + 1) * TK);
        mma_stage<true, true, 4>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = n0 + wv * 32 + r;
    if (col < N) {
        float* out = part + (long long)blockIdx.z * B * N;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + tile_row(t, e, h);
                if (row < B) out[(long long)row * N + col] = acc[t][e];
            }
    }
}

__global__ __launch_bounds__(256) void tail_merge_kernel(const float* __restrict__ part, int slices, int B, int N, const float* __restrict__ bias,
                                                         float* __restrict__ z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * N) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double)part[(long long)k * B * N + i];
    z[i] = (float)(s + (double)bias[i % N]);
}

// ---- forward: features ------------------------------------------------------------------------------------------------------------
// grid n / 64: thread (g, c) takes rows g, g + 4, ... of column c, shifted by row 0; the four in order; thread (0, c) finishes.
__global__ __launch_bounds__(256) void tail_feat_stats_kernel(const float* __restrict__ z, int B, int N, int training, double eps, double momentum,
                                                              float* __restrict__ rmean, float* __restrict__ rvar, double* __restrict__ stat,
                                                              int32_t* __restrict__ flags) {
    __shared__ double l1[256], l2[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, t = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    const double z0 = (double)z[c];
    if (training)
        for (int r = g; r < B; r += 4) {
            const double v = (double)z[(long long)r * N + c] - z0;
            s1 += v;
            s2 += v * v;
        }
    l1[t] = s1, l2[t] = s2;
    __syncthreads();
    if (g != 0) return;
    double mean, var;
    if (training) {
        s1 = ((l1[t] + l1[t + 64]) + l1[t + 128]) + l1[t + 192];
        s2 = ((l2[t] + l2[t + 64]) + l2[t + 128]) + l2[t + 192];
        const double n = (double)B, m = s1 / n;
        mean = z0 + m;
        var = (s2 - s1 * m) / n;
        if (var < 0.0) var = 0.0;
        rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
        rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * (var * (n / (n - 1.0))));
    } else {
        mean = (double)rmean[c];
        var = (double)rvar[c];
    }
    stat[c] = mean;
    stat[N + c] = 1.0 / sqrt(var + eps);
    if (!(fabs(mean) <= 1.7e308) || !(var <= 1.7e308)) flags[0] = 1;
    else if (var + eps == 0.0) flags[2] = 1;
}

// one wave per sample: f = (z - mean) invstd w + bias in double, rounded once; norm = |f| of the rounded row in double;
// emb = f / max(norm, 1e-12), rounded once
__global__ __launch_bounds__(256) void tail_rows_kernel(const float* __restrict__ z, const double* __restrict__ stat, const float* __restrict__ fw,
                                                        const float* __restrict__ fb, int B, int N, float* __restrict__ f, float* __restrict__ emb,
                                                        double* __restrict__ norms, int32_t* __restrict__ flags) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (row >= B) return;
    float fv[16];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = l + 64 * i;
        fv[i] = 0.f;
        if (j < N) {
            fv[i] = (float)(((double)z[(long long)row * N + j] - stat[j]) * stat[N + j] * (double)fw[j] + (double)fb[j]);
            f[(long long)row * N + j] = fv[i];
            ss += (double)fv[i] * (double)fv[i];
        }
    }
    const double norm = sqrt(wave_sum_d(ss)), den = norm > 1e-12 ? norm : 1e-12;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = l + 64 * i;
        if (j < N) emb[(long long)row * N + j] = (float)((double)fv[i] / den);
    }
    if (l == 0) {
        norms[row] = norm;
        if (!(norm <= 1.7e308)) flags[0] = 1;              // eval mode has no statistics launch: a NaN or infinity in x shows here
    }
}

// ---- backward: rows ---------------------------------------------------------------------------------------------------------------
// one wave per sample.  renormalised: g <- (g - y <y, g>) / |e| with e the stored unit row and y = e / |e| (the loop's
// `torch.div(features, torch.norm(features, 2, 1, True))`).  Then g_f = (g - u <u, g>) / max(norm, 1e-12) with u = f / max(norm, 1e-12).
__global__ __launch_bounds__(256) void tail_bwd_rows_kernel(const float* __restrict__ g, const float* __restrict__ emb, const float* __restrict__ f,
                                                            const double* __restrict__ norms, int B, int N, int renorm, double* __restrict__ gf) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (row >= B) return;
    const long long o = (long long)row * N;
    const double den = norms[row] > 1e-12 ? norms[row] : 1e-12;
    double ne = 1.0, egn = 0.0;                            // |e| and <e, g> / |e|
    if (renorm) {
        double ee = 0.0, eg = 0.0;
        for (int j = l; j < N; j += 64) {
            const double e = (double)emb[o + j];
            ee += e * e;
            eg += e * (double)g[o + j];
        }
        ne = sqrt(wave_sum_d(ee));
        egn = wave_sum_d(eg) / ne;
    }
    // the cotangent after the optional second projection, recomputed where it is needed instead of kept in registers
    auto g1 = [&](int j) { return renorm ? ((double)g[o + j] - (double)emb[o + j] / ne * egn) / ne : (double)g[o + j]; };
    double ug = 0.0;
    for (int j = l; j < N; j += 64) ug += (double)f[o + j] / den * g1(j);
    ug = wave_sum_d(ug);
    for (int j = l; j < N; j += 64) gf[o + j] = (g1(j) - (double)f[o + j] / den * ug) / den;
}

// ---- backward: features (BatchNorm1d with a frozen weight) ------------------------------------------------------------------------
// grid n / 64, thread (g, c) rows g, g + 4, ...: S1 = sum g_f, S2 = sum g_f zhat; g_z = w invstd (g_f - S1 / b - zhat S2 / b), fp32;
// d features.bias = S1, d fc.bias = sum of the rounded g_z.
__global__ __launch_bounds__(256) void tail_bwd_feat_kernel(const double* __restrict__ gf, const float* __restrict__ z, const double* __restrict__ stat,
                                                            const float* __restrict__ fw, int B, int N, float* __restrict__ gz,
                                                            float* __restrict__ d_feat_b, float* __restrict__ d_fc_b) {
    __shared__ double l1[256], l2[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, t = threadIdx.x, c0 = threadIdx.x & 63;
    const double mean = stat[c], invstd = stat[N + c];
    double s1 = 0.0, s2 = 0.0;
    for (int r = g; r < B; r += 4) {
        const double v = gf[(long long)r * N + c];
        s1 += v;
        s2 += v * (((double)z[(long long)r * N + c] - mean) * invstd);
    }
    l1[t] = s1, l2[t] = s2;
    __syncthreads();
    s1 = ((l1[c0] + l1[c0 + 64]) + l1[c0 + 128]) + l1[c0 + 192];
    s2 = ((l2[c0] + l2[c0 + 64]) + l2[c0 + 128]) + l2[c0 + 192];
    __syncthreads();
    const double m1 = s1 / (double)B, m2 = s2 / (double)B, k = (double)fw[c] * invstd;
    double s3 = 0.0;
    for (int r = g; r < B; r += 4) {
        const double zh = ((double)z[(long long)r * N + c] - mean) * invstd;
        const float v = (float)(k * (gf[(long long)r * N + c] - m1 - zh * m2));
        gz[(long long)r * N + c] = v;
        s3 += (double)v;
    }
    l1[t] = s3;
    __syncthreads();
    if (g == 0) {
        d_feat_b[c] = (float)s1;
        d_fc_b[c] = (float)(((l1[t] + l1[t + 64]) + l1[t + 128]) + l1[t + 192]);
    }
}

// ---- backward: dgrad --------------------------------------------------------------------------------------------------------------
// grid (column tiles of K, row tiles of b): g_d = g_z W over all of n; g_y = g_d keep / (1 - p), fp32 [b][K]; per column the sums of
// g_y and g_y xhat over the tile's rows in double, rows ascending, the two half-waves last: cpart double [row tiles][2][K].
template <typename T>
__global__ __launch_bounds__(256) void tail_dgrad_kernel(const float* __restrict__ gz, const float* __restrict__ w, const T* __restrict__ x,
                                                         const uint8_t* __restrict__ keep, const double* __restrict__ stat, int B, int ch, int K, int N,
                                                         float inv_keep, float* __restrict__ gy, double* __restrict__ cpart) {
    __shared__ __attribute__((aligned(16))) float sA[TM * LDR];
    __shared__ __attribute__((aligned(16))) float sB[TK * LDK];
    const int n0 = blockIdx.x * TM, m0 = blockIdx.y * TM;
    const int kc = (threadIdx.x & 7) * 4, rr = threadIdx.x >> 3, cc = (threadIdx.x & 31) * 4, cr = threadIdx.x >> 5;
    f32x16 acc[4];
    zero_acc<4>(acc);
    f32x4 va[4], vb[4];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + rr + 32 * i;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (row < B) a = *(const f32x4*)(gz + (long long)row * N + j0 + kc);
            if (n0 + cc < K) b = *(const f32x4*)(w + (long long)(j0 + cr + 8 * i) * K + n0 + cc);
            va[i] = a, vb[i] = b;
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < N; j0 += TK) {
        __syncthreads();
        stash_rows<4>(sA, va);
        stash_cols(sB, vb);
        __syncthreads();
        if (j0 + TK < N) fetch(j0 + TK);
        mma_stage<true, false, 4>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = n0 + wv * 32 + r;
    const bool valid = col < K;
    const int c = valid ? col % ch : 0;
    const double mean = stat[c], invstd = stat[ch + c];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = m0 + tile_row(t, e, h);
            if (valid && row < B) {
                const long long o = (long long)row * K + col;
                const bool kept = keep ? keep[o] != 0 : true;
                const float v = kept ? acc[t][e] * inv_keep : 0.f;
                gy[o] = v;
                s1 += (double)v;
                s2 += (double)v * (((double)(float)x[o] - mean) * invstd);
            }
        }
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (valid && h == 0) {
        cpart[((long long)blockIdx.y * 2 + 0) * K + col] = s1;
        cpart[((long long)blockIdx.y * 2 + 1) * K + col] = s2;
    }
}

// one thread per channel: the partials over row tiles, then positions, ascending.  cmean: double [2][ch], the sums / (b hw).
__global__ __launch_bounds__(64) void tail_bn2_grad_kernel(const double* __restrict__ cpart, int row_tiles, int hw, int ch, int rows,
                                                           float* __restrict__ d_w, float* __restrict__ d_b, double* __restrict__ cmean) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const long long K = (long long)hw * ch;
    double s1 = 0.0, s2 = 0.0;
    for (int rt = 0; rt < row_tiles; ++rt)
        for (int p = 0; p < hw; ++p) {
            s1 += cpart[((long long)rt * 2 + 0) * K + (long long)p * ch + c];
            s2 += cpart[((long long)rt * 2 + 1) * K + (long long)p * ch + c];
        }
    d_b[c] = (float)s1;
    d_w[c] = (float)s2;
    cmean[c] = s1 / (double)rows;
    cmean[ch + c] = s2 / (double)rows;
}

template <typename T>
__global__ __launch_bounds__(256) void tail_dx_kernel(const float* __restrict__ gy, const T* __restrict__ x, const double* __restrict__ stat,
                                                      const double* __restrict__ cmean, const float* __restrict__ gamma, long long total, int ch,
                                                      float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % ch);
    const double invstd = stat[ch + c], xh = ((double)(float)x[i] - stat[c]) * invstd;
    dx[i] = (float)((double)gamma[c] * invstd * ((double)gy[i] - cmean[c] - xh * cmean[ch + c]));
}

// ---- backward: wgrad --------------------------------------------------------------------------------------------------------------
// grid (column tiles of K, row tiles of n): dW[j][k] = sum_i g_z[i][j] d[i][k], the batch in ascending stages of 32 inside the
// workgroup; d is recomputed from x, the affine and the mask exactly as the forward formed it.
template <typename T>
__global__ __launch_bounds__(256) void tail_wgrad_kernel(const float* __restrict__ gz, const T* __restrict__ x, const uint8_t* __restrict__ keep,
                                                         const float* __restrict__ affine, int B, int ch, int K, int N, float inv_keep,
                                                         float* __restrict__ dw) {
    __shared__ __attribute__((aligned(16))) float sA[TK * LDK];
    __shared__ __attribute__((aligned(16))) float sB[TK * LDK];
    const int k0 = blockIdx.x * TM, j0 = blockIdx.y * TM;
    const int cc = (threadIdx.x & 31) * 4, cr = threadIdx.x >> 5;
    const bool kin = k0 + cc < K, jin = j0 + cc < N;
    const int c = kin ? (k0 + cc) % ch : 0;
    const f32x4 sc = *(const f32x4*)(affine + c), sh = *(const f32x4*)(affine + ch + c);
    f32x16 acc[4];
    zero_acc<4>(acc);
    f32x4 va[4], vb[4];
    auto fetch = [&](int i0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i0 + cr + 8 * i;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (row < B) {
                if (jin) a = *(const f32x4*)(gz + (long long)row * N + j0 + cc);
                if (kin) {
                    const long long o = (long long)row * K + k0 + cc;
                    b = dropped4(load4<T>(x + o), sc, sh, keep ? *(const uint32_t*)(keep + o) : 0x01010101u, inv_keep);
                }
            }
            va[i] = a, vb[i] = b;
        }
    };
    fetch(0);
    for (int i0 = 0; i0 < B; i0 += TK) {
        __syncthreads();
        stash_cols(sA, va);
        stash_cols(sB, vb);
        __syncthreads();
        if (i0 + TK < B) fetch(i0 + TK);
        mma_stage<false, false, 4>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = k0 + wv * 32 + r;
    if (col < K) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = j0 + tile_row(t, e, h);
                if (row < N) dw[(long long)row * K + col] = acc[t][e];
            }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct TailPlan {
    int row_tiles, col_tiles, steps, per, k_slices, stat_per, stat_slices;
    size_t spart, fpart, gf, gz, gy, cpart, cmean, total;      // workspace offsets
};

inline bool tail_dims_ok(int b, int ch, int hw, int n) {
    return b >= 1 && b <= TAIL_MAX_B && ch >= 64 && ch <= TAIL_MAX_CH && ch % 64 == 0 && hw >= 1 && hw <= TAIL_MAX_HW && n >= 64 &&
           n <= TAIL_MAX_N && n % 64 == 0;
}

// K slices of the fc forward: enough workgroups to fill the machine, at least 8 stages of 32 per slice, at most 64 slices
// (b = 128, 512 / 49 / 512: 4 column tiles x 61 slices of 13 stages)
TailPlan tail_plan(int b, int ch, int hw, int n) {
    TailPlan p;
    const long long K = (long long)hw * ch;
    p.row_tiles = (b + TM - 1) / TM;
    p.col_tiles = (n + TM - 1) / TM;
    p.steps = (int)(K / TK);
    int ks = TAIL_FILL / (p.row_tiles * p.col_tiles);
    if (ks > p.steps / 8) ks = p.steps / 8;
    if (ks > TAIL_MAX_SLICES) ks = TAIL_MAX_SLICES;
    if (ks < 1) ks = 1;
    p.per = (p.steps + ks - 1) / ks;
    p.k_slices = (p.steps + p.per - 1) / p.per;
    const int rows = b * hw;
    int ss = (rows + 63) / 64;
    if (ss > TAIL_MAX_SLICES) ss = TAIL_MAX_SLICES;
    p.stat_per = (rows + ss - 1) / ss;
    p.stat_slices = (rows + p.stat_per - 1) / p.stat_per;
    size_t o = 0;
    p.spart = o, o += align256(sizeof(double) * 2 * (size_t)p.stat_slices * ch);
    p.fpart = o, o += align256(sizeof(float) * (size_t)p.k_slices * b * n);
    p.gf = o, o += align256(sizeof(double) * (size_t)b * n);
    p.gz = o, o += align256(sizeof(float) * (size_t)b * n);
    p.gy = o, o += align256(sizeof(float) * (size_t)b * K);
    p.cpart = o, o += align256(sizeof(double) * 2 * (size_t)p.row_tiles * K);
    p.cmean = o, o += align256(sizeof(double) * 2 * (size_t)ch);
    p.total = o;
    return p;
}

int tail_check(const char* api, const idb_tail_desc* d, const void* ws, size_t ws_bytes) {
    IDB_REQUIRE(d, "%s: null descriptor", api);
    IDB_REQUIRE(tail_dims_ok(d->b, d->ch, d->hw, d->n), "%s: b in 1..%d, ch %% 64 == 0 up to %d, hw in 1..%d, n %% 64 == 0 up to %d", api,
                TAIL_MAX_B, TAIL_MAX_CH, TAIL_MAX_HW, TAIL_MAX_N);
    IDB_REQUIRE(d->x_dtype == IDB_F16 || d->x_dtype == IDB_BF16 || d->x_dtype == IDB_F32, "%s: x_dtype %d, expected IDB_F16, IDB_BF16 or IDB_F32",
                api, d->x_dtype);
    IDB_REQUIRE(d->training == 0 || d->training == 1, "%s: training must be 0 or 1", api);
    IDB_REQUIRE(!d->training || d->b >= 2, "%s: a batch of one in training mode (upstream's BatchNorm1d raises: no batch variance)", api);
    IDB_REQUIRE(d->p >= 0.0 && d->p < 1.0, "%s: dropout p in [0, 1)", api);
    IDB_REQUIRE(d->eps2 >= 0.0 && d->eps2 <= 1.0 && d->eps1 >= 0.0 && d->eps1 <= 1.0 && d->momentum >= 0.0 && d->momentum <= 1.0,
                "%s: eps in [0, 1], momentum in [0, 1]", api);
    IDB_REQUIRE(d->x && d->bn2_weight && d->bn2_bias && d->bn2_mean && d->bn2_var && d->fc_weight && d->fc_bias && d->feat_weight &&
                    d->feat_bias && d->feat_mean && d->feat_var,
                "%s: null pointer", api);
    IDB_REQUIRE(idb_aligned16(d->x) && idb_aligned16(d->fc_weight) && (((uintptr_t)d->keep) & 3) == 0,
                "%s: x and fc_weight 16-byte aligned, keep 4-byte aligned", api);
    IDB_REQUIRE(!d->keep || d->training, "%s: a keep-mask in eval mode", api);
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= tail_plan(d->b, d->ch, d->hw, d->n).total, "%s: workspace too small or unaligned", api);
    return IDB_OK;
}

inline float tail_inv_keep(const idb_tail_desc* d) { return d->training ? (float)(1.0 / (1.0 - d->p)) : 1.f; }

template <typename T>
int tail_forward_run(const idb_tail_desc* d, float* emb, double* norms, double* bn2_stat, float* affine, float* z, double* feat_stat, float* f,
                     int32_t* flags, char* w, hipStream_t st) {
    const TailPlan p = tail_plan(d->b, d->ch, d->hw, d->n);
    const int K = d->hw * d->ch, rows = d->b * d->hw;
    const T* x = (const T*)d->x;
    if (hipMemsetAsync(flags, 0, 4 * sizeof(int32_t), st) != hipSuccess) {
        idb_set_error("idb_tail_forward: hipMemsetAsync failed");
        return IDB_EHIP;
    }
    if (d->training) {
        hipLaunchKernelGGL(tail_stats_kernel<T>, dim3(d->ch / 64, p.stat_slices), dim3(256), 0, st, x, rows, d->ch, p.stat_per,
                           (double*)(w + p.spart));
        IDB_CHECK_LAUNCH("idb_tail_forward(stats)");
    }
    hipLaunchKernelGGL(tail_bn2_kernel<T>, dim3(d->ch / 64), dim3(64), 0, st, x, (const double*)(w + p.spart), p.stat_slices, rows, d->ch,
                       d->training, d->eps2, d->momentum, d->bn2_weight, d->bn2_bias, d->bn2_mean, d->bn2_var, bn2_stat, affine, flags);
    IDB_CHECK_LAUNCH("idb_tail_forward(bn2)");
    hipLaunchKernelGGL(tail_fc_kernel<T>, dim3(p.col_tiles, p.row_tiles, p.k_slices), dim3(256), 0, st, x, d->keep, (const float*)affine,
                       d->fc_weight, d->b, d->ch, K, d->n, p.per, tail_inv_keep(d), (float*)(w + p.fpart));
    IDB_CHECK_LAUNCH("idb_tail_forward(fc)");
    hipLaunchKernelGGL(tail_merge_kernel, dim3((d->b * d->n + 255) / 256), dim3(256), 0, st, (const float*)(w + p.fpart), p.k_slices, d->b, d->n,
                       d->fc_bias, z);
    IDB_CHECK_LAUNCH("idb_tail_forward(merge)");
    hipLaunchKernelGGL(tail_feat_stats_kernel, dim3(d->n / 64), dim3(256), 0, st, (const float*)z, d->b, d->n, d->training, d->eps1, d->momentum,
                       d->feat_mean, d->feat_var, feat_stat, flags);
    IDB_CHECK_LAUNCH("idb_tail_forward(features)");
    hipLaunchKernelGGL(tail_rows_kernel, dim3((d->b + 3) / 4), dim3(256), 0, st, (const float*)z, (const double*)feat_stat, d->feat_weight,
                       d->feat_bias, d->b, d->n, f, emb, norms, flags);
    IDB_CHECK_LAUNCH("idb_tail_forward(rows)");
    return IDB_OK;
}

template <typename T>
int tail_backward_run(const idb_tail_desc* d, const float* g_emb, const float* emb, const double* norms, const double* bn2_stat,
                      const float* affine, const float* z, const double* feat_stat, const float* f, int renorm, float* d_bn2_w, float* d_bn2_b,
                      float* d_fc_w, float* d_fc_b, float* d_feat_b, float* d_x, char* w, hipStream_t st) {
    const TailPlan p = tail_plan(d->b, d->ch, d->hw, d->n);
    const int K = d->hw * d->ch, rows = d->b * d->hw, kt = (K + TM - 1) / TM;
    const T* x = (const T*)d->x;
    double* gf = (double*)(w + p.gf);
    float* gz = (float*)(w + p.gz);
    float* gy = (float*)(w + p.gy);
    double* cpart = (double*)(w + p.cpart);
    double* cmean = (double*)(w + p.cmean);
    const float ik = tail_inv_keep(d);
    hipLaunchKernelGGL(tail_bwd_rows_kernel, dim3((d->b + 3) / 4), dim3(256), 0, st, g_emb, emb, f, norms, d->b, d->n, renorm, gf);
    IDB_CHECK_LAUNCH("idb_tail_backward(rows)");
    hipLaunchKernelGGL(tail_bwd_feat_kernel, dim3(d->n / 64), dim3(256), 0, st, (const double*)gf, z, feat_stat, d->feat_weight, d->b, d->n, gz,
                       d_feat_b, d_fc_b);
    IDB_CHECK_LAUNCH("idb_tail_backward(features)");
    hipLaunchKernelGGL(tail_dgrad_kernel<T>, dim3(kt, p.row_tiles), dim3(256), 0, st, (const float*)gz, d->fc_weight, x, d->keep, bn2_stat, d->b,
                       d->ch, K, d->n, ik, gy, cpart);
    IDB_CHECK_LAUNCH("idb_tail_backward(dgrad)");
    hipLaunchKernelGGL(tail_bn2_grad_kernel, dim3(d->ch / 64), dim3(64), 0, st, (const double*)cpart, p.row_tiles, d->hw, d->ch, rows, d_bn2_w,
                       d_bn2_b, cmean);
    IDB_CHECK_LAUNCH("idb_tail_backward(bn2)");
    if (d_x) {
        const long long total = (long long)d->b * K;
        hipLaunchKernelGGL(tail_dx_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)gy, x, bn2_stat,
                           (const double*)cmean, d->bn2_weight, total, d->ch, d_x);
        IDB_CHECK_LAUNCH("idb_tail_backward(dx)");
    }
    hipLaunchKernelGGL(tail_wgrad_kernel<T>, dim3(kt, p.col_tiles), dim3(256), 0, st, (const float*)gz, x, d->keep, affine, d->b, d->ch, K, d->n,
                       ik, d_fc_w);
    IDB_CHECK_LAUNCH("idb_tail_backward(wgrad)");
    return IDB_OK;
}

}  // namespace

extern "C" size_t idb_tail_workspace_bytes(int32_t b, int32_t ch, int32_t hw, int32_t n, int32_t* k_slices, int32_t* row_tiles) {
    if (!tail_dims_ok(b, ch, hw, n)) return 0;
    const TailPlan p = tail_plan(b, ch, hw, n);
    if (k_slices) *k_slices = p.k_slices;
    if (row_tiles) *row_tiles = p.row_tiles;
    return p.total;
}

extern "C" int idb_tail_forward(const idb_tail_desc* d, float* emb, double* norms, double* bn2_stat, float* affine, float* z, double* feat_stat,
                                float* f, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const int rc = tail_check("idb_tail_forward", d, ws, ws_bytes);
    if (rc != IDB_OK) return rc;
    IDB_REQUIRE(emb && norms && bn2_stat && affine && z && feat_stat && f && flags, "idb_tail_forward: null output pointer");
    IDB_REQUIRE(idb_aligned16(affine), "idb_tail_forward: affine 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (d->x_dtype == IDB_F32) return tail_forward_run<float>(d, emb, norms, bn2_stat, affine, z, feat_stat, f, flags, (char*)ws, st);
    if (d->x_dtype == IDB_F16) return tail_forward_run<_Float16>(d, emb, norms, bn2_stat, affine, z, feat_stat, f, flags, (char*)ws, st);
    return tail_forward_run<__bf16>(d, emb, norms, bn2_stat, affine, z, feat_stat, f, flags, (char*)ws, st);
}

extern "C" int idb_tail_backward(const idb_tail_desc* d, const float* g_emb, const float* emb, const double* norms, const double* bn2_stat,
                                 const float* affine, const float* z, const double* feat_stat, const float* f, int32_t renormalised,
                                 float* d_bn2_weight, float* d_bn2_bias, float* d_fc_weight, float* d_fc_bias, float* d_feat_bias, float* d_x,
                                 void* ws, size_t ws_bytes, void* stream) {
    const int rc = tail_check("idb_tail_backward", d, ws, ws_bytes);
    if (rc != IDB_OK) return rc;
    IDB_REQUIRE(d->training, "idb_tail_backward: the forward ran in eval mode (the backward is that of the batch statistics)");
    IDB_REQUIRE(g_emb && emb && norms && bn2_stat && affine && z && feat_stat && f, "idb_tail_backward: null input pointer");
    IDB_REQUIRE(d_bn2_weight && d_bn2_bias && d_fc_weight && d_fc_bias && d_feat_bias, "idb_tail_backward: null output pointer");
    IDB_REQUIRE(idb_aligned16(affine) && idb_aligned16(g_emb), "idb_tail_backward: affine and g_emb 16-byte aligned");
    IDB_REQUIRE(renormalised == 0 || renormalised == 1, "idb_tail_backward: renormalised must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
#define TAIL_BWD(T)                                                                                                                          \
    tail_backward_run<T>(d, g_emb, emb, norms, bn2_stat, affine, z, feat_stat, f, renormalised, d_bn2_weight, d_bn2_bias, d_fc_weight, d_fc_bias, \
                         d_feat_bias, d_x, (char*)ws, st)
    if (d->x_dtype == IDB_F32) return TAIL_BWD(float);
    if (d->x_dtype == IDB_F16) return TAIL_BWD(_Float16);
    return TAIL_BWD(__bf16);
#undef TAIL_BWD
}
