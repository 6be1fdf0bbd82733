// The convolutional trunk of the face-recognition backbone in training (ID-Booth's FR_training/backbones/iresnet.py: the stem and
// IBasicBlock), forward and backward, as the pieces a block is composed of.  fp32 state, every product on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32), every
// statistic and cross-workgroup reduction in double in an order the shapes alone decide, no floating-point atomics, every index in
// 64 bits, tile rows and columns past the end loaded as zeros and never stored.
//   Activations and their gradients are NHWC [b][h][w][c]; conv weights and their gradients are [cout][ky][kx][cin].
//   bn        stats     shifted sums per channel over slices of the rows (the shift is row 0), as tail_stats_kernel
//             finish    one wave per channel: lane l takes slices l, l + 64, ... ascending, then the xor butterfly; mean, biased
//                       variance, invstd, the running statistics, the fp32 affine sc = gamma invstd, sh = beta - mean sc
//   conv      forward   implicit GEMM, M = b ho wo, N = cout, K = taps cin; a = prelu(fma(x, sc, sh)) formed in the A-operand load,
//                       an out-of-image tap is an exact 0 (the padding comes after the BatchNorm)
//             dgrad     M = the input pixels of one stride-parity class, N = cin, K = (the taps that reach the class) cout
//             wgrad     rows = the (tap, cin) index, columns = cout, the reduction over b ho wo in slices; a recomputed as in forward
//             merge     the slices in ascending order in double, rounded once
//   bn bwd    sums      per (row slice, channel) in double: S1 = sum g_y, S2 = sum g_y xhat, S3 = sum g min(y, 0)
//             finish    one wave per channel as above: d beta, d gamma, d slope, the two means
//             apply     g_c = gamma invstd (g_y - S1 / n - xhat S2 / n) (+ a second gradient), rounded once
//   affine    out = prelu(fma(c, sc, sh)) (+ identity or + fma(cd, scd, shd)): the stem's activation and the block's residual
//   pack      float NCHW [b][3][h][w] -> NHWC [b][h][w][4], the fourth channel 0
// The tile helpers are idb_f32mma.h's; the loop's clipped SGD step over a table of tensors is idb_sgd.hip.
#include "idb_f32mma.h"
#include <math.h>

namespace {

constexpr int BLK_MAX_B = 1024, BLK_MAX_C = 2048, BLK_MAX_HW = 128;
constexpr int BLK_FILL = 256;      // workgroups that fill the machine
constexpr int BLK_MAX_WSLICES = 64, BLK_MAX_SSLICES = 1024;

// the activation a conv reads: fma(x, sc, sh), one rounding, then PReLU (one more on the negative side)
__device__ __forceinline__ f32x4 act4(f32x4 x, f32x4 sc, f32x4 sh, f32x4 sl, bool affine, bool prelu) {
    f32x4 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = affine ? __builtin_fmaf(x[e], sc[e], sh[e]) : x[e];
        if (prelu) v = v > 0.f ? v : sl[e] * v;
        a[e] = v;
    }
    return a;
}

struct ConvGeo {
    int B, H, W, cin, cout, ks, stride, pad, Ho, Wo, taps, K;      // K = taps cin
    int Mo;                                                        // b ho wo (<= 2^24)
};

// ---- BatchNorm2d statistics ---------------------------------------------------------------------------------------------------------
// grid (ch / 64, slices): thread (g = t >> 6, c = t & 63) sums x - x[0][c] and its square over rows first + g, first + g + 4, ... of its
// slice in double; the four are added in order.  part: double [slices][2][ch].
__global__ __launch_bounds__(256) void blk_stats_kernel(const float* __restrict__ x, int rows, int ch, int per, double* __restrict__ part) {
    __shared__ double l1[256], l2[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int first = blockIdx.y * per, last = min(rows, first + per);
    const double x0 = (double)x[c];
    double s1 = 0.0, s2 = 0.0;
    for (int r = first + g; r < last; r += 4) {
        const double v = (double)x[(long long)r * ch + c] - x0;
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

// the slices of one channel's partial `which` (of `nsum` per slice) met in one wave: lane l adds slices l, l + 64, ... in ascending
// order, then the xor butterfly; every lane gets the total
__device__ __forceinline__ double wave_merge_d(const double* __restrict__ part, int slices, int nsum, int which, int ch, int c) {
    const int l = threadIdx.x & 63;
    double s = 0.0;
    for (int i = l; i < slices; i += 64) s += part[((long long)i * nsum + which) * ch + c];
    return wave_sum_d(s);
}

// grid ch / 4, one wave per channel (tail_bn2_kernel's arithmetic without its one-thread chain over the slices).
// stat: double [2][ch] mean, invstd.  affine: fp32 [2][ch] sc, sh.  flags[0]: a statistic is not finite.  flags[1]: var + eps == 0.
__global__ __launch_bounds__(256) void blk_bn_kernel(const float* __restrict__ x, const double* __restrict__ part, int slices, int rows, int ch,
                                                     int training, double eps, double momentum, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar,
                                                     double* __restrict__ stat, float* __restrict__ affine, int32_t* __restrict__ flags) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    double mean, var;
    if (training) {
        const double s1 = wave_merge_d(part, slices, 2, 0, ch, c), s2 = wave_merge_d(part, slices, 2, 1, ch, c);
        if ((threadIdx.x & 63) != 0) return;
        const double n = (double)rows, m = s1 / n;
        mean = (double)x[c] + m;
        var = (s2 - s1 * m) / n;
        if (var < 0.0) var = 0.0;
        rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
        rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * (var * (n / (n - 1.0))));
    } else {
        if ((threadIdx.x & 63) != 0) return;
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

// ---- convolution forward ------------------------------------------------------------------------------------------------------------
// grid (row tiles of b ho wo, column tiles of cout).  Thread t stages reduction columns 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i: the
// four columns lie inside one tap (cin % 4 == 0).
template <int WN>
__global__ __launch_bounds__(256) void blk_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ affine,
                                                           const float* __restrict__ slope, const float* __restrict__ w, ConvGeo g,
                                                           float* __restrict__ out) {
    __shared__ float sA[TM * LDR], sB[TM * LDR];
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * (32 * WN);
    const int kc = (threadIdx.x & 7) * 4, rr = threadIdx.x >> 3;
    int rb[4], ry[4], rx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + rr + 32 * i;
        rb[i] = -1, ry[i] = 0, rx[i] = 0;
        if (m < g.Mo) {
            const int b = m / (g.Ho * g.Wo), rem = m - b * (g.Ho * g.Wo), oy = rem / g.Wo;
            rb[i] = b, ry[i] = oy * g.stride - g.pad, rx[i] = (rem - oy * g.Wo) * g.stride - g.pad;
        }
    }
    f32x16 acc[WN];
    zero_acc<WN>(acc);
    f32x4 va[4], vb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + kc;
        const bool kin = k < g.K;
        const int tap = kin ? k / g.cin : 0, ci = kin ? k - tap * g.cin : 0, ky = tap / g.ks, kx = tap - ky * g.ks;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 sc = zero, sh = zero, sl = zero;
        if (affine) sc = *(const f32x4*)(affine + ci), sh = *(const f32x4*)(affine + g.cin + ci);
        if (slope) sl = *(const f32x4*)(slope + ci);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = ry[i] + ky, ix = rx[i] + kx;
            f32x4 a = zero;
            if (kin && rb[i] >= 0 && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                a = act4(*(const f32x4*)(x + (((long long)rb[i] * g.H + iy) * g.W + ix) * g.cin + ci), sc, sh, sl, affine != nullptr,
                         slope != nullptr);
            va[i] = a;
            f32x4 b = zero;
            const int col = n0 + rr + 32 * i;
            if (i < WN && kin && col < g.cout) b = *(const f32x4*)(w + (long long)col * g.K + k);
            vb[i] = b;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < g.K; k0 += TK) {
        __syncthreads();
        stash_rows<4>(sA, va);
        stash_rows<WN>(sB, vb);
        __syncthreads();
        if (k0 + TK < g.K) fetch(k0 + TK);
        mma_stage<true, true, WN>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = n0 + (wv % WN) * 32 + r, wr = (wv / WN) * WN;
    if (col < g.cout) {
#pragma unroll
        for (int t = 0; t < WN; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + tile_row(wr + t, e, h);
                if (row < g.Mo) out[(long long)row * g.cout + col] = acc[t][e];
            }
    }
}

// ---- convolution dgrad --------------------------------------------------------------------------------------------------------------
// grid (row tiles of the largest parity class, column tiles of cin, stride^2 classes).  Class (py, px) holds the input pixels
// y = py + stride i, x = px + stride j; only the taps with (y + pad - ky) % stride == 0 (and likewise in x) reach it, and the
// reduction runs over those taps alone: no MFMA step is spent on a tap that cannot contribute.  A class no tap reaches (the 1x1
// stride-2 conv's odd pixels) is written as zeros.
template <int WN>
__global__ __launch_bounds__(256) void blk_conv_dgrad_kernel(const float* __restrict__ go, const float* __restrict__ w, ConvGeo g,
                                                             float* __restrict__ gi) {
    __shared__ __attribute__((aligned(16))) float sA[TM * LDR];
    __shared__ __attribute__((aligned(16))) float sB[TK * LDK];
    const int s = g.stride, py = blockIdx.z / s, px = blockIdx.z % s;
    const int Hc = py < g.H ? (g.H - py + s - 1) / s : 0, Wc = px < g.W ? (g.W - px + s - 1) / s : 0, Mc = g.B * Hc * Wc;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * (32 * WN);
    if (m0 >= Mc) return;
    unsigned long long list = 0;       // the taps that reach this class, 4 bits each
    int nvalid = 0;
    for (int tap = 0; tap < g.taps; ++tap) {
        const int ky = tap / g.ks, kx = tap - ky * g.ks;
        if (((py + g.pad - ky) & (s - 1)) == 0 && ((px + g.pad - kx) & (s - 1)) == 0) list |= (unsigned long long)tap << (4 * nvalid++);
    }
    const int kc = (threadIdx.x & 7) * 4, rr = threadIdx.x >> 3, cc = (threadIdx.x & 31) * 4, cr = threadIdx.x >> 5;
    int rb[4], ry[4], rx[4];           // the sample, y + pad, x + pad of this thread's staged rows
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + rr + 32 * i;
        rb[i] = -1, ry[i] = 0, rx[i] = 0;
        if (m < Mc) {
            const int b = m / (Hc * Wc), rem = m - b * (Hc * Wc), yc = rem / Wc;
            rb[i] = b, ry[i] = py + s * yc + g.pad, rx[i] = px + s * (rem - yc * Wc) + g.pad;
        }
    }
    f32x16 acc[WN];
    zero_acc<WN>(acc);
    f32x4 va[4], vb[4];
    const int per_tap = g.cout / TK, stages = nvalid * per_tap;
    auto fetch = [&](int st) {
        const int ti = st / per_tap, c0 = (st - ti * per_tap) * TK, tap = (int)((list >> (4 * ti)) & 15), ky = tap / g.ks, kx = tap - ky * g.ks;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ny = ry[i] - ky, nx = rx[i] - kx, oy = ny / s, ox = nx / s;      // exact by the class
            f32x4 a = zero, b = zero;
            if (rb[i] >= 0 && ny >= 0 && nx >= 0 && oy < g.Ho && ox < g.Wo)
                a = *(const f32x4*)(go + (((long long)rb[i] * g.Ho + oy) * g.Wo + ox) * g.cout + c0 + kc);
            if (cc < 32 * WN && n0 + cc < g.cin) b = *(const f32x4*)(w + ((long long)(c0 + cr + 8 * i) * g.taps + tap) * g.cin + n0 + cc);
            va[i] = a, vb[i] = b;
        }
    };
    if (stages > 0) fetch(0);
    for (int st = 0; st < stages; ++st) {
        __syncthreads();
        stash_rows<4>(sA, va);
        stash_cols(sB, vb);
        __syncthreads();
        if (st + 1 < stages) fetch(st + 1);
        mma_stage<true, false, WN>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = n0 + (wv % WN) * 32 + r, wr = (wv / WN) * WN;
    if (col < g.cin) {
#pragma unroll
        for (int t = 0; t < WN; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + tile_row(wr + t, e, h);
                if (row < Mc) {
                    long long pix = row;
                    if (s > 1) {
                        const int b = row / (Hc * Wc), rem = row - b * (Hc * Wc), yc = rem / Wc;
                        pix = ((long long)b * g.H + py + s * yc) * g.W + px + s * (rem - yc * Wc);
                    }
                    gi[pix * g.cin + col] = acc[t][e];
                }
            }
    }
}

// ---- convolution wgrad --------------------------------------------------------------------------------------------------------------
// grid (row tiles of K = taps cin, column tiles of cout, slices of b ho wo).  dW[co][k] = sum_m g_out[m][co] a[m, k]: both operands
// staged [m][.]; thread t holds K-columns 4 (t & 31) .. + 3 (one tap, four channels, fixed for the whole kernel) and cout-columns
// 4 (t & 31) .. + 3 of reduction rows (t >> 5) + 8 i.  part: fp32 [slices][cout][K].
template <int WN>
__global__ __launch_bounds__(256) void blk_conv_wgrad_kernel(const float* __restrict__ go, const float* __restrict__ x,
                                                             const float* __restrict__ affine, const float* __restrict__ slope, ConvGeo g,
                                                             int per, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sA[TK * LDK];
    __shared__ __attribute__((aligned(16))) float sB[TK * LDK];
    const int k0 = blockIdx.x * TM, j0 = blockIdx.y * (32 * WN);
    const int cc = (threadIdx.x & 31) * 4, cr = threadIdx.x >> 5;
    const int k = k0 + cc;
    const bool kin = k < g.K, jin = cc < 32 * WN && j0 + cc < g.cout;
    const int tap = kin ? k / g.cin : 0, ci = kin ? k - tap * g.cin : 0, ky = tap / g.ks - g.pad, kx = tap % g.ks - g.pad;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 sc = zero, sh = zero, sl = zero;
    if (affine) sc = *(const f32x4*)(affine + ci), sh = *(const f32x4*)(affine + g.cin + ci);
    if (slope) sl = *(const f32x4*)(slope + ci);
    const int mfirst = blockIdx.z * per * TK, mlast = min(g.Mo, mfirst + per * TK);
    f32x16 acc[WN];
    zero_acc<WN>(acc);
    f32x4 va[4], vb[4];
    auto fetch = [&](int ms) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = ms + cr + 8 * i;
            f32x4 a = zero, b = zero;
            if (m < mlast) {
                if (kin) {
                    const int bb = m / (g.Ho * g.Wo), rem = m - bb * (g.Ho * g.Wo), oy = rem / g.Wo;
                    const int iy = oy * g.stride + ky, ix = (rem - oy * g.Wo) * g.stride + kx;
                    if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                        a = act4(*(const f32x4*)(x + (((long long)bb * g.H + iy) * g.W + ix) * g.cin + ci), sc, sh, sl, affine != nullptr,
                                 slope != nullptr);
                }
                if (jin) b = *(const f32x4*)(go + (long long)m * g.cout + j0 + cc);
            }
            va[i] = a, vb[i] = b;
        }
    };
    if (mfirst < mlast) fetch(mfirst);
    for (int ms = mfirst; ms < mlast; ms += TK) {
        __syncthreads();
        stash_cols(sA, va);
        stash_cols(sB, vb);
        __syncthreads();
        if (ms + TK < mlast) fetch(ms + TK);
        mma_stage<false, false, WN>(sA, sB, acc);
    }
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, r = l & 31, h = l >> 5, col = j0 + (wv % WN) * 32 + r, wr = (wv / WN) * WN;
    if (col < g.cout) {
        float* o = part + ((long long)blockIdx.z * g.cout + col) * g.K;
#pragma unroll
        for (int t = 0; t < WN; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = k0 + tile_row(wr + t, e, h);
                if (row < g.K) o[row] = acc[t][e];
            }
    }
}

__global__ __launch_bounds__(256) void blk_wgrad_merge_kernel(const float* __restrict__ part, int slices, long long total, float* __restrict__ dw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double)part[(long long)k * total + i];
    dw[i] = (float)s;
}

// ---- BatchNorm (+ PReLU) backward ---------------------------------------------------------------------------------------------------
// y = fma(c, sc, sh) is the forward's own fp32 value, so the PReLU branch is the forward's; g_y = y > 0 ? g : slope g (y == 0 takes the
// slope, as torch does); xhat = (c - mean) invstd in double.
__device__ __forceinline__ double bwd_gy(float c, float g, float sc, float sh, bool prelu, float sl, float* y_out) {
    const float y = __builtin_fmaf(c, sc, sh);
    *y_out = y;
    return prelu && !(y > 0.f) ? (double)sl * (double)g : (double)g;
}

// grid (ch / 64, slices), thread (g4, c) as blk_stats_kernel.  part: double [slices][3][ch] S1, S2, S3.
__global__ __launch_bounds__(256) void blk_bnbwd_sums_kernel(const float* __restrict__ c, const float* __restrict__ g, const float* __restrict__ affine,
                                                             const double* __restrict__ stat, const float* __restrict__ slope, int rows, int ch,
                                                             int per, double* __restrict__ part) {
    __shared__ double l1[256], l2[256], l3[256];
    const int cidx = blockIdx.x * 64 + (threadIdx.x & 63), g4 = threadIdx.x >> 6;
    const int first = blockIdx.y * per, last = min(rows, first + per);
    const float sc = affine[cidx], sh = affine[ch + cidx], sl = slope ? slope[cidx] : 0.f;
    const double mean = stat[cidx], invstd = stat[ch + cidx];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = first + g4; r < last; r += 4) {
        const long long o = (long long)r * ch + cidx;
        float y;
        const double gy = bwd_gy(c[o], g[o], sc, sh, slope != nullptr, sl, &y);
        s1 += gy;
        s2 += gy * (((double)c[o] - mean) * invstd);
        s3 += (double)g[o] * (double)(y < 0.f ? y : 0.f);
    }
    const int t = threadIdx.x;
    l1[t] = s1, l2[t] = s2, l3[t] = s3;
    __syncthreads();
    if (g4 == 0) {
        part[((long long)blockIdx.y * 3 + 0) * ch + cidx] = ((l1[t] + l1[t + 64]) + l1[t + 128]) + l1[t + 192];
        part[((long long)blockIdx.y * 3 + 1) * ch + cidx] = ((l2[t] + l2[t + 64]) + l2[t + 128]) + l2[t + 192];
        part[((long long)blockIdx.y * 3 + 2) * ch + cidx] = ((l3[t] + l3[t + 64]) + l3[t + 128]) + l3[t + 192];
    }
}

// grid ch / 4, one wave per channel.  cmean: double [2][ch], S1 / n and S2 / n.
__global__ __launch_bounds__(256) void blk_bnbwd_finish_kernel(const double* __restrict__ part, int slices, int rows, int ch, float* __restrict__ d_gamma,
                                                               float* __restrict__ d_beta, float* __restrict__ d_slope, double* __restrict__ cmean) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double s1 = wave_merge_d(part, slices, 3, 0, ch, c), s2 = wave_merge_d(part, slices, 3, 1, ch, c),
                 s3 = wave_merge_d(part, slices, 3, 2, ch, c);
    if ((threadIdx.x & 63) != 0) return;
    d_beta[c] = (float)s1;
    d_gamma[c] = (float)s2;
    if (d_slope) d_slope[c] = (float)s3;
    cmean[c] = s1 / (double)rows;
    cmean[ch + c] = s2 / (double)rows;
}

// four channels per thread: g_c = gamma invstd (g_y - S1 / n - xhat S2 / n) + add, in double, rounded once
__global__ __launch_bounds__(256) void blk_bnbwd_apply_kernel(const float* __restrict__ c, const float* __restrict__ g, const float* __restrict__ affine,
                                                              const double* __restrict__ stat, const double* __restrict__ cmean,
                                                              const float* __restrict__ gamma, const float* __restrict__ slope,
                                                              const float* __restrict__ add, long long total4, int ch, float* __restrict__ gc) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const long long o = i * 4;
    const int c0 = (int)(o % ch);
    const f32x4 cv = *(const f32x4*)(c + o), gv = *(const f32x4*)(g + o);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 av = add ? *(const f32x4*)(add + o) : zero;
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int cidx = c0 + e;
        float y;
        const double gy = bwd_gy(cv[e], gv[e], affine[cidx], affine[ch + cidx], slope != nullptr, slope ? slope[cidx] : 0.f, &y);
        const double invstd = stat[ch + cidx], xh = ((double)cv[e] - stat[cidx]) * invstd;
        double v = (double)gamma[cidx] * invstd * (gy - cmean[cidx] - xh * cmean[ch + cidx]);
        if (add) v += (double)av[e];
        r[e] = (float)v;
    }
    *(f32x4*)(gc + o) = r;
}

// ---- the stem's activation and the block's residual ---------------------------------------------------------------------------------
// out = prelu(fma(c, sc, sh)) + (identity | fma(identity, scd, shd)): each fma rounded once, the sum rounded once
__global__ __launch_bounds__(256) void blk_affine_kernel(const float* __restrict__ c, const float* __restrict__ affine, const float* __restrict__ slope,
                                                         const float* __restrict__ idn, const float* __restrict__ id_affine, long long total4, int ch,
                                                         float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const long long o = i * 4;
    const int c0 = (int)(o % ch);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 v = act4(*(const f32x4*)(c + o), *(const f32x4*)(affine + c0), *(const f32x4*)(affine + ch + c0),
                   slope ? *(const f32x4*)(slope + c0) : zero, true, slope != nullptr);
    if (idn) {
        f32x4 d = *(const f32x4*)(idn + o);
        if (id_affine) d = act4(d, *(const f32x4*)(id_affine + c0), *(const f32x4*)(id_affine + ch + c0), zero, true, false);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] + d[e];
    }
    *(f32x4*)(out + o) = v;
}

// float NCHW [b][3][h][w] -> NHWC [b][h][w][4]
__global__ __launch_bounds__(256) void blk_pack_kernel(const float* __restrict__ img, long long pixels, int hw, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pixels) return;
    const long long b = i / hw, p = i - b * hw;
    const float* s = img + b * 3 * hw + p;
    const f32x4 v = {s[0], s[hw], s[2 * (long long)hw], 0.f};
    *(f32x4*)(out + i * 4) = v;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
inline bool conv_dims_ok(int b, int h, int w, int cin, int cout, int ks, int stride) {
    return b >= 1 && b <= BLK_MAX_B && h >= 1 && h <= BLK_MAX_HW && w >= 1 && w <= BLK_MAX_HW && (cin == 4 || (cin >= 64 && cin % 64 == 0)) &&
           cin <= BLK_MAX_C && cout >= 64 && cout % 64 == 0 && cout <= BLK_MAX_C && (ks == 1 || ks == 3) && (stride == 1 || stride == 2);
}

ConvGeo conv_geo(int b, int h, int w, int cin, int cout, int ks, int stride) {
    ConvGeo g;
    g.B = b, g.H = h, g.W = w, g.cin = cin, g.cout = cout, g.ks = ks, g.stride = stride, g.pad = ks == 3 ? 1 : 0;
    g.Ho = (h + 2 * g.pad - ks) / stride + 1, g.Wo = (w + 2 * g.pad - ks) / stride + 1;
    g.taps = ks * ks, g.K = g.taps * cin;
    g.Mo = b * g.Ho * g.Wo;
    return g;
}

struct ConvPlan {
    int wn_out, wn_in;                 // 32-column groups per tile over cout and over cin
    int fwd_row_tiles, dgrad_row_tiles, wgrad_row_tiles, wgrad_col_tiles, per, slices;
    size_t total;
};

// wgrad slices of the b ho wo reduction: enough workgroups to fill the machine, at least 4 stages of 32 rows per slice, at most 64
ConvPlan conv_plan(const ConvGeo& g) {
    ConvPlan p;
    p.wn_out = g.cout % 128 == 0 ? 4 : 2;
    p.wn_in = g.cin % 128 == 0 ? 4 : 2;
    p.fwd_row_tiles = (g.Mo + TM - 1) / TM;
    const int hc = (g.H + g.stride - 1) / g.stride, wc = (g.W + g.stride - 1) / g.stride;      // class (0, 0) is the largest
    p.dgrad_row_tiles = (g.B * hc * wc + TM - 1) / TM;
    p.wgrad_row_tiles = (g.K + TM - 1) / TM;
    p.wgrad_col_tiles = g.cout / (32 * p.wn_out);
    const int steps = (g.Mo + TK - 1) / TK;
    int ks = BLK_FILL / (p.wgrad_row_tiles * p.wgrad_col_tiles);
    if (ks > steps / 4) ks = steps / 4;
    if (ks > BLK_MAX_WSLICES) ks = BLK_MAX_WSLICES;
    if (ks < 1) ks = 1;
    p.per = (steps + ks - 1) / ks;
    p.slices = (steps + p.per - 1) / p.per;
    p.total = align256(sizeof(float) * (size_t)p.slices * g.cout * g.K);
    return p;
}

int conv_check(const char* api, const idb_blk_conv_desc* d) {
    IDB_REQUIRE(d, "%s: null descriptor", api);
    IDB_REQUIRE(conv_dims_ok(d->b, d->h, d->w, d->cin, d->cout, d->ksize, d->stride),
                "%s: b in 1..%d, h and w in 1..%d, cin 4 or %% 64 == 0 up to %d, cout %% 64 == 0 up to %d, ksize 1 or 3, stride 1 or 2", api,
                BLK_MAX_B, BLK_MAX_HW, BLK_MAX_C, BLK_MAX_C);
    IDB_REQUIRE(d->x && d->weight, "%s: null pointer", api);
    IDB_REQUIRE(idb_aligned16(d->x) && idb_aligned16(d->weight) && idb_aligned16(d->affine) && idb_aligned16(d->slope),
                "%s: x, weight, affine and slope 16-byte aligned", api);
    IDB_REQUIRE(!d->slope || d->affine, "%s: a PReLU slope without the BatchNorm's affine pair", api);
    return IDB_OK;
}

struct BnPlan {
    int per, slices;
    size_t part, cmean, total;
};

inline bool bn_dims_ok(long long rows, int ch) { return rows >= 1 && rows <= (long long)BLK_MAX_B * BLK_MAX_HW * BLK_MAX_HW && ch >= 64 && ch % 64 == 0 && ch <= BLK_MAX_C; }

// row slices of the statistics and of the backward's sums: 256 rows each, at most 1024 slices
BnPlan bn_plan(long long rows, int ch) {
    BnPlan p;
    long long ss = (rows + 255) / 256;
    if (ss > BLK_MAX_SSLICES) ss = BLK_MAX_SSLICES;
    p.per = (int)((rows + ss - 1) / ss);
    p.slices = (int)((rows + p.per - 1) / p.per);
    size_t o = 0;
    p.part = o, o += align256(sizeof(double) * 3 * (size_t)p.slices * ch);
    p.cmean = o, o += align256(sizeof(double) * 2 * (size_t)ch);
    p.total = o;
    return p;
}

}  // namespace

extern "C" size_t idb_blk_conv_workspace_bytes(int32_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ksize, int32_t stride,
                                               int32_t* wgrad_slices, int32_t* dgrad_row_tiles) {
    if (!conv_dims_ok(b, h, w, cin, cout, ksize, stride)) return 0;
    const ConvPlan p = conv_plan(conv_geo(b, h, w, cin, cout, ksize, stride));
    if (wgrad_slices) *wgrad_slices = p.slices;
    if (dgrad_row_tiles) *dgrad_row_tiles = p.dgrad_row_tiles;
    return p.total;
}

extern "C" int idb_blk_conv_forward(const idb_blk_conv_desc* d, float* out, void* stream) {
    const int rc = conv_check("idb_blk_conv_forward", d);
    if (rc != IDB_OK) return rc;
    IDB_REQUIRE(out && idb_aligned16(out), "idb_blk_conv_forward: out null or not 16-byte aligned");
    const ConvGeo g = conv_geo(d->b, d->h, d->w, d->cin, d->cout, d->ksize, d->stride);
    const ConvPlan p = conv_plan(g);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.fwd_row_tiles, g.cout / (32 * p.wn_out));
    if (p.wn_out == 4)
        hipLaunchKernelGGL(blk_conv_fwd_kernel<4>, grid, dim3(256), 0, st, d->x, d->affine, d->slope, d->weight, g, out);
    else
        hipLaunchKernelGGL(blk_conv_fwd_kernel<2>, grid, dim3(256), 0, st, d->x, d->affine, d->slope, d->weight, g, out);
    IDB_CHECK_LAUNCH("idb_blk_conv_forward");
    return IDB_OK;
}

extern "C" int idb_blk_conv_dgrad(const idb_blk_conv_desc* d, const float* g_out, float* g_in, void* stream) {
    const int rc = conv_check("idb_blk_conv_dgrad", d);
    if (rc != IDB_OK) return rc;
    IDB_REQUIRE(d->cin % 64 == 0, "idb_blk_conv_dgrad: cin %% 64 == 0 (the stem's image gradient is not built)");
    IDB_REQUIRE(g_out && g_in && idb_aligned16(g_out) && idb_aligned16(g_in), "idb_blk_conv_dgrad: g_out or g_in null or not 16-byte aligned");
    const ConvGeo g = conv_geo(d->b, d->h, d->w, d->cin, d->cout, d->ksize, d->stride);
    const ConvPlan p = conv_plan(g);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.dgrad_row_tiles, g.cin / (32 * p.wn_in), g.stride * g.stride);
    if (p.wn_in == 4)
        hipLaunchKernelGGL(blk_conv_dgrad_kernel<4>, grid, dim3(256), 0, st, g_out, d->weight, g, g_in);
    else
        hipLaunchKernelGGL(blk_conv_dgrad_kernel<2>, grid, dim3(256), 0, st, g_out, d->weight, g, g_in);
    IDB_CHECK_LAUNCH("idb_blk_conv_dgrad");
    return IDB_OK;
}

extern "C" int idb_blk_conv_wgrad(const idb_blk_conv_desc* d, const float* g_out, float* d_weight, void* ws, size_t ws_bytes, void* stream) {
    const int rc = conv_check("idb_blk_conv_wgrad", d);
    if (rc != IDB_OK) return rc;
    IDB_REQUIRE(g_out && d_weight && idb_aligned16(g_out), "idb_blk_conv_wgrad: g_out or d_weight null, or g_out not 16-byte aligned");
    const ConvGeo g = conv_geo(d->b, d->h, d->w, d->cin, d->cout, d->ksize, d->stride);
    const ConvPlan p = conv_plan(g);
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= p.total, "idb_blk_conv_wgrad: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.wgrad_row_tiles, p.wgrad_col_tiles, p.slices);
    if (p.wn_out == 4)
        hipLaunchKernelGGL(blk_conv_wgrad_kernel<4>, grid, dim3(256), 0, st, g_out, d->x, d->affine, d->slope, g, p.per, (float*)ws);
    else
        hipLaunchKernelGGL(blk_conv_wgrad_kernel<2>, grid, dim3(256), 0, st, g_out, d->x, d->affine, d->slope, g, p.per, (float*)ws);
    IDB_CHECK_LAUNCH("idb_blk_conv_wgrad");
    const long long total = (long long)g.cout * g.K;
    hipLaunchKernelGGL(blk_wgrad_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ws, p.slices, total, d_weight);
    IDB_CHECK_LAUNCH("idb_blk_conv_wgrad(merge)");
    return IDB_OK;
}

extern "C" size_t idb_blk_bn_workspace_bytes(int64_t rows, int32_t ch, int32_t* slices) {
    if (!bn_dims_ok(rows, ch)) return 0;
    const BnPlan p = bn_plan(rows, ch);
    if (slices) *slices = p.slices;
    return p.total;
}

extern "C" int idb_blk_bn_forward(const float* x, int64_t rows, int32_t ch, int32_t training, double eps, double momentum, const float* gamma,
                                  const float* beta, float* running_mean, float* running_var, double* stat, float* affine, int32_t* flags,
                                  void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(bn_dims_ok(rows, ch), "idb_blk_bn_forward: rows in 1..%d x %d x %d, ch %% 64 == 0 up to %d", BLK_MAX_B, BLK_MAX_HW, BLK_MAX_HW,
                BLK_MAX_C);
    IDB_REQUIRE(training == 0 || training == 1, "idb_blk_bn_forward: training must be 0 or 1");
    IDB_REQUIRE(!training || rows >= 2, "idb_blk_bn_forward: one value per channel in training mode (upstream's BatchNorm raises)");
    IDB_REQUIRE(eps >= 0.0 && eps <= 1.0 && momentum >= 0.0 && momentum <= 1.0, "idb_blk_bn_forward: eps in [0, 1], momentum in [0, 1]");
    IDB_REQUIRE(x && gamma && beta && running_mean && running_var && stat && affine && flags, "idb_blk_bn_forward: null pointer");
    IDB_REQUIRE(idb_aligned16(affine) && (((uintptr_t)stat) & 7) == 0, "idb_blk_bn_forward: affine 16-byte, stat 8-byte aligned");
    const BnPlan p = bn_plan(rows, ch);
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= p.total, "idb_blk_bn_forward: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)((char*)ws + p.part);
    if (training) {
        hipLaunchKernelGGL(blk_stats_kernel, dim3(ch / 64, p.slices), dim3(256), 0, st, x, (int)rows, ch, p.per, part);
        IDB_CHECK_LAUNCH("idb_blk_bn_forward(stats)");
    }
    hipLaunchKernelGGL(blk_bn_kernel, dim3(ch / 4), dim3(256), 0, st, x, (const double*)part, p.slices, (int)rows, ch, training, eps, momentum, gamma,
                       beta, running_mean, running_var, stat, affine, flags);
    IDB_CHECK_LAUNCH("idb_blk_bn_forward");
    return IDB_OK;
}

extern "C" int idb_blk_bn_backward(const float* c, const float* g, int64_t rows, int32_t ch, const double* stat, const float* affine,
                                   const float* gamma, const float* slope, const float* add, float* d_gamma, float* d_beta, float* d_slope,
                                   float* g_c, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(bn_dims_ok(rows, ch) && rows >= 2, "idb_blk_bn_backward: rows in 2..%d x %d x %d, ch %% 64 == 0 up to %d", BLK_MAX_B, BLK_MAX_HW,
                BLK_MAX_HW, BLK_MAX_C);
    IDB_REQUIRE(c && g && stat && affine && gamma && d_gamma && d_beta && g_c, "idb_blk_bn_backward: null pointer");
    IDB_REQUIRE((slope != nullptr) == (d_slope != nullptr), "idb_blk_bn_backward: slope and d_slope go together");
    IDB_REQUIRE(idb_aligned16(c) && idb_aligned16(g) && idb_aligned16(add) && idb_aligned16(g_c) && (((uintptr_t)stat) & 7) == 0,
                "idb_blk_bn_backward: c, g, add and g_c 16-byte, stat 8-byte aligned");
    const BnPlan p = bn_plan(rows, ch);
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= p.total, "idb_blk_bn_backward: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)((char*)ws + p.part);
    double* cmean = (double*)((char*)ws + p.cmean);
    hipLaunchKernelGGL(blk_bnbwd_sums_kernel, dim3(ch / 64, p.slices), dim3(256), 0, st, c, g, affine, stat, slope, (int)rows, ch, p.per, part);
    IDB_CHECK_LAUNCH("idb_blk_bn_backward(sums)");
    hipLaunchKernelGGL(blk_bnbwd_finish_kernel, dim3(ch / 4), dim3(256), 0, st, (const double*)part, p.slices, (int)rows, ch, d_gamma, d_beta, d_slope,
                       cmean);
    IDB_CHECK_LAUNCH("idb_blk_bn_backward(finish)");
    const long long total4 = rows * ch / 4;
    hipLaunchKernelGGL(blk_bnbwd_apply_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, c, g, affine, stat, (const double*)cmean, gamma,
                       slope, add, total4, ch, g_c);
    IDB_CHECK_LAUNCH("idb_blk_bn_backward(apply)");
    return IDB_OK;
}

extern "C" int idb_blk_affine(const float* c, const float* affine, const float* slope, const float* identity, const float* id_affine, int64_t rows,
                              int32_t ch, float* out, void* stream) {
    IDB_REQUIRE(bn_dims_ok(rows, ch), "idb_blk_affine: rows in 1..%d x %d x %d, ch %% 64 == 0 up to %d", BLK_MAX_B, BLK_MAX_HW, BLK_MAX_HW, BLK_MAX_C);
    IDB_REQUIRE(c && affine && out, "idb_blk_affine: null pointer");
    IDB_REQUIRE(!id_affine || identity, "idb_blk_affine: an identity affine pair without the identity");
    IDB_REQUIRE(idb_aligned16(c) && idb_aligned16(affine) && idb_aligned16(slope) && idb_aligned16(identity) && idb_aligned16(id_affine) &&
                    idb_aligned16(out),
                "idb_blk_affine: every pointer 16-byte aligned");
    const long long total4 = rows * ch / 4;
    hipLaunchKernelGGL(blk_affine_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, affine, slope, identity,
                       id_affine, total4, ch, out);
    IDB_CHECK_LAUNCH("idb_blk_affine");
    return IDB_OK;
}

extern "C" int idb_blk_pack_images(const float* images, int32_t b, int32_t h, int32_t w, float* out, void* stream) {
    IDB_REQUIRE(b >= 1 && b <= BLK_MAX_B && h >= 1 && h <= BLK_MAX_HW && w >= 1 && w <= BLK_MAX_HW, "idb_blk_pack_images: b in 1..%d, h and w in 1..%d",
                BLK_MAX_B, BLK_MAX_HW);
    IDB_REQUIRE(images && out && idb_aligned16(out), "idb_blk_pack_images: null pointer, or out not 16-byte aligned");
    const long long pixels = (long long)b * h * w;
    hipLaunchKernelGGL(blk_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images, pixels, h * w, out);
    IDB_CHECK_LAUNCH("idb_blk_pack_images");
    return IDB_OK;
}
