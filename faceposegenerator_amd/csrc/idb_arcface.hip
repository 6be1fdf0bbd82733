// ArcFace IResNet (insightface arcface_torch iresnet.py, the identity network of ID-Booth's embedding extraction, genuine/impostor
// scoring and identity loss): the two pieces that are not implicit GEMMs.  The 49 residual blocks run on idb_gemm (PReLU epilogue,
// strided 1x1 shortcut segment, affine second output); faceposegenerator_amd/arcface.py drives them.
//   stem: conv1 3->64 (3x3, stride 1, pad 1) with bn1 folded, PReLU — 3 input channels, ~43 MFLOP per face: VALU work
//   head: [B][K] operand-dtype activations x fp32 [N][K] (bn2 + fc + features folded into one matrix) -> fp32 [B][N]
#include "idb_common.h"

namespace {

constexpr int STEM_C = 64, STEM_MAXW = 256;

// One workgroup per (output row, image).  The three input rows the row needs are normalised ((u8 / 255 - 0.5) / 0.5 for uint8 NHWC
// crops; fp32 NCHW taken as is), rounded to the operand dtype (autocast casts the input before the conv) and staged in LDS with the
// zero padding; each thread then owns 8 output channels of one pixel: 27 taps x 8 FMAs in fp32, PReLU, one rounding, and the second
// output fma(rounded, out2_scale, out2_shift) rounded once (the next block's bn1, as idb_gemm_desc.out2).
template <typename T, bool U8>
__global__ __launch_bounds__(256) void arcface_stem_kernel(const void* __restrict__ x, int H, int W, const float* __restrict__ wgt,
                                                           const float* __restrict__ bias, const float* __restrict__ slope,
                                                           const float* __restrict__ s2, const float* __restrict__ b2, T* __restrict__ out,
                                                           T* __restrict__ out2) {
    using V8 = typename Op<T>::v8;
    __shared__ float sw[STEM_C * 27];
    __shared__ float sx[3][STEM_MAXW + 2][3];
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < STEM_C * 27; i += 256) sw[i] = wgt[i];
    const int row_elems = (W + 2) * 3;
    for (int i = tid; i < 3 * row_elems; i += 256) {
        const int r = i / row_elems, rem = i - r * row_elems, px = rem / 3, c = rem - px * 3;
        const int iy = y - 1 + r, ix = px - 1;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            if constexpr (U8) {
                const float u = (float)((const uint8_t*)x)[(((long long)b * H + iy) * W + ix) * 3 + c];
                v = (u / 255.f - 0.5f) / 0.5f;
            } else {
                v = ((const float*)x)[(((long long)b * 3 + c) * H + iy) * W + ix];
            }
            v = to_f32<T>(from_f32<T>(v));
        }
        sx[r][px][c] = v;
    }
    __syncthreads();
    for (int t = tid; t < W * 8; t += 256) {
        const int px = t >> 3, c0 = (t & 7) * 8;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = bias[c0 + k];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float xv = sx[ky][px + kx][ci];
                    const int tap = (ky * 3 + kx) * 3 + ci;
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(xv, sw[(c0 + k) * 27 + tap], acc[k]);
                }
        V8 o, o2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = acc[k] >= 0.f ? acc[k] : acc[k] * slope[c0 + k];
            o[k] = from_f32<T>(v);
            if (out2) o2[k] = affine_round<T>(to_f32<T>(o[k]), s2[c0 + k], b2[c0 + k]);
        }
        const long long off = (((long long)b * H + y) * W + px) * STEM_C + c0;
        *(V8*)(out + off) = o;
        if (out2) *(V8*)(out2 + off) = o2;
    }
}

// Head: partial[z][m][n] = sum over K-slice z of x[m][k] * w[n][k], fp32, 64 x 64 tiles, 256 threads with 4 x 4 outputs each, 32-deep
// K chunks through LDS; then head_reduce adds the slices in ascending order plus the bias (deterministic, no atomics).
constexpr int HT = 64, HK = 32;
template <typename T>
__global__ __launch_bounds__(256) void arcface_head_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ partial,
                                                           int M, int N, int K, int chunks_per_split) {
    __shared__ float xs[HK][HT + 4];
    __shared__ float ws[HK][HT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * HT, n0 = blockIdx.y * HT, z = blockIdx.z;
    const int nchunks = K / HK;
    const int c_begin = z * chunks_per_split;
    const int c_end = min(nchunks, c_begin + chunks_per_split);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    // loader mapping: 64 rows x 32 k = 2048 values per operand, 8 per thread: row = tid / 4, k = (tid % 4) * 8 .. + 7
    const int lr = tid >> 2, lk = (tid & 3) * 8;
    for (int c = c_begin; c < c_end; ++c) {
        const int k0 = c * HK + lk;
        const int mr = m0 + lr, nr = n0 + lr;
        float xv[8], wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xv[e] = mr < M ? to_f32<T>(x[(long long)mr * K + k0 + e]) : 0.f;
            wv[e] = nr < N ? w[(long long)nr * K + k0 + e] : 0.f;
        }
        __syncthreads();                                          // the previous chunk's reads are done
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xs[lk + e][lr] = xv[e];
            ws[lk + e][lr] = wv[e];
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < HK; ++kk) {
            const f32x4 a = *(const f32x4*)&xs[kk][ty * 4];
            const f32x4 bb = *(const f32x4*)&ws[kk][tx * 4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], bb[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m < M) *(f32x4*)(partial + ((long long)z * M + m) * N + n0 + tx * 4) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    }
}

__global__ __launch_bounds__(256) void arcface_head_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                                                  float* __restrict__ y, int M, int N, int splits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * N) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += partial[(long long)z * M * N + i];
    y[i] = s + (bias ? bias[i % N] : 0.f);
}

int head_splits(int m, int n, int k) {
    const int tiles = ((m + HT - 1) / HT) * (n / HT);
    int s = (512 + tiles - 1) / tiles;                            // about two workgroups per CU
    const int nchunks = k / HK;
    if (s > nchunks / 8) s = nchunks / 8;                         // at least 8 K chunks per workgroup
    if (s < 1) s = 1;
    const int per = (nchunks + s - 1) / s;
    return (nchunks + per - 1) / per;                             // no empty slice
}

}  // namespace

extern "C" int idb_arcface_stem(const void* x, int32_t x_u8, int32_t batch, int32_t h, int32_t w, const float* weight, const float* bias,
                                const float* slope, const float* out2_scale, const float* out2_shift, void* out, void* out2, int32_t dtype,
                                void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_arcface_stem: dtype must be bf16/f16");
    IDB_REQUIRE(x && weight && bias && slope && out && idb_aligned16(out) && (!out2 || idb_aligned16(out2)),
                "idb_arcface_stem: null or unaligned pointer");
    IDB_REQUIRE(!out2 || (out2_scale && out2_shift), "idb_arcface_stem: out2 needs out2_scale and out2_shift");
    IDB_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0 && w <= STEM_MAXW, "idb_arcface_stem: batch 1..65535, width 1..256");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(h, batch);
#define IDB_STEM(T, U)                                                                                                       \
    hipLaunchKernelGGL((arcface_stem_kernel<T, U>), grid, dim3(256), 0, st, x, h, w, weight, bias, slope, out2_scale, out2_shift, \
                       (T*)out, (T*)out2)
    if (dtype == IDB_BF16) {
        if (x_u8) IDB_STEM(__bf16, true);
        else IDB_STEM(__bf16, false);
    } else {
        if (x_u8) IDB_STEM(_Float16, true);
        else IDB_STEM(_Float16, false);
    }
#undef IDB_STEM
    IDB_CHECK_LAUNCH("idb_arcface_stem");
    return IDB_OK;
}

extern "C" size_t idb_arcface_head_workspace_bytes(int32_t m, int32_t n, int32_t k) {
    if (m <= 0 || n <= 0 || n % HT || k <= 0 || k % HK) return 0;
    return (size_t)head_splits(m, n, k) * m * n * sizeof(float);
}

extern "C" int idb_arcface_head(const void* x, const float* w, const float* bias, float* y, int32_t m, int32_t n, int32_t k, int32_t dtype,
                                void* workspace, size_t workspace_bytes, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_arcface_head: dtype must be bf16/f16");
    IDB_REQUIRE(x && w && y && m > 0 && n > 0 && n % HT == 0 && k > 0 && k % HK == 0, "idb_arcface_head: n %% 64 == 0 and k %% 32 == 0 required");
    const int splits = head_splits(m, n, k);
    const size_t need = (size_t)splits * m * n * sizeof(float);
    IDB_REQUIRE(workspace && workspace_bytes >= need && idb_aligned16(workspace), "idb_arcface_head: workspace too small (%zu < %zu)",
                workspace_bytes, need);
    const int per = (k / HK + splits - 1) / splits;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((m + HT - 1) / HT, n / HT, splits);
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((arcface_head_kernel<__bf16>), grid, dim3(256), 0, st, (const __bf16*)x, w, (float*)workspace, m, n, k, per);
    else
        hipLaunchKernelGGL((arcface_head_kernel<_Float16>), grid, dim3(256), 0, st, (const _Float16*)x, w, (float*)workspace, m, n, k, per);
    IDB_CHECK_LAUNCH("idb_arcface_head");
    hipLaunchKernelGGL(arcface_head_reduce_kernel, dim3((unsigned)(((long long)m * n + 255) / 256)), dim3(256), 0, st, (const float*)workspace,
                       bias, y, m, n, splits);
    IDB_CHECK_LAUNCH("idb_arcface_head_reduce");
    return IDB_OK;
}
