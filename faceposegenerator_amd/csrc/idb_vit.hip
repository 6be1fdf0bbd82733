// DINOv2 ViT image encoder (facebookresearch/dinov2 vision_transformer.py DinoVisionTransformer; the `--model dinov2` encoder of the
// dgm-eval run in ID-Booth's Evaluation/dgm-eval notebook): the pieces around the transformer blocks.  The blocks themselves run on
// idb_layernorm, idb_gemm (bias / exact-GELU / residual epilogues, LayerScale folded into the weights) and idb_attention;
// faceposegenerator_amd/dinov2.py drives them.
//   patchify: PatchEmbed's 14x14 stride-14 conv as a GEMM operand — one row of 3*14*14 = 588 values per patch, zero-padded to 640
//   tokens:   cat(cls_token, patches) + pos_embed (prepare_tokens_with_masks without masks)
//   head:     the final LayerNorm on the class token alone (x_norm_clstoken; head = Identity), fp32
#include "idb_common.h"

namespace {

constexpr int VP_SIZE = 224, VP_PATCH = 14, VP_GRID = VP_SIZE / VP_PATCH, VP_K = 3 * VP_PATCH * VP_PATCH, VP_KPAD = 640;

// One workgroup per (patch row, image): 16 patches x 640 columns = 1280 vectors of 8, five per thread.  Column k < 588 of patch
// (py, px) is pixel (14 py + ky, 14 px + kx) of channel c with k = (c * 14 + ky) * 14 + kx — the flattening of the conv weight
// [D][3][14][14]; columns 588..639 are zero.  uint8 NHWC input is normalised in fp32 as ToTensor + Normalize do
// ((u / 255 - mean) / std); either way the fp32 value is rounded once to the operand dtype.
template <typename T, bool U8>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const void* __restrict__ x, T* __restrict__ out) {
    using V8 = typename Op<T>::v8;
    const int py = blockIdx.x, b = blockIdx.y;
    constexpr int VEC_PER_ROW = VP_KPAD / 8;
    for (int v = threadIdx.x; v < VP_GRID * VEC_PER_ROW; v += 256) {
        const int px = v / VEC_PER_ROW, k0 = (v - px * VEC_PER_ROW) * 8;
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            float val = 0.f;
            if (k < VP_K) {
                const int c = k / (VP_PATCH * VP_PATCH), r = k - c * (VP_PATCH * VP_PATCH), ky = r / VP_PATCH, kx = r - ky * VP_PATCH;
                const int iy = py * VP_PATCH + ky, ix = px * VP_PATCH + kx;
                if constexpr (U8) {
                    const float u = (float)((const uint8_t*)x)[(((long long)b * VP_SIZE + iy) * VP_SIZE + ix) * 3 + c];
                    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f;
                    const float stdv = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
                    val = (u / 255.f - mean) / stdv;
                } else {
                    val = ((const float*)x)[(((long long)b * 3 + c) * VP_SIZE + iy) * VP_SIZE + ix];
                }
            }
            o[e] = from_f32<T>(val);
        }
        *(V8*)(out + ((long long)(b * VP_GRID + py) * VP_GRID + px) * VP_KPAD + k0) = o;
    }
}

// One thread per 8 output elements of [batch][1 + n][dim].  fp32 add of the fp32 tables, one rounding.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const T* __restrict__ patches, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, T* __restrict__ out, long long vecs, int n, int dim) {
    using V8 = typename Op<T>::v8;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= vecs) return;
    const int vpr = dim / 8;
    const long long row = v / vpr;
    const int d0 = (int)(v - row * vpr) * 8;
    const long long b = row / (n + 1);
    const int t = (int)(row - b * (n + 1));
    const f32x4 p0 = *(const f32x4*)(pos + (long long)t * dim + d0), p1 = *(const f32x4*)(pos + (long long)t * dim + d0 + 4);
    float a[8];
    if (t == 0) {
        const f32x4 c0 = *(const f32x4*)(cls + d0), c1 = *(const f32x4*)(cls + d0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = c0[e];
            a[e + 4] = c1[e];
        }
    } else {
        const V8 pv = *(const V8*)(patches + (b * n + (t - 1)) * dim + d0);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = to_f32<T>(pv[e]);
    }
    V8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o[e] = from_f32<T>(a[e] + p0[e]);
        o[e + 4] = from_f32<T>(a[e + 4] + p1[e]);
    }
    *(V8*)(out + row * dim + d0) = o;
}

// Block-wide sum in a fixed order: the shuffle tree of each wave, then the four wave sums left to right; every thread gets the result.
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per image: nn.LayerNorm over row b * row_stride of x in fp32, two passes (mean, then the variance of x - mean), a true
// division by dim so that a constant row has an exact mean.  Thread t owns elements t, t + 256, ...
template <typename T>
__global__ __launch_bounds__(256) void vit_head_kernel(const T* __restrict__ x, long long row_stride, int dim, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, float* __restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const T* xr = x + (long long)b * row_stride * dim;
    float s = 0.f;
    for (int i = tid; i < dim; i += 256) s += to_f32<T>(xr[i]);
    const float mean = block_sum256(s, red) / (float)dim;
    float q = 0.f;
    for (int i = tid; i < dim; i += 256) {
        const float d = to_f32<T>(xr[i]) - mean;
        q = __builtin_fmaf(d, d, q);
    }
    const float var = block_sum256(q, red) / (float)dim;
    const float rstd = 1.0f / sqrtf(var + eps);
    for (int i = tid; i < dim; i += 256) out[(long long)b * dim + i] = (to_f32<T>(xr[i]) - mean) * rstd * gamma[i] + beta[i];
}

}  // namespace

extern "C" int idb_vit_patchify(const void* x, int32_t x_u8, int32_t batch, void* out, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_vit_patchify: dtype must be bf16/f16");
    IDB_REQUIRE(x && out && idb_aligned16(out), "idb_vit_patchify: null or unaligned pointer");
    IDB_REQUIRE(batch > 0 && batch <= 65535, "idb_vit_patchify: batch 1..65535");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(VP_GRID, batch);
#define IDB_VPATCH(T, U) hipLaunchKernelGGL((vit_patchify_kernel<T, U>), grid, dim3(256), 0, st, x, (T*)out)
    if (dtype == IDB_BF16) {
        if (x_u8) IDB_VPATCH(__bf16, true);
        else IDB_VPATCH(__bf16, false);
    } else {
        if (x_u8) IDB_VPATCH(_Float16, true);
        else IDB_VPATCH(_Float16, false);
    }
#undef IDB_VPATCH
    IDB_CHECK_LAUNCH("idb_vit_patchify");
    return IDB_OK;
}

extern "C" int idb_vit_tokens(const void* patches, const float* cls, const float* pos, void* out, int32_t batch, int32_t n_patches,
                              int32_t dim, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_vit_tokens: dtype must be bf16/f16");
    IDB_REQUIRE(patches && cls && pos && out && idb_aligned16(patches) && idb_aligned16(cls) && idb_aligned16(pos) && idb_aligned16(out),
                "idb_vit_tokens: null or unaligned pointer");
    IDB_REQUIRE(batch > 0 && n_patches > 0 && dim > 0 && dim % 8 == 0, "idb_vit_tokens: batch > 0, n_patches > 0, dim %% 8 == 0");
    const long long vecs = (long long)batch * (n_patches + 1LL) * (dim / 8);
    const long long blocks = (vecs + 255) / 256;
    IDB_REQUIRE(blocks < (1LL << 31), "idb_vit_tokens: grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((vit_tokens_kernel<__bf16>), dim3((unsigned)blocks), dim3(256), 0, st, (const __bf16*)patches, cls, pos, (__bf16*)out,
                           vecs, n_patches, dim);
    else
        hipLaunchKernelGGL((vit_tokens_kernel<_Float16>), dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)patches, cls, pos,
                           (_Float16*)out, vecs, n_patches, dim);
    IDB_CHECK_LAUNCH("idb_vit_tokens");
    return IDB_OK;
}

extern "C" int idb_vit_head(const void* x, int64_t row_stride, int32_t batch, int32_t dim, const float* gamma, const float* beta, float eps,
                            float* out, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_vit_head: dtype must be bf16/f16");
    IDB_REQUIRE(x && gamma && beta && out, "idb_vit_head: null pointer");
    IDB_REQUIRE(batch > 0 && batch <= 65535 && dim > 0 && row_stride > 0 && eps > 0.f &&
                    (long long)batch * row_stride < (1LL << 40) / dim,
                "idb_vit_head: batch 1..65535, dim > 0, row_stride > 0, eps > 0");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((vit_head_kernel<__bf16>), dim3(batch), dim3(256), 0, st, (const __bf16*)x, (long long)row_stride, dim, gamma, beta,
                           eps, out);
    else
        hipLaunchKernelGGL((vit_head_kernel<_Float16>), dim3(batch), dim3(256), 0, st, (const _Float16*)x, (long long)row_stride, dim, gamma,
                           beta, eps, out);
    IDB_CHECK_LAUNCH("idb_vit_head");
    return IDB_OK;
}
