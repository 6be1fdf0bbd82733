// The bandwidth-bound kernels a LoRA transformer block's training adds to the attention modules (faceposegenerator_amd/lorablock.py):
// LayerNorm's input gradient, and GEGLU forward and backward as launches of their own (the backward needs the projection's raw
// output, which the inference GEMM's fused GEGLU epilogue never stores).  f16 / bf16 operands, fp32 arithmetic, every result rounded
// once; no atomics, no workgroup waits for another, every sum in an order the shape alone decides.
//   layernorm_bwd  one wave per row, the row in registers (C <= 1536 = NCH x 64 lanes x 8), as layernorm_kernel: x, dy, add and gamma
//                  are requested together from clamped addresses, mean and rstd are recomputed with layernorm_kernel's own arithmetic
//                  (two-pass variance, the same wave sums), then g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ add).
//                  A wave has read its whole rows before it stores, so dx may be add or dy.
//   geglu_fwd/bwd  one 8-vector of value and of gate per thread, 256 vectors per workgroup, the last workgroup partial.
#include "idb_common.h"
#include <math.h>

namespace {

template <typename T, int NCH>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* x, const T* dy, const T* add, const float* gamma, T* dx, long long rows, int C,
                                                            float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int Ct = C >> 3;
    typename Op<T>::v8 raw[NCH], rdy[NCH], radd[NCH];
    f32x4 g0[NCH], g1[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int cc = min(lane + i * 64, Ct - 1);
        raw[i] = *(const typename Op<T>::v8*)(x + row * C + cc * 8);
        rdy[i] = *(const typename Op<T>::v8*)(dy + row * C + cc * 8);
        if (add) radd[i] = *(const typename Op<T>::v8*)(add + row * C + cc * 8);
        g0[i] = *(const f32x4*)(gamma + cc * 8);
        g1[i] = *(const f32x4*)(gamma + cc * 8 + 4);
    }
    // the forward's statistics, with the forward's arithmetic
    float v[NCH][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const bool in = lane + i * 64 < Ct;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] = in ? to_f32<T>(raw[i][e]) : 0.f;
            sum += v[i][e];
        }
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        if (lane + i * 64 < Ct) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[i][e] - mean;
                sq += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
    // g = dy gamma and xhat in place of dy and x; the two row means over the C real elements (lanes past the row hold clamped copies
    // and are left out)
    float g[NCH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const bool in = lane + i * 64 < Ct;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gm = e < 4 ? g0[i][e] : g1[i][e - 4];
            g[i][e] = in ? to_f32<T>(rdy[i][e]) * gm : 0.f;
            v[i][e] = in ? (v[i][e] - mean) * rstd : 0.f;
            s1 += g[i][e];
            s2 += g[i][e] * v[i][e];
        }
    }
    const float mg = wave_sum(s1) / (float)C, mgx = wave_sum(s2) / (float)C;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int cc = lane + i * 64;
        if (cc < Ct) {
            typename Op<T>::v8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float r = rstd * (g[i][e] - mg - v[i][e] * mgx);
                if (add) r += to_f32<T>(radd[i][e]);
                o[e] = from_f32<T>(r);
            }
            *(typename Op<T>::v8*)(dx + row * C + cc * 8) = o;
        }
    }
}

// gelu_erf_f's cumulative normal (the same operations in the same order, so x * cdf is gelu_erf_f(x)) and the density, which shares
// the exponential: exp(-z^2) with z = |x| / sqrt 2 is exp(-x^2 / 2)
__device__ __forceinline__ void normal_cdf_pdf(float x, float& cdf, float& pdf) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
    float poly = 1.061405429f;
    poly = poly * t - 1.453152027f;
    poly = poly * t + 1.421413741f;
    poly = poly * t - 0.284496736f;
    poly = poly * t + 0.254829592f;
    const float e = __expf(-z * z);
    const float erfc_z = poly * t * e;
    cdf = x >= 0.f ? 1.0f - 0.5f * erfc_z : 0.5f * erfc_z;
    pdf = 0.3989422804014327f * e;
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const T* __restrict__ hg, int hg_ld, T* __restrict__ out, unsigned total, unsigned vec_per_row) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned row = i / vec_per_row, col = (i - row * vec_per_row) * 8u;
    const T* p = hg + (long long)row * hg_ld + col;
    const typename Op<T>::v8 val = *(const typename Op<T>::v8*)p;
    const typename Op<T>::v8 gate = *(const typename Op<T>::v8*)(p + vec_per_row * 8u);
    typename Op<T>::v8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(to_f32<T>(val[e]) * gelu_erf_f(to_f32<T>(gate[e])));
    *(typename Op<T>::v8*)(out + (long long)i * 8) = o;
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ hg, int hg_ld, const T* __restrict__ dout, T* __restrict__ dhg, unsigned total,
                                                        unsigned vec_per_row) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const unsigned row = i / vec_per_row, col = (i - row * vec_per_row) * 8u;
    const unsigned inner = vec_per_row * 8u;
    const T* p = hg + (long long)row * hg_ld + col;
    const typename Op<T>::v8 val = *(const typename Op<T>::v8*)p;
    const typename Op<T>::v8 gate = *(const typename Op<T>::v8*)(p + inner);
    const typename Op<T>::v8 d = *(const typename Op<T>::v8*)(dout + (long long)i * 8);
    typename Op<T>::v8 dv, dg;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gt = to_f32<T>(gate[e]), go = to_f32<T>(d[e]);
        float cdf, pdf;
        normal_cdf_pdf(gt, cdf, pdf);
        dv[e] = from_f32<T>(go * (gt * cdf));
        dg[e] = from_f32<T>(go * to_f32<T>(val[e]) * (cdf + gt * pdf));
    }
    T* q = dhg + (long long)row * 2 * inner + col;
    *(typename Op<T>::v8*)q = dv;
    *(typename Op<T>::v8*)(q + inner) = dg;
}

// rows x inner / 8 vectors in a 32-bit index and a grid of 256-vector workgroups
int geglu_check(const char* api, int64_t rows, int32_t inner, const void* hg, int32_t hg_ld) {
    IDB_REQUIRE(rows > 0, "%s: rows must be positive", api);
    IDB_REQUIRE(inner > 0 && inner % 8 == 0 && inner <= (1 << 28), "%s: inner must be a positive multiple of 8 (16-byte vectors)", api);
    IDB_REQUIRE(hg_ld >= 2 * (int64_t)inner && hg_ld % 8 == 0, "%s: hg_ld must be at least 2 * inner and a multiple of 8 elements (16 bytes)", api);
    IDB_REQUIRE(rows <= (1ll << 31) / (inner / 8) - 1, "%s: rows * inner too large (rows * inner / 8 must stay below 2^31)", api);
    return IDB_OK;
}

}  // namespace

extern "C" int idb_layernorm_bwd(const void* x, const void* dy, const void* add, const float* gamma, void* dx, int64_t rows, int32_t c, float eps,
                                 int32_t dtype, void* stream) {
    const char* api = "idb_layernorm_bwd";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be f16 or bf16", api);
        return IDB_EUNSUPPORTED;
    }
    const void* ptrs[] = {x, dy, gamma, dx};
    const char* names[] = {"x", "dy", "gamma", "dx"};
    for (int i = 0; i < 4; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        IDB_REQUIRE(idb_aligned16(ptrs[i]), "%s: %s is not aligned (16 bytes)", api, names[i]);
    }
    IDB_REQUIRE(idb_aligned16(add), "%s: add is not aligned (16 bytes)", api);
    IDB_REQUIRE(rows > 0, "%s: rows must be positive", api);
    IDB_REQUIRE(c > 0 && c % 8 == 0 && c <= 1536, "%s: c=%d unsupported (a multiple of 8, at most 1536)", api, c);
    IDB_REQUIRE(eps > 0.f && eps < INFINITY, "%s: eps must be positive and finite", api);
    const long long blocks = (rows + 3) / 4;
    IDB_REQUIRE(blocks < (1LL << 31), "%s: rows too large for the grid", api);
    // dx may be add or dy exactly (the same rows); any other overlap with an input would be read after another wave's store
    const size_t bytes = (size_t)rows * c * 2;
    auto overlaps = [&](const void* a, size_t na, const void* b, size_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    IDB_REQUIRE(!overlaps(dx, bytes, x, bytes), "%s: dx aliases x", api);
    IDB_REQUIRE(!overlaps(dx, bytes, gamma, (size_t)c * 4), "%s: dx aliases gamma", api);
    IDB_REQUIRE(dx == dy || !overlaps(dx, bytes, dy, bytes), "%s: dx aliases dy partially (dx may be dy itself)", api);
    IDB_REQUIRE(!add || dx == add || !overlaps(dx, bytes, add, bytes), "%s: dx aliases add partially (dx may be add itself)", api);
    hipStream_t st = (hipStream_t)stream;
    const int nch = (c / 8 + 63) / 64;
#define IDB_LNB_LAUNCH(TT, N)                                                                                                                 \
    hipLaunchKernelGGL((layernorm_bwd_kernel<TT, N>), dim3((unsigned)blocks), dim3(256), 0, st, (const TT*)x, (const TT*)dy, (const TT*)add, gamma, \
                       (TT*)dx, (long long)rows, c, eps)
    if (dtype == IDB_BF16) {
        if (nch == 1) IDB_LNB_LAUNCH(__bf16, 1); else if (nch == 2) IDB_LNB_LAUNCH(__bf16, 2); else IDB_LNB_LAUNCH(__bf16, 3);
    } else {
        if (nch == 1) IDB_LNB_LAUNCH(_Float16, 1); else if (nch == 2) IDB_LNB_LAUNCH(_Float16, 2); else IDB_LNB_LAUNCH(_Float16, 3);
    }
#undef IDB_LNB_LAUNCH
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

extern "C" int idb_geglu_fwd(const void* hg, int32_t hg_ld, void* out, int64_t rows, int32_t inner, int32_t dtype, void* stream) {
    const char* api = "idb_geglu_fwd";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be f16 or bf16", api);
        return IDB_EUNSUPPORTED;
    }
    IDB_REQUIRE(hg, "%s: hg is null", api);
    IDB_REQUIRE(out, "%s: out is null", api);
    IDB_REQUIRE(idb_aligned16(hg), "%s: hg is not aligned (16 bytes)", api);
    IDB_REQUIRE(idb_aligned16(out), "%s: out is not aligned (16 bytes)", api);
    if (int rc = geglu_check(api, rows, inner, hg, hg_ld)) return rc;
    const size_t in_bytes = ((size_t)(rows - 1) * hg_ld + 2 * (size_t)inner) * 2, out_bytes = (size_t)rows * inner * 2;
    IDB_REQUIRE(!((uintptr_t)out < (uintptr_t)hg + in_bytes && (uintptr_t)hg < (uintptr_t)out + out_bytes), "%s: out aliases hg", api);
    const unsigned vpr = inner / 8, total = (unsigned)(rows * vpr);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((geglu_fwd_kernel<__bf16>), dim3((total + 255) / 256), dim3(256), 0, st, (const __bf16*)hg, hg_ld, (__bf16*)out, total, vpr);
    else
        hipLaunchKernelGGL((geglu_fwd_kernel<_Float16>), dim3((total + 255) / 256), dim3(256), 0, st, (const _Float16*)hg, hg_ld, (_Float16*)out, total,
                           vpr);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

extern "C" int idb_geglu_bwd(const void* hg, int32_t hg_ld, const void* dout, void* dhg, int64_t rows, int32_t inner, int32_t dtype, void* stream) {
    const char* api = "idb_geglu_bwd";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be f16 or bf16", api);
        return IDB_EUNSUPPORTED;
    }
    const void* ptrs[] = {hg, dout, dhg};
    const char* names[] = {"hg", "dout", "dhg"};
    for (int i = 0; i < 3; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        IDB_REQUIRE(idb_aligned16(ptrs[i]), "%s: %s is not aligned (16 bytes)", api, names[i]);
    }
    if (int rc = geglu_check(api, rows, inner, hg, hg_ld)) return rc;
    const size_t in_bytes = ((size_t)(rows - 1) * hg_ld + 2 * (size_t)inner) * 2, d_bytes = (size_t)rows * inner * 2;
    auto overlaps = [&](const void* a, size_t na, const void* b, size_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    IDB_REQUIRE(!overlaps(dhg, 2 * d_bytes, hg, in_bytes), "%s: dhg aliases hg", api);
    IDB_REQUIRE(!overlaps(dhg, 2 * d_bytes, dout, d_bytes), "%s: dhg aliases dout", api);
    const unsigned vpr = inner / 8, total = (unsigned)(rows * vpr);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((geglu_bwd_kernel<__bf16>), dim3((total + 255) / 256), dim3(256), 0, st, (const __bf16*)hg, hg_ld, (const __bf16*)dout,
                           (__bf16*)dhg, total, vpr);
    else
        hipLaunchKernelGGL((geglu_bwd_kernel<_Float16>), dim3((total + 255) / 256), dim3(256), 0, st, (const _Float16*)hg, hg_ld, (const _Float16*)dout,
                           (_Float16*)dhg, total, vpr);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}
