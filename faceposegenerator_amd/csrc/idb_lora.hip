// LoRA adapter gradients of one linear layer y = W x + scale B (A x) (peft lora.Linear: lora_a [rank][in], lora_b [out][rank], fp32):
//   db = scale dy^T (x A^T)      [out][rank]
//   da = scale (dy B)^T x        [rank][in]
// The out x in weight gradient dy^T x is never formed: both results factor through the [m][rank] projections u = x A^T and t = dy B.
//   lora_proj    one wave per row: u and t in fp32, [m][16] each (columns past the rank are 0).
//   lora_outer   one thread per column PAIR of x | dy and one row chunk: 16 x 2 fp32 accumulators, the rows in ascending order; partial
//                sums [chunk][rank][in + out].  x and dy are read a second time here; the first read left them in the Infinity Cache at
//                every SD-2.1 shape (at most 10 MB each).
//   lora_merge   the chunks in ascending order in double, times scale, rounded once to fp32.
// No atomics: bit-identical from run to run.
#include "idb_common.h"

namespace {

constexpr int RMAX = IDB_LORA_MAX_RANK;           // 16
constexpr int CHUNK_ROWS = IDB_LORA_GRAD_CHUNK_ROWS, MAX_CHUNKS = IDB_LORA_GRAD_MAX_CHUNKS;

struct GradPlan {
    int chunk_rows, chunks;
    size_t proj_bytes, part_bytes;
};

GradPlan grad_plan(long long m, int in, int out, int rank) {
    GradPlan p;
    const long long cr = m <= (long long)CHUNK_ROWS * MAX_CHUNKS ? CHUNK_ROWS : (m + MAX_CHUNKS - 1) / MAX_CHUNKS;
    p.chunk_rows = (int)cr;
    p.chunks = (int)((m + cr - 1) / cr);
    p.proj_bytes = (size_t)m * RMAX * 4 * 2;
    p.part_bytes = (size_t)p.chunks * rank * (in + out) * 4;
    return p;
}

template <typename T>
__global__ __launch_bounds__(256) void lora_grad_proj_kernel(const T* __restrict__ x, int x_ld, const T* __restrict__ dy, int dy_ld,
                                                       const float* __restrict__ la, const float* __restrict__ lb, float* __restrict__ u,
                                                       float* __restrict__ t, int m, int in, int out, int rank) {
    using V8 = typename Op<T>::v8;
    const int lane = threadIdx.x & 63;
    const int row = min(blockIdx.x * 4 + (threadIdx.x >> 6), m - 1);       // a surplus wave repeats the last row (same values, same stores)
    float au[RMAX], at[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) au[r] = at[r] = 0.f;
    for (int i = lane * 8; i < in; i += 512) {
        const V8 xv = *(const V8*)(x + (long long)row * x_ld + i);
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
            if (r < rank) {
                const f32x4 a0 = *(const f32x4*)(la + (long long)r * in + i), a1 = *(const f32x4*)(la + (long long)r * in + i + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    au[r] = __builtin_fmaf(to_f32<T>(xv[j]), a0[j], au[r]);
                    au[r] = __builtin_fmaf(to_f32<T>(xv[j + 4]), a1[j], au[r]);
                }
            }
    }
    for (int o = lane * 8; o < out; o += 512) {
        const V8 gv = *(const V8*)(dy + (long long)row * dy_ld + o);
#pragma unroll
        for (int r = 0; r < RMAX; ++r)
            if (r < rank) {
#pragma unroll
                for (int j = 0; j < 8; ++j) at[r] = __builtin_fmaf(to_f32<T>(gv[j]), lb[(long long)(o + j) * rank + r], at[r]);
            }
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        au[r] = wave_sum(au[r]);
        at[r] = wave_sum(at[r]);
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < RMAX / 4; ++g) {
            const f32x4 a = {au[4 * g], au[4 * g + 1], au[4 * g + 2], au[4 * g + 3]};
            const f32x4 b = {at[4 * g], at[4 * g + 1], at[4 * g + 2], at[4 * g + 3]};
            *(f32x4*)(u + (long long)row * RMAX + 4 * g) = a;
            *(f32x4*)(t + (long long)row * RMAX + 4 * g) = b;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_grad_outer_kernel(const T* __restrict__ x, int x_ld, const T* __restrict__ dy, int dy_ld,
                                                        const float* __restrict__ u, const float* __restrict__ t, float* __restrict__ part,
                                                        int m, int in, int out, int rank, int chunk_rows) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 2;                   // column of x | dy
    if (col >= in + out) return;
    const bool left = col < in;                                             // da takes x and t, db takes dy and u
    const T* val = left ? x + col : dy + (col - in);
    const int ld = left ? x_ld : dy_ld;
    const float* coef = left ? t : u;
    const int r0 = blockIdx.y * chunk_rows, r1 = min(r0 + chunk_rows, m);
    float a0[RMAX], a1[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) a0[r] = a1[r] = 0.f;
#pragma unroll 4
    for (int row = r0; row < r1; ++row) {
        const T* vp = val + (long long)row * ld;
        const float v0 = to_f32<T>(vp[0]), v1 = to_f32<T>(vp[1]);
#pragma unroll
        for (int g = 0; g < RMAX / 4; ++g) {
            const f32x4 c = *(const f32x4*)(coef + (long long)row * RMAX + 4 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0[4 * g + e] = __builtin_fmaf(c[e], v0, a0[4 * g + e]);
                a1[4 * g + e] = __builtin_fmaf(c[e], v1, a1[4 * g + e]);
            }
        }
    }
    float* pp = part + (long long)blockIdx.y * rank * (in + out) + col;
#pragma unroll
    for (int r = 0; r < RMAX; ++r)
        if (r < rank) {
            const f32x2 w = {a0[r], a1[r]};
            *(f32x2*)(pp + (long long)r * (in + out)) = w;
        }
}

__global__ __launch_bounds__(256) void lora_grad_merge_kernel(const float* __restrict__ part, int chunks, float* __restrict__ da, float* __restrict__ db,
                                                        int in, int out, int rank, float scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                         // (r, column of x | dy)
    const int cols = in + out;
    if (idx >= rank * cols) return;
    const int r = idx / cols, col = idx - r * cols;
    double s = 0.0;
#pragma unroll 8                                                             // eight loads in flight; the additions stay in ascending order
    for (int c = 0; c < chunks; ++c) s += (double)part[(long long)c * rank * cols + idx];
    const float g = (float)(s * (double)scale);
    if (col < in) da[(long long)r * in + col] = g;
    else db[(long long)(col - in) * rank + r] = g;
}

int grad_check_dims(const char* api, long long m, int in, int out, int rank) {
    IDB_REQUIRE(m > 0 && m < (1ll << 31) - 4, "%s: m must be positive and below 2^31", api);
    IDB_REQUIRE(in > 0 && in % 64 == 0 && in <= (1 << 20), "%s: in must be a positive multiple of 64", api);
    IDB_REQUIRE(out > 0 && out % 64 == 0 && out <= (1 << 20), "%s: out must be a positive multiple of 64", api);
    IDB_REQUIRE(rank >= 1 && rank <= RMAX, "%s: rank must be 1..%d", api, RMAX);
    return IDB_OK;
}

}  // namespace

extern "C" size_t idb_lora_grad_workspace_bytes(int64_t m, int32_t in, int32_t out, int32_t rank) {
    if (grad_check_dims("idb_lora_grad_workspace_bytes", m, in, out, rank) != IDB_OK) return 0;
    const GradPlan p = grad_plan(m, in, out, rank);
    return p.proj_bytes + p.part_bytes;
}

extern "C" int idb_lora_grad(const void* x, int32_t x_ld, const void* dy, int32_t dy_ld, const float* lora_a, const float* lora_b, float* da,
                             float* db, int64_t m, int32_t in, int32_t out, int32_t rank, float scale, void* workspace, size_t workspace_bytes,
                             int32_t dtype, void* stream) {
    const char* api = "idb_lora_grad";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be bf16/f16", api);
        return IDB_EUNSUPPORTED;
    }
    const void* ptrs[] = {x, dy, lora_a, lora_b, da, db, workspace};
    const char* names[] = {"x", "dy", "lora_a", "lora_b", "da", "db", "workspace"};
    for (int i = 0; i < 7; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        IDB_REQUIRE(i == 4 || i == 5 ? ((uintptr_t)ptrs[i] & 3) == 0 : idb_aligned16(ptrs[i]), "%s: %s is not aligned (16 bytes; da, db 4)", api,
                    names[i]);
    }
    if (int rc = grad_check_dims(api, m, in, out, rank)) return rc;
    IDB_REQUIRE(x_ld >= in && x_ld % 8 == 0, "%s: x_ld must be at least in and a multiple of 8 elements (16 bytes)", api);
    IDB_REQUIRE(dy_ld >= out && dy_ld % 8 == 0, "%s: dy_ld must be at least out and a multiple of 8 elements (16 bytes)", api);
    const GradPlan p = grad_plan(m, in, out, rank);
    IDB_REQUIRE(workspace_bytes >= p.proj_bytes + p.part_bytes, "%s: workspace_bytes %zu < %zu (idb_lora_grad_workspace_bytes)", api,
                workspace_bytes, p.proj_bytes + p.part_bytes);
    hipStream_t st = (hipStream_t)stream;
    float* u = (float*)workspace;
    float* t = u + m * RMAX;
    float* part = t + m * RMAX;
    const dim3 pgrid((unsigned)((m + 3) / 4)), ogrid((in + out + 511) / 512, p.chunks);
    if (dtype == IDB_BF16) {
        hipLaunchKernelGGL(lora_grad_proj_kernel<__bf16>, pgrid, dim3(256), 0, st, (const __bf16*)x, x_ld, (const __bf16*)dy, dy_ld, lora_a, lora_b, u, t,
                           (int)m, in, out, rank);
        IDB_CHECK_LAUNCH(api);
        hipLaunchKernelGGL(lora_grad_outer_kernel<__bf16>, ogrid, dim3(256), 0, st, (const __bf16*)x, x_ld, (const __bf16*)dy, dy_ld, u, t, part, (int)m, in,
                           out, rank, p.chunk_rows);
    } else {
        hipLaunchKernelGGL(lora_grad_proj_kernel<_Float16>, pgrid, dim3(256), 0, st, (const _Float16*)x, x_ld, (const _Float16*)dy, dy_ld, lora_a, lora_b, u,
                           t, (int)m, in, out, rank);
        IDB_CHECK_LAUNCH(api);
        hipLaunchKernelGGL(lora_grad_outer_kernel<_Float16>, ogrid, dim3(256), 0, st, (const _Float16*)x, x_ld, (const _Float16*)dy, dy_ld, u, t, part,
                           (int)m, in, out, rank, p.chunk_rows);
    }
    IDB_CHECK_LAUNCH(api);
    hipLaunchKernelGGL(lora_grad_merge_kernel, dim3((rank * (in + out) + 255) / 256), dim3(256), 0, st, part, p.chunks, da, db, in, out, rank, scale);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}
