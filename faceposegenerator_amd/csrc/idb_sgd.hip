// The face-recognition training loop's joint clip_grad_norm_ + SGD-with-momentum step (train_FR.py:293-296) over a list or a table
// of tensors: the embedding stage's five (idb_sgd_clip_step) and the whole backbone's (idb_sgd_clip_step_table).  fp32 state, the norm
// and every element's step in double, every fp32 state rounded once, no floating-point atomics, every sum in an order the element
// counts alone decide.  The arithmetic is idb_sgd.h's, which the loss head's own two launches (idb_head.hip) share.
//   sqsum  grid (1024, tensors): workgroup b < sgd_parts(numel) of a tensor writes the squared sum of its part: [tensor][1024] doubles
//   norm   one workgroup: tensor after tensor, each tensor's partials met in the fixed block sum; the root of the total
//   step   the geometry of sqsum: d = coef g + wd w with coef = min(1, max_norm / (norm + 1e-6)), buf = d (first step) or
//          momentum buf + d, w -= lr buf
// The kernels are templated on how the tensor list is read: SgdList travels by value in the kernel arguments (up to 8 tensors, no
// upload), SgdTable points at tables in device memory (up to 1024 tensors).  Both run the same code on the same geometry.
#include "idb_sgd.h"
#include <math.h>

namespace {

constexpr int SGD_MAX_TENSORS = 8, SGD_TABLE_MAX = 1024;

struct SgdList {
    float* w[SGD_MAX_TENSORS];
    const float* g[SGD_MAX_TENSORS];
    float* buf[SGD_MAX_TENSORS];
    long long n[SGD_MAX_TENSORS];
    int count;
};

struct SgdTable {
    float* const* w;
    const float* const* g;
    float* const* buf;
    const long long* n;
    int count;
};

template <typename L>
__global__ __launch_bounds__(256) void sgd_sqsum_kernel(L list, double* __restrict__ out) {
    __shared__ double lds4[4];
    const int ti = blockIdx.y;
    const long long n = list.n[ti];
    const int np = sgd_parts(n);
    if ((int)blockIdx.x >= np) return;
    const double s = sgd_sqsum_part(list.g[ti], n, np, lds4);
    if (threadIdx.x == 0) out[(long long)ti * SGD_PARTS + blockIdx.x] = s;
}

template <typename L>
__global__ __launch_bounds__(256) void sgd_norm_kernel(L list, const double* __restrict__ parts, double* __restrict__ total_norm) {
    __shared__ double lds4[4];
    double sum = 0.0;
    for (int ti = 0; ti < list.count; ++ti) sum += sgd_sum_parts(parts + (long long)ti * SGD_PARTS, sgd_parts(list.n[ti]), lds4);
    if (threadIdx.x == 0) *total_norm = sqrt(sum);
}

template <typename L>
__global__ __launch_bounds__(256) void sgd_step_kernel(L list, const double* __restrict__ total_norm, double lr, double momentum, double wd,
                                                       double max_norm, int first) {
    const int ti = blockIdx.y;
    const long long n = list.n[ti];
    const int np = sgd_parts(n);
    if ((int)blockIdx.x >= np) return;
    sgd_step_part(list.w[ti], list.g[ti], list.buf[ti], n, np, sgd_clip_coef(max_norm, *total_norm), lr, momentum, wd, first);
}

// the three launches of `api`, after its checks
template <typename L>
int sgd_run(const char* api, const L& list, double lr, double momentum, double wd, double max_norm, int first, double* total_norm, double* parts,
            hipStream_t st) {
    char name[96];
    hipLaunchKernelGGL(sgd_sqsum_kernel<L>, dim3(SGD_PARTS, list.count), dim3(256), 0, st, list, parts);
    snprintf(name, sizeof(name), "%s(norm partials)", api);
    IDB_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(sgd_norm_kernel<L>, dim3(1), dim3(256), 0, st, list, (const double*)parts, total_norm);
    snprintf(name, sizeof(name), "%s(norm)", api);
    IDB_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(sgd_step_kernel<L>, dim3(SGD_PARTS, list.count), dim3(256), 0, st, list, (const double*)total_norm, lr, momentum, wd,
                       max_norm, first);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

}  // namespace

extern "C" int idb_sgd_clip_step(int32_t count, float* const* weights, const float* const* grads, float* const* momentum_bufs,
                                 const int64_t* numel, double lr, double momentum, double weight_decay, double max_norm, int32_t first_step,
                                 double* total_norm, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(count >= 1 && count <= SGD_MAX_TENSORS, "idb_sgd_clip_step: 1..%d tensors", SGD_MAX_TENSORS);
    IDB_REQUIRE(weights && grads && momentum_bufs && numel && total_norm, "idb_sgd_clip_step: null pointer");
    IDB_REQUIRE((((uintptr_t)total_norm) & 7) == 0, "idb_sgd_clip_step: total_norm 8-byte aligned");
    IDB_REQUIRE(lr >= 0.0 && lr <= 1e4 && momentum >= 0.0 && momentum < 1.0 && weight_decay >= 0.0 && weight_decay <= 1e4 && max_norm > 0.0 &&
                    max_norm <= 1e30,
                "idb_sgd_clip_step: lr in [0, 1e4], momentum in [0, 1), weight_decay in [0, 1e4], max_norm in (0, 1e30]");
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= IDB_SGD_CLIP_WS_BYTES, "idb_sgd_clip_step: workspace too small or unaligned (%d bytes)",
                IDB_SGD_CLIP_WS_BYTES);
    SgdList L;
    memset(&L, 0, sizeof(L));
    L.count = count;
    for (int i = 0; i < count; ++i) {
        IDB_REQUIRE(weights[i] && grads[i] && momentum_bufs[i], "idb_sgd_clip_step: tensor %d: null pointer", i);
        IDB_REQUIRE(numel[i] >= 1 && numel[i] <= (1ll << 32), "idb_sgd_clip_step: tensor %d: 1..2^32 elements", i);
        L.w[i] = weights[i], L.g[i] = grads[i], L.buf[i] = momentum_bufs[i], L.n[i] = numel[i];
        for (int j = 0; j < i; ++j)
            IDB_REQUIRE(weights[i] != weights[j] && momentum_bufs[i] != momentum_bufs[j] && weights[i] != momentum_bufs[j] &&
                            momentum_bufs[i] != weights[j],
                        "idb_sgd_clip_step: tensors %d and %d share a weight or momentum buffer", j, i);
        IDB_REQUIRE(weights[i] != momentum_bufs[i], "idb_sgd_clip_step: tensor %d: weight and momentum buffer are the same", i);
    }
    return sgd_run("idb_sgd_clip_step", L, lr, momentum, weight_decay, max_norm, first_step != 0, total_norm, (double*)ws, (hipStream_t)stream);
}

extern "C" size_t idb_sgd_clip_table_workspace_bytes(int32_t count) {
    if (count < 1 || count > SGD_TABLE_MAX) return 0;
    return sizeof(double) * (size_t)count * SGD_PARTS;
}

extern "C" int idb_sgd_clip_step_table(int32_t count, float* const* weights, const float* const* grads, float* const* momentum_bufs,
                                       const int64_t* numel, double lr, double momentum, double weight_decay, double max_norm,
                                       int32_t first_step, double* total_norm, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(count >= 1 && count <= SGD_TABLE_MAX, "idb_sgd_clip_step_table: 1..%d tensors", SGD_TABLE_MAX);
    IDB_REQUIRE(weights && grads && momentum_bufs && numel && total_norm, "idb_sgd_clip_step_table: null pointer");
    IDB_REQUIRE(((((uintptr_t)total_norm) | ((uintptr_t)weights) | ((uintptr_t)grads) | ((uintptr_t)momentum_bufs) | ((uintptr_t)numel)) & 7) == 0,
                "idb_sgd_clip_step_table: total_norm and the tables 8-byte aligned");
    IDB_REQUIRE(lr >= 0.0 && lr <= 1e4 && momentum >= 0.0 && momentum < 1.0 && weight_decay >= 0.0 && weight_decay <= 1e4 && max_norm > 0.0 &&
                    max_norm <= 1e30,
                "idb_sgd_clip_step_table: lr in [0, 1e4], momentum in [0, 1), weight_decay in [0, 1e4], max_norm in (0, 1e30]");
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= sizeof(double) * (size_t)count * SGD_PARTS,
                "idb_sgd_clip_step_table: workspace too small or unaligned");
    SgdTable L;
    L.w = weights, L.g = grads, L.buf = momentum_bufs, L.n = (const long long*)numel, L.count = count;
    return sgd_run("idb_sgd_clip_step_table", L, lr, momentum, weight_decay, max_norm, first_step != 0, total_norm, (double*)ws,
                   (hipStream_t)stream);
}
