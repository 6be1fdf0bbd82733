// ID-Booth fine-tuning's optimiser step (train_ID-Booth.py: GradScaler.unscale_, clip_grad_norm_(params, 1.0), torch.optim.AdamW.step
// under fp16 mixed precision) over a table of fp32 tensors: the LoRA adapters.  fp32 states, the norm and every element's step in
// double, every fp32 state rounded once, no floating-point atomics, every sum in an order the element counts alone decide.  The norm's
// arithmetic and geometry are idb_sgd.h's (sgd_parts, sgd_sqsum_part, sgd_sum_parts, sgd_clip_coef), as the clipped SGD step's.
//   sqsum  grid (1024, tensors): workgroup b < sgd_parts(numel) of a tensor writes the squared sum of its part: [tensor][1024] doubles
//   norm   one workgroup: tensor after tensor, each tensor's partials met in the fixed block sum; total_norm = inv_scale sqrt(total),
//          skipped = the norm is not finite
//   step   the geometry of sqsum; nothing is written when the norm is not finite (GradScaler.step's skip).  Otherwise, with
//          g^ = coef inv_scale g and coef = min(1, max_norm / (norm + 1e-6)):  w *= 1 - lr wd;  m = b1 m + (1 - b1) g^;
//          v = b2 v + (1 - b2) g^2;  w -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
// The bias corrections bc1 = 1 - b1^step and bc2 = 1 - b2^step are computed on the HOST in double (pow) and travel as kernel arguments.
#include "idb_sgd.h"
#include <math.h>

namespace {

constexpr int ADAMW_TABLE_MAX = 1024;

struct AdamwTable {
    float* const* w;
    const float* const* g;
    float* const* m;
    float* const* v;
    const long long* n;
    int count;
};

struct AdamwHyper {
    double lr, beta1, beta2, eps, wd, max_norm, inv_scale, bc1, bc2;
};

__global__ __launch_bounds__(256) void adamw_sqsum_kernel(AdamwTable list, double* __restrict__ out) {
    __shared__ double lds4[4];
    const int ti = blockIdx.y;
    const long long n = list.n[ti];
    const int np = sgd_parts(n);
    if ((int)blockIdx.x >= np) return;
    const double s = sgd_sqsum_part(list.g[ti], n, np, lds4);
    if (threadIdx.x == 0) out[(long long)ti * SGD_PARTS + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void adamw_norm_kernel(AdamwTable list, const double* __restrict__ parts, double inv_scale, double* __restrict__ total_norm,
                                                         int* __restrict__ skipped) {
    __shared__ double lds4[4];
    double sum = 0.0;
    for (int ti = 0; ti < list.count; ++ti) sum += sgd_sum_parts(parts + (long long)ti * SGD_PARTS, sgd_parts(list.n[ti]), lds4);
    if (threadIdx.x == 0) {
        const double norm = inv_scale * sqrt(sum);
        *total_norm = norm;
        *skipped = isfinite(norm) ? 0 : 1;
    }
}

__global__ __launch_bounds__(256) void adamw_step_kernel(AdamwTable list, const double* __restrict__ total_norm, AdamwHyper h) {
    const int ti = blockIdx.y;
    const long long n = list.n[ti];
    const int np = sgd_parts(n);
    if ((int)blockIdx.x >= np) return;
    const double norm = *total_norm;
    if (!isfinite(norm)) return;
    const double k = sgd_clip_coef(h.max_norm, norm) * h.inv_scale, decay = 1.0 - h.lr * h.wd, step_size = h.lr / h.bc1, rbc2 = sqrt(h.bc2);
    float* w = list.w[ti];
    const float* g = list.g[ti];
    float* m = list.m[ti];
    float* v = list.v[ti];
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += np * 256LL) {
        const double gh = k * (double)g[i];
        // the weight's step takes the moments as computed, not as stored: each of the three states is the double result rounded once
        const double mi = h.beta1 * (double)m[i] + (1.0 - h.beta1) * gh;
        const double vi = h.beta2 * (double)v[i] + (1.0 - h.beta2) * gh * gh;
        m[i] = (float)mi;
        v[i] = (float)vi;
        w[i] = (float)((double)w[i] * decay - step_size * mi / (sqrt(vi) / rbc2 + h.eps));
    }
}

}  // namespace

extern "C" size_t idb_adamw_clip_table_workspace_bytes(int32_t count) {
    if (count < 1 || count > ADAMW_TABLE_MAX) return 0;
    return sizeof(double) * (size_t)count * SGD_PARTS;
}

extern "C" int idb_adamw_clip_step_table(int32_t count, float* const* weights, const float* const* grads, float* const* exp_avg,
                                         float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2, double eps,
                                         double weight_decay, double max_norm, double inv_scale, int64_t step, double* total_norm,
                                         int32_t* skipped, void* ws, size_t ws_bytes, void* stream) {
    const char* api = "idb_adamw_clip_step_table";
    IDB_REQUIRE(count >= 1 && count <= ADAMW_TABLE_MAX, "%s: count must be 1..%d tensors", api, ADAMW_TABLE_MAX);
    const void* ptrs[] = {weights, grads, exp_avg, exp_avg_sq, numel, total_norm, skipped, ws};
    const char* names[] = {"weights", "grads", "exp_avg", "exp_avg_sq", "numel", "total_norm", "skipped", "ws"};
    for (int i = 0; i < 8; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        const uintptr_t mask = i == 6 ? 3 : i == 7 ? 15 : 7;
        IDB_REQUIRE(((uintptr_t)ptrs[i] & mask) == 0, "%s: %s is not aligned (tables and total_norm 8 bytes, skipped 4, ws 16)", api, names[i]);
    }
    IDB_REQUIRE(lr >= 0.0 && lr <= 1e4, "%s: lr must be in [0, 1e4]", api);
    IDB_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "%s: beta1 must be in [0, 1)", api);
    IDB_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "%s: beta2 must be in [0, 1)", api);
    IDB_REQUIRE(eps >= 0.0 && eps <= 1.0, "%s: eps must be in [0, 1]", api);
    IDB_REQUIRE(weight_decay >= 0.0 && weight_decay <= 1e4, "%s: weight_decay must be in [0, 1e4]", api);
    IDB_REQUIRE(max_norm > 0.0 && max_norm <= 1e30, "%s: max_norm must be in (0, 1e30]", api);
    IDB_REQUIRE(inv_scale > 0.0 && inv_scale <= 1e30, "%s: inv_scale must be in (0, 1e30]", api);
    IDB_REQUIRE(step >= 1, "%s: step must be at least 1", api);
    IDB_REQUIRE(ws_bytes >= sizeof(double) * (size_t)count * SGD_PARTS, "%s: ws_bytes %zu < %zu (idb_adamw_clip_table_workspace_bytes)", api, ws_bytes,
                sizeof(double) * (size_t)count * SGD_PARTS);
    AdamwTable L;
    L.w = weights, L.g = grads, L.m = exp_avg, L.v = exp_avg_sq, L.n = (const long long*)numel, L.count = count;
    AdamwHyper h;
    h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.eps = eps, h.wd = weight_decay, h.max_norm = max_norm, h.inv_scale = inv_scale;
    h.bc1 = 1.0 - pow(beta1, (double)step), h.bc2 = 1.0 - pow(beta2, (double)step);
    hipStream_t st = (hipStream_t)stream;
    double* parts = (double*)ws;
    hipLaunchKernelGGL(adamw_sqsum_kernel, dim3(SGD_PARTS, count), dim3(256), 0, st, L, parts);
    IDB_CHECK_LAUNCH("idb_adamw_clip_step_table(norm partials)");
    hipLaunchKernelGGL(adamw_norm_kernel, dim3(1), dim3(256), 0, st, L, (const double*)parts, inv_scale, total_norm, skipped);
    IDB_CHECK_LAUNCH("idb_adamw_clip_step_table(norm)");
    hipLaunchKernelGGL(adamw_step_kernel, dim3(SGD_PARTS, count), dim3(256), 0, st, L, (const double*)total_norm, h);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}
