// K8b: classifier-free guidance + one PLMS step (PNDMScheduler with skip_prk_steps) in one launch, fp32.  Launch-latency sized and
// HBM-bound (batch * 4 * hw elements): plain C++, fp32 arithmetic, coalesced accesses.
#include "idb_common.h"

namespace {

struct PlmsArgs {
    const float* eps;      // [rep*batch][hw][C], uncond first
    float* lat;            // [batch][C][hw], updated in place
    float* slot_w;         // history slot that receives this step's guided eps, or nullptr (the counter == 1 step)
    const float* h1;       // ets[-2], ets[-3], ets[-4] (ets[-1] on the counter == 1 step): dereferenced only below n_terms
    const float* h2;
    const float* h3;
    float* saved;          // the sample of the counter == 0 step
    const float* coef;     // device: {w0, w1, w2, w3, sqrt_abar, sqrt_bbar, c_sample, c_eps, guidance}
    int batch, C, hw, rep, vpred, n_terms, mode;
};

struct PlmsCoef {
    float w0, w1, w2, w3, sqrt_a, sqrt_b, c_sample, c_eps, g;
};

__device__ __forceinline__ PlmsCoef plms_coef(const float* __restrict__ c) {
    return {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
}

struct PlmsIn {
    float x, h1, h2, h3;
};

// What the update of NCHW element i reads.  A history slot is read only if n_terms says it holds a prediction, the saved sample only
// on the step that restores it: a zero weight would not protect against NaN in memory nobody has written yet.
__device__ __forceinline__ PlmsIn plms_load(const PlmsArgs& a, long long i) {
    PlmsIn in = {0.f, 0.f, 0.f, 0.f};
    in.x = a.mode == IDB_PLMS_RESTORE ? a.saved[i] : a.lat[i];
    if (a.n_terms > 1) in.h1 = a.h1[i];
    if (a.n_terms > 2) in.h2 = a.h2[i];
    if (a.n_terms > 3) in.h3 = a.h3[i];
    return in;
}

// e: the guided eps of element i.  Loads and stores are kept apart so that a thread with several elements has all its loads in
// flight before its first store (the buffers may alias as far as the compiler knows).
__device__ __forceinline__ void plms_store(const PlmsArgs& a, const PlmsCoef& k, long long i, float e, const PlmsIn& in) {
    if (a.slot_w) a.slot_w[i] = e;
    if (a.mode == IDB_PLMS_SAVE) a.saved[i] = in.x;
    float m = k.w0 * e;
    if (a.n_terms > 1) m += k.w1 * in.h1;
    if (a.n_terms > 2) m += k.w2 * in.h2;
    if (a.n_terms > 3) m += k.w3 * in.h3;
    if (a.vpred) m = k.sqrt_a * m + k.sqrt_b * in.x;
    a.lat[i] = k.c_sample * in.x - k.c_eps * m;
}

// one thread per NCHW element (any channel count)
__global__ __launch_bounds__(256) void cfg_plms_kernel(PlmsArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.batch * a.C * a.hw) return;
    const int pix = (int)(i % a.hw);
    const int c = (int)((i / a.hw) % a.C);
    const int b = (int)(i / ((long long)a.hw * a.C));
    const PlmsCoef k = plms_coef(a.coef);
    float e = a.eps[((long long)b * a.hw + pix) * a.C + c];
    if (a.rep == 2) {
        const float ec = a.eps[((long long)(a.batch + b) * a.hw + pix) * a.C + c];
        e = e + k.g * (ec - e);
    }
    plms_store(a, k, i, e, plms_load(a, i));
}

// C == 4 and eps 16-byte aligned: one thread per pixel reads its four channels of eps as one float4 (a whole NHWC pixel); the NCHW
// side stays one dword per channel, consecutive lanes on consecutive pixels.  No tail: hw need not be a multiple of anything.
__global__ __launch_bounds__(256) void cfg_plms_c4_kernel(PlmsArgs a) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)a.batch * a.hw) return;
    const int pix = (int)(p % a.hw);
    const long long b = p / a.hw;
    const PlmsCoef k = plms_coef(a.coef);
    const float4* eps4 = (const float4*)a.eps;
    float4 e = eps4[p];
    if (a.rep == 2) {
        const float4 ec = eps4[(long long)a.batch * a.hw + p];
        e.x = e.x + k.g * (ec.x - e.x);
        e.y = e.y + k.g * (ec.y - e.y);
        e.z = e.z + k.g * (ec.z - e.z);
        e.w = e.w + k.g * (ec.w - e.w);
    }
    const long long i0 = b * 4 * a.hw + pix, i1 = i0 + a.hw, i2 = i1 + a.hw, i3 = i2 + a.hw;
    const PlmsIn in0 = plms_load(a, i0), in1 = plms_load(a, i1), in2 = plms_load(a, i2), in3 = plms_load(a, i3);
    plms_store(a, k, i0, e.x, in0);
    plms_store(a, k, i1, e.y, in1);
    plms_store(a, k, i2, e.z, in2);
    plms_store(a, k, i3, e.w, in3);
}

}  // namespace

extern "C" int idb_cfg_plms_step(const float* eps, float* latents, float* hist, float* saved, const float* coef, int32_t batch,
                                 int32_t channels, int32_t hw, int32_t rep, int32_t prediction_type, int32_t write_slot,
                                 int32_t n_terms, int32_t slot1, int32_t slot2, int32_t slot3, int32_t sample_mode, void* stream) {
    IDB_REQUIRE(eps && latents && hist && saved && coef && batch > 0 && channels > 0 && hw > 0, "idb_cfg_plms_step: bad args");
    IDB_REQUIRE(rep == 1 || rep == 2, "idb_cfg_plms_step: rep must be 1 or 2, got %d", rep);
    IDB_REQUIRE(prediction_type == 0 || prediction_type == 1, "idb_cfg_plms_step: prediction_type must be 0 (epsilon) or 1 (v)");
    IDB_REQUIRE(n_terms >= 1 && n_terms <= IDB_PLMS_SLOTS, "idb_cfg_plms_step: n_terms must be 1..%d, got %d", IDB_PLMS_SLOTS, n_terms);
    IDB_REQUIRE(write_slot >= -1 && write_slot < IDB_PLMS_SLOTS, "idb_cfg_plms_step: write_slot %d out of range (-1..%d)", write_slot,
                IDB_PLMS_SLOTS - 1);
    IDB_REQUIRE(sample_mode == IDB_PLMS_KEEP || sample_mode == IDB_PLMS_SAVE || sample_mode == IDB_PLMS_RESTORE,
                "idb_cfg_plms_step: sample_mode must be 0 (keep), 1 (save) or 2 (restore)");
    const int32_t slots[3] = {slot1, slot2, slot3};
    const long long total = (long long)batch * channels * hw;
    const float* h[3] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < n_terms - 1; ++j) {                  // slots past n_terms are never looked at
        IDB_REQUIRE(slots[j] >= 0 && slots[j] < IDB_PLMS_SLOTS, "idb_cfg_plms_step: read slot %d out of range (0..%d)", slots[j],
                    IDB_PLMS_SLOTS - 1);
        IDB_REQUIRE(slots[j] != write_slot, "idb_cfg_plms_step: slot %d is both read and written", slots[j]);
        h[j] = hist + slots[j] * total;
    }
    PlmsArgs a = {eps, latents, write_slot >= 0 ? hist + write_slot * total : nullptr, h[0], h[1], h[2], saved, coef,
                  batch, channels, hw, rep, prediction_type, n_terms, sample_mode};
    const long long blocks = channels == 4 && idb_aligned16(eps) ? ((long long)batch * hw + 255) / 256 : (total + 255) / 256;
    IDB_REQUIRE(blocks <= 0x7fffffffll, "idb_cfg_plms_step: tensor too large");
    if (channels == 4 && idb_aligned16(eps))
        hipLaunchKernelGGL(cfg_plms_c4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(cfg_plms_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    IDB_CHECK_LAUNCH("idb_cfg_plms_step");
    return IDB_OK;
}
