// The training objective's forward pass (/root/reference/train_ID-Booth.py:996-1134): the small kernels that sit
// between vae.encode, the UNet, vae.decode, MTCNN and ArcFace when a checkpoint's step losses are evaluated under no_grad.
//   diffuse:   noise_scheduler.add_noise (:1018) and the target selection (:1055-1058), one launch
//   mse_x0:    F.mse_loss(model_pred.float(), target.float()) per sample (:1072-1074) and noise_scheduler.step(...).pred_original_sample
//              (:1081, :1109), one pass over model_pred, target and the noisy latents
//   bilinear:  the bounding-box crop (:1090) and cropped_image_to_arcface_input (:445-455) on the float image
//   losses:    nn.CosineSimilarity(dim=1, eps=1e-6) (:972, :1096), 1 - cos (:1098), TripletMarginWithDistanceLoss over the cosine
//              distance (:974-979, :1133)
// faceposegenerator_amd/objective.py drives them.  All are fp32 in and out; whatever decides an output's last bits (the schedule's
// coefficients, the sums, the interpolation weights) is computed in double and rounded to fp32 once.  No floating-point atomics: every
// sum has a fixed order, so results are bit-identical from run to run.
#include "idb_common.h"

namespace {

// sqrt(abar_t) and sqrt(1 - abar_t) of sample b in double from the fp32 table.  A timestep outside [0, T) cannot be refused without a
// synchronisation, so it is clamped into the table.
__device__ __forceinline__ void schedule_coefs(const int* __restrict__ ts, const float* __restrict__ ac, int T, int b, double& sa, double& sb) {
    const int t = min(max(ts[b], 0), T - 1);
    const double a = (double)ac[t];
    sa = sqrt(a);
    sb = sqrt(1.0 - a);
}

// fixed-order sum over the 256 threads of a workgroup: a shuffle tree inside each wave, then the four waves in ascending order
__device__ __forceinline__ double block_sum256(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// ---- diffuse -----------------------------------------------------------------------------------------------------------------
// noisy = sa x0 + sb noise; target = noise (epsilon) or sa noise - sb x0 (v-prediction).  V elements per thread (V = 4: 16-byte
// accesses); grid.y is the sample, so the two coefficients are uniform over a workgroup.
template <int V>
__global__ __launch_bounds__(256) void diffuse_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const int* __restrict__ ts,
                                                      const float* __restrict__ ac, int T, int vpred, long long chw,
                                                      float* __restrict__ noisy, float* __restrict__ target) {
    const int b = blockIdx.y;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= chw) return;
    double sa, sb;
    schedule_coefs(ts, ac, T, b, sa, sb);
    const long long e = (long long)b * chw + i;
    float x[V], n[V], y[V], tg[V];
    if constexpr (V == 4) {
        *(f32x4*)x = *(const f32x4*)(x0 + e);
        *(f32x4*)n = *(const f32x4*)(noise + e);
    } else {
        x[0] = x0[e];
        n[0] = noise[e];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        y[k] = (float)(sa * (double)x[k] + sb * (double)n[k]);
        tg[k] = vpred ? (float)(sa * (double)n[k] - sb * (double)x[k]) : n[k];
    }
    if constexpr (V == 4) {
        *(f32x4*)(noisy + e) = *(const f32x4*)y;
        if (target) *(f32x4*)(target + e) = *(const f32x4*)tg;
    } else {
        noisy[e] = y[0];
        if (target) target[e] = tg[0];
    }
}

// ---- mse + predicted x0 ------------------------------------------------------------------------------------------------------
// One thread per latent pixel, MSE_PIX pixels per workgroup, the channels in an inner loop: target, noisy and x0_pred (NCHW) are
// read and written coalesced along the pixels, and pred either the same way (NCHW) or as the pixel's C adjacent values (the engine's
// [B][HW][C]).  The mapping of elements to threads does not depend on pred's layout, so neither does the order of the sum.
constexpr int MSE_PIX = 1024;

__global__ __launch_bounds__(256) void mse_x0_kernel(const float* __restrict__ pred, int nhwc, const float* __restrict__ target,
                                                     const float* __restrict__ noisy, const int* __restrict__ ts, const float* __restrict__ ac,
                                                     int T, int vpred, int C, int hw, double* __restrict__ partial, float* __restrict__ x0_pred) {
    __shared__ double lds[4];
    const int b = blockIdx.y;
    double sa = 1.0, sb = 0.0;
    if (x0_pred) schedule_coefs(ts, ac, T, b, sa, sb);
    const long long base = (long long)b * C * hw;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < MSE_PIX / 256; ++k) {
        const int p = blockIdx.x * MSE_PIX + k * 256 + threadIdx.x;
        if (p >= hw) continue;
        for (int c = 0; c < C; ++c) {
            const long long e = base + (long long)c * hw + p;
            const double pr = (double)pred[nhwc ? base + (long long)p * C + c : e];
            const double df = pr - (double)target[e];
            acc += df * df;
            if (x0_pred) {
                const double nz = (double)noisy[e];
                x0_pred[e] = (float)(vpred ? sa * nz - sb * pr : (nz - sb * pr) / sa);
            }
        }
    }
    acc = block_sum256(acc, lds);
    if (threadIdx.x == 0) partial[(long long)b * gridDim.x + blockIdx.x] = acc;
}

// one workgroup per sample: thread t takes partials t, t + 256, ... in ascending order, then the same tree
__global__ __launch_bounds__(256) void mse_finish_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ sse) {
    __shared__ double lds[4];
    const int b = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[(long long)b * nblk + i];
    acc = block_sum256(acc, lds);
    if (threadIdx.x == 0) sse[b] = acc;
}

// ---- crop + bilinear resize + ArcFace normalisation --------------------------------------------------------------------------
// torchvision 0.16.2's tensor resize(img, size, antialias=None) is F.interpolate(mode="bilinear", align_corners=False,
// antialias=False), restated from ATen's upsample_bilinear2d (UpSampleKernel.cpp: area_pixel_compute_source_index, guard_index_and_lambda);
// PARITY UNPINNED against a torchvision binary (there is none here).  Per axis: source coordinate s = (o + 0.5) in / out - 0.5, clamped at
// 0; first tap i = floor(s), second tap min(i + 1, in - 1); weights 1 - (s - i) and s - i.  The coordinate and both weights are computed
// in double (ATen uses the tensor's fp32) and rounded to fp32 once, so a float64 oracle sees the same weights to half an ulp.  The four
// taps are then combined in ATen's order in fp32, followed by ((v / 255) - 0.5) / 0.5 as the reference writes it.
__device__ __forceinline__ void bilinear_taps(int o, int in, int out, int& i0, int& i1, float& w0, float& w1) {
    double s = ((double)o + 0.5) * ((double)in / (double)out) - 0.5;
    s = s < 0.0 ? 0.0 : s;
    i0 = min((int)s, in - 1);
    i1 = min(i0 + 1, in - 1);
    const double l1 = fmin(fmax(s - (double)i0, 0.0), 1.0);
    w0 = (float)(1.0 - l1);
    w1 = (float)l1;
}

// boxes: [n][5] = {image, y0, y1, x0, x1} (y1 / x1 exclusive, already clipped to the image).  One thread per output pixel; a wave reads
// runs of adjacent source pixels (C adjacent floats each) on two rows and writes C coalesced NCHW rows.
__global__ __launch_bounds__(256) void crop_resize_bilinear_kernel(const float* __restrict__ src, int h, int w, int c, const int* __restrict__ boxes,
                                                                   int n, float* __restrict__ out, int oh, int ow) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * oh * ow) return;
    const int ox = (int)(idx % ow);
    const int oy = (int)((idx / ow) % oh);
    const int k = (int)(idx / ((long long)ow * oh));
    const int img = boxes[k * 5], y0 = boxes[k * 5 + 1], y1 = boxes[k * 5 + 2], x0 = boxes[k * 5 + 3], x1 = boxes[k * 5 + 4];
    int ya, yb, xa, xb;
    float hy0, hy1, wx0, wx1;
    bilinear_taps(oy, y1 - y0, oh, ya, yb, hy0, hy1);
    bilinear_taps(ox, x1 - x0, ow, xa, xb, wx0, wx1);
    const float* ra = src + (((long long)img * h + (y0 + ya)) * w + x0) * c;
    const float* rb = src + (((long long)img * h + (y0 + yb)) * w + x0) * c;
    float* o = out + (long long)k * c * oh * ow + (long long)oy * ow + ox;
    for (int ch = 0; ch < c; ++ch) {
        const float top = wx0 * ra[(long long)xa * c + ch] + wx1 * ra[(long long)xb * c + ch];
        const float bot = wx0 * rb[(long long)xa * c + ch] + wx1 * rb[(long long)xb * c + ch];
        const float v = hy0 * top + hy1 * bot;
        o[(long long)ch * oh * ow] = ((v / 255.0f) - 0.5f) / 0.5f;
    }
}

// ---- identity losses ---------------------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup.  Lane l takes elements l, l + 64, ... in ascending order: the dot products with the positive
// (and negative) embedding and the three sums of squares in double (a product of two fp32 numbers is exact in double), then a fixed
// shuffle tree.  torch's cosine similarity clamps EACH norm: cos_eps(a, b) = a.b / (max(|a|, eps) max(|b|, eps)).
//   cos = cos_1e-6(a, pos)                 identity = 1 - cos
//   triplet = max((1 - cos_1e-8(a, pos)) - (1 - cos_1e-8(a, neg)) + 1, 0)
// each from the double sums with one rounding to fp32.
__device__ __forceinline__ double cos_eps(double dot, double ssa, double ssb, double eps) {
    return dot / (fmax(sqrt(ssa), eps) * fmax(sqrt(ssb), eps));
}

__global__ __launch_bounds__(256) void identity_losses_kernel(const float* __restrict__ feat, const float* __restrict__ pos,
                                                              const float* __restrict__ neg, int n, int d, float* __restrict__ cosv,
                                                              float* __restrict__ identity, float* __restrict__ triplet) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;                                          // whole waves leave together: no shuffle crosses a row
    const float* a = feat + (long long)r * d;
    const float* p = pos + (long long)r * d;
    const float* q = neg ? neg + (long long)r * d : nullptr;
    double ap = 0.0, an = 0.0, aa = 0.0, pp = 0.0, nn = 0.0;
    for (int i = lane; i < d; i += 64) {
        const double x = (double)a[i], y = (double)p[i];
        ap += x * y;
        aa += x * x;
        pp += y * y;
        if (q) {
            const double z = (double)q[i];
            an += x * z;
            nn += z * z;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ap += __shfl_xor(ap, o, 64);
        aa += __shfl_xor(aa, o, 64);
        pp += __shfl_xor(pp, o, 64);
        an += __shfl_xor(an, o, 64);
        nn += __shfl_xor(nn, o, 64);
    }
    if (lane != 0) return;
    const double c6 = cos_eps(ap, aa, pp, 1e-6);
    cosv[r] = (float)c6;
    identity[r] = (float)(1.0 - c6);
    if (q) {
        const double dp = 1.0 - cos_eps(ap, aa, pp, 1e-8), dn = 1.0 - cos_eps(an, aa, nn, 1e-8);
        triplet[r] = (float)fmax(dp - dn + 1.0, 0.0);
    }
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// the arguments idb_diffuse_targets and idb_objective_mse_x0 share; sets the error text and returns a status
static int check_schedule_args(const char* api, const int32_t* timesteps, const float* alphas_cumprod, int32_t n_train, int32_t prediction_type,
                               int32_t batch, int32_t channels, int32_t hw) {
    IDB_REQUIRE(timesteps && alphas_cumprod && n_train > 0, "%s: timesteps, alphas_cumprod (n_train > 0) are required", api);
    IDB_REQUIRE(aligned_to(timesteps, 4) && aligned_to(alphas_cumprod, 4), "%s: unaligned pointer", api);
    IDB_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && hw > 0 && (long long)channels * hw < (1LL << 31),
                "%s: batch 1..65535, channels, hw > 0, channels * hw < 2^31", api);
    if (prediction_type != 0 && prediction_type != 1) {
        idb_set_error("%s: prediction_type %d (0 = epsilon, 1 = v_prediction)", api, prediction_type);
        return IDB_EUNSUPPORTED;
    }
    return IDB_OK;
}

}  // namespace

extern "C" int idb_diffuse_targets(const float* x0, const float* noise, const int32_t* timesteps, const float* alphas_cumprod, int32_t n_train,
                                   int32_t prediction_type, int32_t batch, int32_t channels, int32_t hw, float* noisy, float* target,
                                   void* stream) {
    IDB_REQUIRE(x0 && noise && noisy, "idb_diffuse_targets: null pointer");
    IDB_REQUIRE(aligned_to(x0, 4) && aligned_to(noise, 4) && aligned_to(noisy, 4) && aligned_to(target, 4), "idb_diffuse_targets: unaligned pointer");
    const int rc = check_schedule_args("idb_diffuse_targets", timesteps, alphas_cumprod, n_train, prediction_type, batch, channels, hw);
    if (rc != IDB_OK) return rc;
    const long long chw = (long long)channels * hw;
    hipStream_t st = (hipStream_t)stream;
    if (chw % 4 == 0 && aligned_to(x0, 16) && aligned_to(noise, 16) && aligned_to(noisy, 16) && aligned_to(target, 16))
        hipLaunchKernelGGL(diffuse_kernel<4>, dim3((unsigned)((chw / 4 + 255) / 256), batch), dim3(256), 0, st, x0, noise, timesteps, alphas_cumprod,
                           n_train, prediction_type, chw, noisy, target);
    else
        hipLaunchKernelGGL(diffuse_kernel<1>, dim3((unsigned)((chw + 255) / 256), batch), dim3(256), 0, st, x0, noise, timesteps, alphas_cumprod,
                           n_train, prediction_type, chw, noisy, target);
    IDB_CHECK_LAUNCH("idb_diffuse_targets");
    return IDB_OK;
}

extern "C" size_t idb_objective_workspace_bytes(int32_t batch, int64_t chw) {
    if (batch <= 0 || batch > 65535 || chw <= 0 || chw >= (1LL << 31)) return 0;
    // the kernel writes ceil(hw / MSE_PIX) partials per sample; hw <= chw, and the ABI of this query does not take the channel count
    return (size_t)batch * (size_t)((chw + MSE_PIX - 1) / MSE_PIX) * sizeof(double);
}

extern "C" int idb_objective_mse_x0(const float* pred, int32_t pred_nhwc, const float* target, const float* noisy, const int32_t* timesteps,
                                    const float* alphas_cumprod, int32_t n_train, int32_t prediction_type, int32_t batch, int32_t channels,
                                    int32_t hw, double* sse, float* x0_pred, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(pred && target && sse && ws, "idb_objective_mse_x0: null pointer");
    IDB_REQUIRE(!x0_pred || noisy, "idb_objective_mse_x0: x0_pred needs noisy");
    IDB_REQUIRE(aligned_to(pred, 4) && aligned_to(target, 4) && aligned_to(noisy, 4) && aligned_to(x0_pred, 4) && aligned_to(sse, 8) && aligned_to(ws, 8),
                "idb_objective_mse_x0: unaligned pointer");
    const int rc = check_schedule_args("idb_objective_mse_x0", timesteps, alphas_cumprod, n_train, prediction_type, batch, channels, hw);
    if (rc != IDB_OK) return rc;
    const int nblk = (hw + MSE_PIX - 1) / MSE_PIX;
    IDB_REQUIRE(ws_bytes >= (size_t)batch * nblk * sizeof(double), "idb_objective_mse_x0: workspace of %zu bytes, %zu needed", ws_bytes,
                (size_t)batch * nblk * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mse_x0_kernel, dim3(nblk, batch), dim3(256), 0, st, pred, pred_nhwc != 0, target, noisy, timesteps, alphas_cumprod, n_train,
                       prediction_type, channels, hw, (double*)ws, x0_pred);
    IDB_CHECK_LAUNCH("idb_objective_mse_x0");
    hipLaunchKernelGGL(mse_finish_kernel, dim3(batch), dim3(256), 0, st, (const double*)ws, nblk, sse);
    IDB_CHECK_LAUNCH("idb_objective_mse_x0 (finish)");
    return IDB_OK;
}

extern "C" int idb_crop_resize_bilinear_f32(const float* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* boxes,
                                            int32_t n, float* out, int32_t out_h, int32_t out_w, void* stream) {
    IDB_REQUIRE(src && boxes && out && batch > 0 && h > 0 && w > 0 && channels > 0 && n >= 0 && out_h > 0 && out_w > 0,
                "idb_crop_resize_bilinear_f32: bad arguments");
    IDB_REQUIRE(aligned_to(src, 4) && aligned_to(boxes, 4) && aligned_to(out, 4), "idb_crop_resize_bilinear_f32: unaligned pointer");
    IDB_REQUIRE((long long)h * w < (1LL << 31) && n <= (1 << 28), "idb_crop_resize_bilinear_f32: image plane or box count too large");
    if (n == 0) return IDB_OK;
    const long long total = (long long)n * out_h * out_w;
    IDB_REQUIRE(total < (1LL << 31) * 256, "idb_crop_resize_bilinear_f32: too many outputs");
    hipLaunchKernelGGL(crop_resize_bilinear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, h, w, channels,
                       boxes, n, out, out_h, out_w);
    IDB_CHECK_LAUNCH("idb_crop_resize_bilinear_f32");
    return IDB_OK;
}

extern "C" int idb_identity_losses(const float* feat, const float* pos, const float* neg, int32_t n, int32_t d, float* cos, float* identity,
                                   float* triplet, void* stream) {
    IDB_REQUIRE(feat && pos && cos && identity, "idb_identity_losses: null pointer");
    IDB_REQUIRE((neg == nullptr) == (triplet == nullptr), "idb_identity_losses: neg and triplet go together");
    IDB_REQUIRE(aligned_to(feat, 4) && aligned_to(pos, 4) && aligned_to(neg, 4) && aligned_to(cos, 4) && aligned_to(identity, 4) && aligned_to(triplet, 4),
                "idb_identity_losses: unaligned pointer");
    IDB_REQUIRE(n > 0 && n <= (1 << 30) && d > 0, "idb_identity_losses: n 1..2^30, d >= 1");
    if (d > 8192) {
        idb_set_error("idb_identity_losses: d %d (1..8192)", d);
        return IDB_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(identity_losses_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, feat, pos, neg, n, d, cos, identity, triplet);
    IDB_CHECK_LAUNCH("idb_identity_losses");
    return IDB_OK;
}
