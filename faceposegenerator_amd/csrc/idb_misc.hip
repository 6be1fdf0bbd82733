// K7/K8/K10 and boundary helpers: time-embedding path (fp32), conv_in (Cin=4), CFG + DDPM step,
// image post-processing, layout/dtype conversion, weight packing and LoRA merge.  All HBM-bound
// elementwise / tiny-GEMV work: coalesced vector accesses, fp32 arithmetic.
#include "idb_common.h"

#include <mutex>

// ---------------------------------------------------------------------------------------------
// error text + zero page
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void idb_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* idb_last_error(void) { return g_err; }
extern "C" int idb_version(void) { return 200; }

unsigned long long idb_launch_counter = 0;
extern "C" uint64_t idb_launch_count(void) { return __atomic_load_n(&idb_launch_counter, __ATOMIC_RELAXED); }

const void* idb_zero_page(void) {
    // one zero page per device; immutable after creation (the only process-global state)
    static std::mutex mu;
    static void* pages[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!pages[dev]) {
        void* p = nullptr;
        if (hipMalloc(&p, 4096) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, 4096) != hipSuccess) return nullptr;
        pages[dev] = p;
    }
    return pages[dev];
}

extern "C" int idb_device_check(int device) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        idb_set_error("idb_device_check: %s", hipGetErrorString(e));
        return IDB_EHIP;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        idb_set_error("idb_device_check: device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        return IDB_EUNSUPPORTED;
    }
    return idb_zero_page() ? IDB_OK : IDB_EHIP;
}

namespace {

// ---------------------------------------------------------------------------------------------
// K7 — sinusoidal timestep features (diffusers get_timestep_embedding, flip_sin_to_cos) and the
// fp32 linear used by TimestepEmbedding and the 22 ResnetBlock2D.time_emb_proj layers.
// ---------------------------------------------------------------------------------------------
__global__ void sinusoid_kernel(const float* t, float* out, int n, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (i >= n * half) return;
    const int row = i / half, j = i - row * half;
    const float freq = expf(-logf(10000.0f) * (float)j / (float)half);
    const float a = t[row] * freq;
    out[row * dim + j] = cosf(a);
    out[row * dim + half + j] = sinf(a);
}

// one wave per output feature, 8 rows of x at a time
__global__ __launch_bounds__(256) void linear_f32_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int m,
                                                         int n, int k, int silu_in) {
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= n) return;
    const float* wr = w + (long long)col * k;
    for (int m0 = 0; m0 < m; m0 += 8) {
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int kk = lane; kk < k; kk += 64) {
            const float wv = wr[kk];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (m0 + j < m) {
                    float xv = x[(long long)(m0 + j) * k + kk];
                    if (silu_in) xv = silu_f(xv);
                    acc[j] += xv * wv;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = wave_sum(acc[j]);
            if (lane == 0 && m0 + j < m) y[(long long)(m0 + j) * n + col] = s + (bias ? bias[col] : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// conv_in: fp32 NCHW (Cin <= 4) -> operand-dtype NHWC, optional input scale and 1x1 pre-conv
// (VAE: z / scaling_factor, post_quant_conv).  Block = 256 pixels x one 8-channel output chunk, so
// the 8*Cin*9 weights are wave-uniform (scalar loads).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ out, int batch,
                                                      int rep, int cin, int H, int W, int cout, float in_scale,
                                                      const float* __restrict__ pre_w, const float* __restrict__ pre_b) {
    const long long pixel = (long long)blockIdx.x * 256 + threadIdx.x;
    const int co0 = blockIdx.y * 8;
    const long long HW = (long long)H * W;
    if (pixel >= (long long)batch * HW) return;
    const int b = (int)(pixel / HW);
    const int rem = (int)(pixel - (long long)b * HW);
    const int oy = rem / W, ox = rem - oy * W;
    float in[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
        float raw[4];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            raw[ci] = (ok && ci < cin) ? x[((long long)b * cin + ci) * HW + (long long)iy * W + ix] * in_scale : 0.f;
        if (pre_w) {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                float v = 0.f;
                if (ok && ci < cin) {
                    v = pre_b[ci];
#pragma unroll
                    for (int cj = 0; cj < 4; ++cj)
                        if (cj < cin) v += pre_w[ci * cin + cj] * raw[cj];
                }
                in[tap][ci] = v;
            }
        } else {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) in[tap][ci] = raw[ci];
        }
    }
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int co = co0 + e;
        float a = co < cout ? bias[co] : 0.f;
        if (co < cout) {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)          // static indices: a `ci < cin` loop bound put in[][] into scratch (160 B per lane): 1.41 ms
                                                    // per launch at B = 64 (batch 64 15.05 -> 15.17 images/s without it; an LDS-weight, 2-pixel
                                                    // form with contiguous stores was measured no faster than this fix and is not kept)
                if (ci < cin) {
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) a += w[((long long)co * cin + ci) * 9 + tap] * in[tap][ci];
                }
        }
        acc[e] = a;
    }
    typename Op<T>::v8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(acc[e]);
    for (int r = 0; r < rep; ++r) {
        T* dst = out + (((long long)r * batch + b) * HW + rem) * cout + co0;
        *(typename Op<T>::v8*)dst = o;
    }
}

// ---------------------------------------------------------------------------------------------
// K8 — CFG combine + DDPMScheduler.step (fixed_small variance, no clipping), fp32.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cfg_ddpm_kernel(const float* __restrict__ eps, float* __restrict__ lat,
                                                       const float* __restrict__ noise, const float* __restrict__ coef,
                                                       float* __restrict__ x0_out, int batch, int C, int hw, int cfg,
                                                       int vpred) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)batch * C * hw;
    if (i >= total) return;
    const int pix = (int)(i % hw);
    const int c = (int)((i / hw) % C);
    const int b = (int)(i / ((long long)hw * C));
    const float sqrt_a = coef[0], sqrt_b = coef[1], c_x0 = coef[2], c_x = coef[3], sigma = coef[4], g = coef[5];
    float e = eps[((long long)b * hw + pix) * C + c];
    if (cfg) {
        const float ec = eps[((long long)(batch + b) * hw + pix) * C + c];
        e = e + g * (ec - e);
    }
    const float x = lat[i];
    const float x0 = vpred ? (sqrt_a * x - sqrt_b * e) : (x - sqrt_b * e) / sqrt_a;
    float prev = c_x0 * x0 + c_x * x;
    if (noise) prev += sigma * noise[i];
    lat[i] = prev;
    if (x0_out) x0_out[i] = x0;
}

// K10
// cv2.warpAffine, 8-bit, INTER_LINEAR, BORDER_CONSTANT: one thread per destination pixel (all channels)
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const unsigned char* __restrict__ src, int batch, int H, int W, int C,
                                                             const double* __restrict__ minv, unsigned char* __restrict__ dst,
                                                             int oh, int ow, int border) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)batch * oh * ow) return;
    const int x = (int)(i % ow), y = (int)((i / ow) % oh);
    const int b = (int)(i / ((long long)ow * oh));
    const double* m = minv + (long long)b * 6;
    // OpenCV: adelta/bdelta and X0/Y0 are rounded separately (saturate_cast<int> = round half to even), then added
    const int adelta = __double2int_rn(m[0] * x * 1024.0), bdelta = __double2int_rn(m[3] * x * 1024.0);
    const int X0 = __double2int_rn((m[1] * y + m[2]) * 1024.0) + 16, Y0 = __double2int_rn((m[4] * y + m[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const unsigned char* img = src + (long long)b * H * W * C;
    const bool y0 = sy >= 0 && sy < H, y1 = sy + 1 >= 0 && sy + 1 < H, x0 = sx >= 0 && sx < W, x1 = sx + 1 >= 0 && sx + 1 < W;
    unsigned char* o = dst + i * C;
    for (int c = 0; c < C; ++c) {
        const int p00 = (y0 && x0) ? img[((long long)sy * W + sx) * C + c] : border;
        const int p01 = (y0 && x1) ? img[((long long)sy * W + sx + 1) * C + c] : border;
        const int p10 = (y1 && x0) ? img[((long long)(sy + 1) * W + sx) * C + c] : border;
        const int p11 = (y1 && x1) ? img[((long long)(sy + 1) * W + sx + 1) * C + c] : border;
        o[c] = (unsigned char)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + (1 << 14)) >> 15);
    }
}

// DiagonalGaussianDistribution.sample()/.mode() * scaling_factor: moments NHWC [B][HW][2C] -> latents NCHW [B][C][HW]
__global__ __launch_bounds__(256) void vae_sample_kernel(const float* __restrict__ moments, const float* __restrict__ noise,
                                                         float scale, float* __restrict__ latents, float* __restrict__ mean_out,
                                                         float* __restrict__ logvar_out, int batch, int channels, int hw) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;         // NCHW index
    if (i >= (long long)batch * channels * hw) return;
    const int p = (int)(i % hw);
    const int c = (int)((i / hw) % channels);
    const long long b = i / ((long long)hw * channels);
    const float* m = moments + (b * hw + p) * (2 * channels);
    const float mean = m[c];
    const float logvar = fminf(fmaxf(m[channels + c], -30.f), 20.f);
    float z = mean;
    if (noise) z += expf(0.5f * logvar) * noise[i];
    latents[i] = z * scale;
    if (mean_out) mean_out[i] = mean;
    if (logvar_out) logvar_out[i] = logvar;
}

__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ x, float* __restrict__ img,
                                                          uint8_t* __restrict__ u8, long long count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float v = x[i] * 0.5f + 0.5f;
    v = fminf(fmaxf(v, 0.f), 1.f);
    if (img) img[i] = v;
    if (u8) u8[i] = (uint8_t)fminf(fmaxf(v * 255.f + 0.5f, 0.f), 255.f);
}

template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ x, float* __restrict__ out, int batch,
                                                           int hw, int C) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // index into NCHW output
    if (i >= (long long)batch * hw * C) return;
    const int pix = (int)(i % hw);
    const int c = (int)((i / hw) % C);
    const int b = (int)(i / ((long long)hw * C));
    out[i] = to_f32<T>(x[((long long)b * hw + pix) * C + c]);
}

template <typename T>
__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ x, T* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = from_f32<T>(x[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ src, T* __restrict__ dst, int cout,
                                                        int cin, int taps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // dst index [co][tap][ci]
    if (i >= (long long)cout * cin * taps) return;
    const int ci = (int)(i % cin);
    const int tap = (int)((i / cin) % taps);
    const int co = (int)(i / ((long long)cin * taps));
    dst[i] = from_f32<T>(src[((long long)co * cin + ci) * taps + tap]);
}

__host__ __device__ inline long long geglu_src_row(long long p, long long rows) {
    const long long blk = p >> 5, t = p & 31;
    return t < 16 ? 16 * blk + t : rows / 2 + 16 * blk + (t - 16);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_matrix_kernel(const float* __restrict__ src, T* __restrict__ dst,
                                                          long long rows, long long cols, int geglu) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols, c = i - r * cols;
    const long long sr = geglu ? geglu_src_row(r, rows) : r;
    dst[i] = from_f32<T>(src[sr * cols + c]);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_matrix_scaled_kernel(const float* __restrict__ src, T* __restrict__ dst, long long rows,
                                                                 long long cols, int geglu, const float* __restrict__ cs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols, c = i - r * cols;
    const long long sr = geglu ? geglu_src_row(r, rows) : r;
    dst[i] = from_f32<T>(src[sr * cols + c] * cs[c]);
}

// one wave per output row: u = row sum of the rounded folded matrix, v = (W + scale B A) beta + bias in fp32
template <typename T>
__global__ __launch_bounds__(256) void ln_fold_vectors_kernel(const float* __restrict__ w, const float* __restrict__ a, const float* __restrict__ bm,
                                                              int rank, float scale, const T* __restrict__ wq, const float* __restrict__ beta,
                                                              const float* __restrict__ bias, float* __restrict__ u, float* __restrict__ v,
                                                              long long rows, long long cols, int geglu) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const long long sr = geglu ? geglu_src_row(r, rows) : r;
    float su = 0.f, sv = 0.f;
    for (long long c = lane; c < cols; c += 64) {
        su += to_f32<T>(wq[r * cols + c]);
        sv += w[sr * cols + c] * beta[c];
    }
    for (int j = 0; j < rank; ++j) {
        float ab = 0.f;
        for (long long c = lane; c < cols; c += 64) ab += a[(long long)j * cols + c] * beta[c];
        sv += scale * bm[sr * rank + j] * ab;       // summed over the lanes below together with the W term
    }
    su = wave_sum(su);
    sv = wave_sum(sv);
    if (lane == 0) {
        u[r] = su;
        v[r] = sv + (bias ? bias[r] : 0.f);
    }
}

// [n][k] -> [ceil(n/16)][k/64][16][64]: one thread per 16-byte chunk of the destination (both element types are 2 bytes)
__global__ __launch_bounds__(256) void tile_weight_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long n, long long k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long kt = k >> 6, nb = (n + 15) >> 4;
    if (i >= nb * kt * 128) return;
    const int c8 = (int)(i & 7), r = (int)((i >> 3) & 15);
    const long long t = i >> 7, ktile = t % kt, blk = t / kt;
    const long long row = blk * 16 + r;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < n) v = src[(row * k + ktile * 64) / 8 + c8];
    dst[i] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ w, const float* __restrict__ a,
                                                         const float* __restrict__ bm, T* __restrict__ dst,
                                                         long long rows, long long cols, int rank, float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols, c = i - r * cols;
    float d = 0.f;
    for (int k = 0; k < rank; ++k) d += bm[r * rank + k] * a[(long long)k * cols + c];
    dst[i] = from_f32<T>(w[i] + scale * d);
}

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_scaled_kernel(const float* __restrict__ w, const float* __restrict__ a,
                                                                const float* __restrict__ bm, T* __restrict__ dst, long long rows,
                                                                long long cols, int rank, float scale, const float* __restrict__ cs) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long long r = i / cols, c = i - r * cols;
    float d = 0.f;
    for (int k = 0; k < rank; ++k) d += bm[r * rank + k] * a[(long long)k * cols + c];
    dst[i] = from_f32<T>((w[i] + scale * d) * cs[c]);
}

template <typename T>
__global__ __launch_bounds__(256) void embed_kernel(const long long* __restrict__ ids, const float* __restrict__ tok,
                                                    const float* __restrict__ pos, T* __restrict__ out, int rows, int n_tokens, int dim) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // one thread per 4 output features
    const int d4 = dim >> 2;
    if (i >= (long long)rows * d4) return;
    const int row = (int)(i / d4), c = (int)(i - (long long)row * d4) * 4;
    const long long id = ids[row];
    const f32x4 a = *(const f32x4*)(tok + id * dim + c);
    const f32x4 b = *(const f32x4*)(pos + (long long)(row % n_tokens) * dim + c);
    typename Op<T>::v4 o = {from_f32<T>(a[0] + b[0]), from_f32<T>(a[1] + b[1]), from_f32<T>(a[2] + b[2]), from_f32<T>(a[3] + b[3])};
    *(typename Op<T>::v4*)(out + (long long)row * dim + c) = o;
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

// blocks_for returns unsigned and a grid's x extent stays below 2^31: one call covers fewer than 2^31 * 256 = 2^39 elements.  The product
// of up to three positive sizes is taken in 128 bits (three int32 sizes, or two int64 ones, overflow a long long).
inline bool below_2p39(long long a, long long b = 1, long long c = 1) {
    const long long lim = 1LL << 39;
    if (a <= 0 || b <= 0 || c <= 0 || a >= lim || b >= lim || c >= lim) return false;
    return (unsigned __int128)a * (unsigned __int128)b * (unsigned __int128)c < (unsigned __int128)lim;
}

}  // namespace

#define DISPATCH_T(dtype, CALL_BF16, CALL_F16) \
    do {                                       \
        if ((dtype) == IDB_BF16) { CALL_BF16; } \
        else { CALL_F16; }                     \
    } while (0)

extern "C" int idb_timestep_sinusoid(const float* timesteps, float* out, int32_t n, int32_t dim, void* stream) {
    IDB_REQUIRE(timesteps && out && n > 0 && dim > 0 && dim % 2 == 0, "idb_timestep_sinusoid: bad args");
    hipLaunchKernelGGL(sinusoid_kernel, dim3(blocks_for((long long)n * dim / 2)), dim3(256), 0, (hipStream_t)stream, timesteps,
                       out, n, dim);
    IDB_CHECK_LAUNCH("idb_timestep_sinusoid");
    return IDB_OK;
}

extern "C" int idb_linear_f32(const float* x, const float* w, const float* bias, float* y, int32_t m, int32_t n, int32_t k,
                              int32_t silu_in, void* stream) {
    IDB_REQUIRE(x && w && y && m > 0 && n > 0 && k > 0, "idb_linear_f32: bad args");
    hipLaunchKernelGGL(linear_f32_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, m, n, k, silu_in);
    IDB_CHECK_LAUNCH("idb_linear_f32");
    return IDB_OK;
}

extern "C" int idb_conv_in(const float* x_nchw, const float* w, const float* bias, void* out, int32_t batch, int32_t rep,
                           int32_t cin, int32_t h, int32_t w_, int32_t cout, float in_scale, const float* pre_w,
                           const float* pre_b, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_conv_in: dtype must be bf16/f16");
    IDB_REQUIRE(x_nchw && w && bias && out && idb_aligned16(out), "idb_conv_in: null/unaligned pointer");
    IDB_REQUIRE(batch > 0 && rep > 0 && cin > 0 && cin <= 4 && h > 0 && w_ > 0 && cout > 0 && cout % 8 == 0,
                "idb_conv_in: unsupported dims (cin<=4, cout%%8==0)");
    IDB_REQUIRE((pre_w == nullptr) == (pre_b == nullptr), "idb_conv_in: pre_w/pre_b must both be given");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(blocks_for((long long)batch * h * w_), cout / 8);
    DISPATCH_T(dtype,
               hipLaunchKernelGGL((conv_in_kernel<__bf16>), grid, dim3(256), 0, st, x_nchw, w, bias, (__bf16*)out, batch, rep,
                                  cin, h, w_, cout, in_scale, pre_w, pre_b),
               hipLaunchKernelGGL((conv_in_kernel<_Float16>), grid, dim3(256), 0, st, x_nchw, w, bias, (_Float16*)out, batch,
                                  rep, cin, h, w_, cout, in_scale, pre_w, pre_b));
    IDB_CHECK_LAUNCH("idb_conv_in");
    return IDB_OK;
}

extern "C" int idb_cfg_ddpm_step(const float* eps, float* latents, const float* noise, const float* coef, float* x0_out,
                                 int32_t batch, int32_t channels, int32_t hw, int32_t cfg, int32_t prediction_type,
                                 void* stream) {
    IDB_REQUIRE(eps && latents && coef && batch > 0 && channels > 0 && hw > 0, "idb_cfg_ddpm_step: bad args");
    IDB_REQUIRE(prediction_type == 0 || prediction_type == 1, "idb_cfg_ddpm_step: prediction_type must be 0 (epsilon) or 1 (v)");
    IDB_REQUIRE(below_2p39(batch, channels, hw), "idb_cfg_ddpm_step: 2^39 or more elements");
    hipLaunchKernelGGL(cfg_ddpm_kernel, dim3(blocks_for((long long)batch * channels * hw)), dim3(256), 0, (hipStream_t)stream,
                       eps, latents, noise, coef, x0_out, batch, channels, hw, cfg, prediction_type);
    IDB_CHECK_LAUNCH("idb_cfg_ddpm_step");
    return IDB_OK;
}

extern "C" int idb_warp_affine_u8(const uint8_t* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const double* m_inv,
                                  uint8_t* dst, int32_t out_h, int32_t out_w, int32_t border_value, void* stream) {
    IDB_REQUIRE(src && m_inv && dst && batch > 0 && h > 0 && w > 0 && channels > 0 && channels <= 4 && out_h > 0 && out_w > 0,
                "idb_warp_affine_u8: bad args");
    IDB_REQUIRE(h < (1 << 20) && w < (1 << 20) && border_value >= 0 && border_value <= 255, "idb_warp_affine_u8: size/border out of range");
    hipLaunchKernelGGL(warp_affine_u8_kernel, dim3(blocks_for((long long)batch * out_h * out_w)), dim3(256), 0, (hipStream_t)stream, src,
                       batch, h, w, channels, m_inv, dst, out_h, out_w, border_value);
    IDB_CHECK_LAUNCH("idb_warp_affine_u8");
    return IDB_OK;
}

extern "C" int idb_vae_sample(const float* moments, const float* noise, float scale, float* latents, float* mean_out,
                              float* logvar_out, int32_t batch, int32_t channels, int32_t hw, void* stream) {
    IDB_REQUIRE(moments && latents && batch > 0 && channels > 0 && hw > 0, "idb_vae_sample: bad args");
    IDB_REQUIRE(below_2p39(batch, channels, hw) && channels < (1 << 30), "idb_vae_sample: 2^39 or more elements, or 2^30 or more channels");
    hipLaunchKernelGGL(vae_sample_kernel, dim3(blocks_for((long long)batch * channels * hw)), dim3(256), 0, (hipStream_t)stream,
                       moments, noise, scale, latents, mean_out, logvar_out, batch, channels, hw);
    IDB_CHECK_LAUNCH("idb_vae_sample");
    return IDB_OK;
}

extern "C" int idb_postprocess(const float* x, float* img01, uint8_t* u8, int64_t count, void* stream) {
    IDB_REQUIRE(x && (img01 || u8) && count > 0, "idb_postprocess: bad args");
    IDB_REQUIRE(below_2p39(count), "idb_postprocess: 2^39 or more elements");
    hipLaunchKernelGGL(postprocess_kernel, dim3(blocks_for(count)), dim3(256), 0, (hipStream_t)stream, x, img01, u8,
                       (long long)count);
    IDB_CHECK_LAUNCH("idb_postprocess");
    return IDB_OK;
}

extern "C" int idb_nhwc_to_nchw_f32(const void* x, float* out, int32_t batch, int32_t hw, int32_t c, int32_t dtype,
                                    void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && x && out && batch > 0 && hw > 0 && c > 0, "idb_nhwc_to_nchw_f32: bad args");
    IDB_REQUIRE(below_2p39(batch, hw, c), "idb_nhwc_to_nchw_f32: 2^39 or more elements");
    const unsigned nb = blocks_for((long long)batch * hw * c);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((nhwc_to_nchw_kernel<__bf16>), dim3(nb), dim3(256), 0, st, (const __bf16*)x, out, batch, hw, c),
               hipLaunchKernelGGL((nhwc_to_nchw_kernel<_Float16>), dim3(nb), dim3(256), 0, st, (const _Float16*)x, out, batch, hw, c));
    IDB_CHECK_LAUNCH("idb_nhwc_to_nchw_f32");
    return IDB_OK;
}

extern "C" int idb_f32_nhwc_to_nchw(const float* x, float* out, int32_t batch, int32_t hw, int32_t c, void* stream) {
    IDB_REQUIRE(x && out && batch > 0 && hw > 0 && c > 0, "idb_f32_nhwc_to_nchw: bad args");
    IDB_REQUIRE(below_2p39(batch, hw, c), "idb_f32_nhwc_to_nchw: 2^39 or more elements");
    hipLaunchKernelGGL((nhwc_to_nchw_kernel<float>), dim3(blocks_for((long long)batch * hw * c)), dim3(256), 0,
                       (hipStream_t)stream, x, out, batch, hw, c);
    IDB_CHECK_LAUNCH("idb_f32_nhwc_to_nchw");
    return IDB_OK;
}

extern "C" int idb_cast_f32(const float* x, void* out, int64_t count, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && x && out && count > 0, "idb_cast_f32: bad args");
    IDB_REQUIRE(below_2p39(count), "idb_cast_f32: 2^39 or more elements");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((cast_kernel<__bf16>), dim3(blocks_for(count)), dim3(256), 0, st, x, (__bf16*)out, (long long)count),
               hipLaunchKernelGGL((cast_kernel<_Float16>), dim3(blocks_for(count)), dim3(256), 0, st, x, (_Float16*)out, (long long)count));
    IDB_CHECK_LAUNCH("idb_cast_f32");
    return IDB_OK;
}

extern "C" int idb_embed_tokens(const int64_t* ids, const float* tok, const float* pos, void* out, int32_t batch, int32_t n_tokens,
                                int32_t dim, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && ids && tok && pos && out, "idb_embed_tokens: bad args");
    IDB_REQUIRE(batch > 0 && n_tokens > 0 && dim > 0 && dim % 4 == 0 && idb_aligned16(tok) && idb_aligned16(pos) && idb_aligned16(out),
                "idb_embed_tokens: dims/alignment");
    IDB_REQUIRE(below_2p39(batch, n_tokens, dim) && (long long)batch * n_tokens < (1LL << 31),
                "idb_embed_tokens: 2^39 or more elements, or 2^31 or more rows");
    const int rows = batch * n_tokens;
    const unsigned nb = blocks_for((long long)rows * (dim / 4));
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((embed_kernel<__bf16>), dim3(nb), dim3(256), 0, st, (const long long*)ids, tok, pos, (__bf16*)out, rows, n_tokens, dim),
               hipLaunchKernelGGL((embed_kernel<_Float16>), dim3(nb), dim3(256), 0, st, (const long long*)ids, tok, pos, (_Float16*)out, rows, n_tokens, dim));
    IDB_CHECK_LAUNCH("idb_embed_tokens");
    return IDB_OK;
}

extern "C" int idb_pack_conv_weight(const float* src, void* dst, int32_t cout, int32_t cin, int32_t ktaps, int32_t dtype,
                                    void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && src && dst && cout > 0 && cin > 0 && ktaps > 0, "idb_pack_conv_weight: bad args");
    IDB_REQUIRE(below_2p39(cout, cin, ktaps), "idb_pack_conv_weight: 2^39 or more elements");
    const unsigned nb = blocks_for((long long)cout * cin * ktaps);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((pack_conv_kernel<__bf16>), dim3(nb), dim3(256), 0, st, src, (__bf16*)dst, cout, cin, ktaps),
               hipLaunchKernelGGL((pack_conv_kernel<_Float16>), dim3(nb), dim3(256), 0, st, src, (_Float16*)dst, cout, cin, ktaps));
    IDB_CHECK_LAUNCH("idb_pack_conv_weight");
    return IDB_OK;
}

extern "C" int idb_pack_matrix(const float* src, void* dst, int64_t rows, int64_t cols, int32_t geglu, int32_t dtype,
                               void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && src && dst && rows > 0 && cols > 0, "idb_pack_matrix: bad args");
    IDB_REQUIRE(!geglu || rows % 32 == 0, "idb_pack_matrix: GEGLU packing needs rows %% 32 == 0");
    IDB_REQUIRE(below_2p39(rows, cols), "idb_pack_matrix: 2^39 or more elements");
    const unsigned nb = blocks_for(rows * cols);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((pack_matrix_kernel<__bf16>), dim3(nb), dim3(256), 0, st, src, (__bf16*)dst, (long long)rows, (long long)cols, geglu),
               hipLaunchKernelGGL((pack_matrix_kernel<_Float16>), dim3(nb), dim3(256), 0, st, src, (_Float16*)dst, (long long)rows, (long long)cols, geglu));
    IDB_CHECK_LAUNCH("idb_pack_matrix");
    return IDB_OK;
}

extern "C" int idb_pack_matrix_scaled(const float* src, void* dst, int64_t rows, int64_t cols, int32_t geglu, const float* col_scale,
                                      int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && src && dst && col_scale && rows > 0 && cols > 0, "idb_pack_matrix_scaled: bad args");
    IDB_REQUIRE(!geglu || rows % 32 == 0, "idb_pack_matrix_scaled: GEGLU packing needs rows %% 32 == 0");
    IDB_REQUIRE(below_2p39(rows, cols), "idb_pack_matrix_scaled: 2^39 or more elements");
    const unsigned nb = blocks_for(rows * cols);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((pack_matrix_scaled_kernel<__bf16>), dim3(nb), dim3(256), 0, st, src, (__bf16*)dst, (long long)rows, (long long)cols, geglu, col_scale),
               hipLaunchKernelGGL((pack_matrix_scaled_kernel<_Float16>), dim3(nb), dim3(256), 0, st, src, (_Float16*)dst, (long long)rows, (long long)cols, geglu, col_scale));
    IDB_CHECK_LAUNCH("idb_pack_matrix_scaled");
    return IDB_OK;
}

extern "C" int idb_ln_fold_vectors(const float* w, const float* lora_a, const float* lora_b, int32_t rank, float scale, const void* w_folded,
                                   const float* beta, const float* bias, float* u, float* v, int64_t rows, int64_t cols, int32_t geglu,
                                   int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && w && w_folded && beta && u && v && rows > 0 && cols > 0 && rank >= 0 && rank <= 16 &&
                    (rank == 0 || !lora_a || lora_b), "idb_ln_fold_vectors: bad args");
    IDB_REQUIRE(!geglu || rows % 32 == 0, "idb_ln_fold_vectors: GEGLU row order needs rows %% 32 == 0");
    IDB_REQUIRE(below_2p39(rows, cols) && rows < (1LL << 33), "idb_ln_fold_vectors: 2^39 or more elements, or 2^33 or more rows (four per workgroup)");
    const int rk = lora_a ? rank : 0;
    const unsigned nb = (unsigned)((rows + 3) / 4);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((ln_fold_vectors_kernel<__bf16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, rk, scale, (const __bf16*)w_folded, beta, bias, u, v, (long long)rows, (long long)cols, geglu),
               hipLaunchKernelGGL((ln_fold_vectors_kernel<_Float16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, rk, scale, (const _Float16*)w_folded, beta, bias, u, v, (long long)rows, (long long)cols, geglu));
    IDB_CHECK_LAUNCH("idb_ln_fold_vectors");
    return IDB_OK;
}

extern "C" size_t idb_tiled_weight_bytes(int64_t n, int64_t k) { return n > 0 && k > 0 ? (size_t)((n + 15) / 16 * 16 * k * 2) : 0; }

extern "C" int idb_tile_weight(const void* src, void* dst, int64_t n, int64_t k, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && src && dst && n > 0 && k > 0 && k % 64 == 0 && idb_aligned16(src) && idb_aligned16(dst),
                "idb_tile_weight: needs operand dtype, 16-byte aligned pointers, k %% 64 == 0");
    IDB_REQUIRE(n < (1LL << 39) && below_2p39((n + 15) / 16 * 16, k), "idb_tile_weight: 2^39 or more elements");
    const unsigned nb = blocks_for((n + 15) / 16 * (k / 64) * 128);
    hipLaunchKernelGGL(tile_weight_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (uint4*)dst, (long long)n, (long long)k);
    IDB_CHECK_LAUNCH("idb_tile_weight");
    return IDB_OK;
}

extern "C" int idb_lora_merge_scaled(const float* w, const float* lora_a, const float* lora_b, void* dst, int64_t rows, int64_t cols,
                                     int32_t rank, float scale, const float* col_scale, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && w && dst && col_scale && rows > 0 && cols > 0 && rank >= 0 && ((lora_a && lora_b) || rank == 0),
                "idb_lora_merge_scaled: bad args");
    IDB_REQUIRE(below_2p39(rows, cols), "idb_lora_merge_scaled: 2^39 or more elements");
    const unsigned nb = blocks_for(rows * cols);
    hipStream_t st = (hipStream_t)stream;
    const int rk = lora_a ? rank : 0;
    DISPATCH_T(dtype, hipLaunchKernelGGL((lora_merge_scaled_kernel<__bf16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, (__bf16*)dst, (long long)rows, (long long)cols, rk, scale, col_scale),
               hipLaunchKernelGGL((lora_merge_scaled_kernel<_Float16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, (_Float16*)dst, (long long)rows, (long long)cols, rk, scale, col_scale));
    IDB_CHECK_LAUNCH("idb_lora_merge_scaled");
    return IDB_OK;
}

extern "C" int idb_lora_merge(const float* w, const float* lora_a, const float* lora_b, void* dst, int64_t rows, int64_t cols,
                              int32_t rank, float scale, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype) && w && lora_a && lora_b && dst && rows > 0 && cols > 0 && rank > 0,
                "idb_lora_merge: bad args");
    IDB_REQUIRE(below_2p39(rows, cols), "idb_lora_merge: 2^39 or more elements");
    const unsigned nb = blocks_for(rows * cols);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, hipLaunchKernelGGL((lora_merge_kernel<__bf16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, (__bf16*)dst, (long long)rows, (long long)cols, rank, scale),
               hipLaunchKernelGGL((lora_merge_kernel<_Float16>), dim3(nb), dim3(256), 0, st, w, lora_a, lora_b, (_Float16*)dst, (long long)rows, (long long)cols, rank, scale));
    IDB_CHECK_LAUNCH("idb_lora_merge");
    return IDB_OK;
}
