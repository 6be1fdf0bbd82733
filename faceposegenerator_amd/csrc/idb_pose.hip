// 6DRepNet head pose (sixdrepnet SixDRepNet_Detector: RepVGG-B1g2 in deploy form + a 6D rotation head; ID-Booth's
// Evaluation/PoseEstimation notebook): the pieces that are not implicit GEMMs.  The 27 3x3 blocks after the stem run on idb_gemm
// (act = 3, ReLU); faceposegenerator_amd/headpose.py drives them.
//   resize: Pillow's antialiased BILINEAR resize (torchvision Resize on a PIL image) of the zero-padded uint8 image, bit-exact;
//           the same passes with the BICUBIC filter serve DINOv2's transform (idb_resize_bicubic_aa_u8)
//   stem:   /255, ImageNet normalisation, conv 3->64 3x3 stride 2 pad 1 + bias + ReLU — 3 input channels: VALU work
//   head:   global average pool, linear 2048->6, Gram-Schmidt to a rotation matrix, Euler angles in degrees, all fp32
#include "idb_common.h"

namespace {

// ---- resize ------------------------------------------------------------------------------------------------------------------
// Pillow (libImaging/Resample.c, 8-bit path), restated: per output index o of an axis of `in` -> `out` samples,
//   scale = in / out, fs = max(scale, 1), support = fs, center = (o + 0.5) scale,
//   taps xmin = max(int(center - support + 0.5), 0) .. xmax = min(int(center + support + 0.5), in) exclusive,
//   w_i = max(0, 1 - |(i + xmin - center + 0.5) / fs|) normalised to sum 1 (double), k_i = int(w_i 2^22 + 0.5) (w_i >= 0),
// and each pass sums 2^21 + sum k_i v_i in integers, shifts right by 22 and clips to [0, 255].  The horizontal pass runs first and
// its uint8 result feeds the vertical pass.  Both axes have the same coefficients (square images).  The double arithmetic must not
// be contracted into FMAs: Pillow's x86 build rounds every product and sum.
constexpr int RS_KMAX = 16, RS_DMAX = 256, RS_PREC = 22;
// The filters of Resample.c: BILINEAR (support 1) and BICUBIC (Keys cubic with a = -0.5, support 2), in Pillow's operation order.
enum { RS_BILINEAR = 0, RS_BICUBIC = 1 };

template <int FILTER>
__device__ __forceinline__ double resize_filter(double t) {
#pragma clang fp contract(off)
    if (t < 0.0) t = -t;
    if constexpr (FILTER == RS_BILINEAR) return t < 1.0 ? 1.0 - t : 0.0;
    if (t < 1.0) return (1.5 * t - 2.5) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * -0.5;
    return 0.0;
}

template <int FILTER>
__device__ int resize_coeffs(int o, int in, int out, int* k) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (FILTER == RS_BICUBIC ? 2.0 : 1.0) * fs, ss = 1.0 / fs;
    const double center = (o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double w[RS_KMAX], ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        w[x] = resize_filter<FILTER>((x + xmin - center + 0.5) * ss);
        ww += w[x];
    }
    for (int x = 0; x < RS_KMAX; ++x) {
        double v = x < xmax && ww != 0.0 ? w[x] / ww : 0.0;
        k[x] = x < xmax ? (int)(v < 0 ? -0.5 + v * (1 << RS_PREC) : 0.5 + v * (1 << RS_PREC)) : 0;
    }
    return xmin | (xmax << 16);
}

__device__ __forceinline__ unsigned char clip8(int ss) {
    const int v = ss >> RS_PREC;
    return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// One workgroup per (output row, image).  Coefficients for all D output columns (= rows) into LDS; the horizontal pass then produces
// only the <= RS_KMAX padded input rows this output row reads, and the vertical pass combines them.  An input row is thus resampled
// horizontally by every output row whose window covers it (about 2-3 rows at 572 -> 224): cheaper than a workspace round trip.
// Sums stay below 2^31: 255 * sum |k_i| < 255 * 2^22 * 1.5 (the bicubic lobes add up to less than 1.5 in absolute value).
template <int FILTER>
__global__ __launch_bounds__(256) void resize_aa_kernel(const unsigned char* __restrict__ src, int S, int pad, int D,
                                                        unsigned char* __restrict__ dst) {
    __shared__ int kc[RS_DMAX][RS_KMAX];
    __shared__ int kb[RS_DMAX];                      // xmin | taps << 16
    __shared__ unsigned char rows[RS_KMAX][RS_DMAX * 3];
    const int oy = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int P = S + 2 * pad;
    for (int o = tid; o < D; o += 256) kb[o] = resize_coeffs<FILTER>(o, P, D, kc[o]);
    __syncthreads();
    const int y0 = kb[oy] & 0xffff, ny = kb[oy] >> 16;
    const unsigned char* img = src + (long long)b * S * S * 3;
    for (int t = tid; t < ny * D * 3; t += 256) {
        const int r = t / (D * 3), rem = t - r * (D * 3), ox = rem / 3, c = rem - ox * 3;
        const int iy = y0 + r - pad;
        const int x0 = kb[ox] & 0xffff, nx = kb[ox] >> 16;
        int ss = 1 << (RS_PREC - 1);
        if ((unsigned)iy < (unsigned)S) {
            for (int i = 0; i < nx; ++i) {
                const int ix = x0 + i - pad;
                if ((unsigned)ix < (unsigned)S) ss += (int)img[((long long)iy * S + ix) * 3 + c] * kc[ox][i];
            }
        }
        rows[r][rem] = clip8(ss);
    }
    __syncthreads();
    unsigned char* out = dst + ((long long)b * D + oy) * D * 3;
    for (int t = tid; t < D * 3; t += 256) {
        int ss = 1 << (RS_PREC - 1);
        for (int r = 0; r < ny; ++r) ss += (int)rows[r][t] * kc[oy][r];
        out[t] = clip8(ss);
    }
}

// ---- stem --------------------------------------------------------------------------------------------------------------------
constexpr int PS_C = 64, PS_MAXW = 256;

// One workgroup per (output row, image).  The three input rows of the stride-2 window, normalised in fp32 ((u / 255 - mean) / std
// for uint8 NHWC, as ToTensor + Normalize; fp32 NCHW taken as is), are staged in LDS with the zero padding; each thread then owns
// 8 output channels of one pixel: 27 taps x 8 FMAs in fp32, bias, ReLU, one rounding to the operand dtype.
template <typename T, bool U8>
__global__ __launch_bounds__(256) void pose_stem_kernel(const void* __restrict__ x, int H, int W, const float* __restrict__ wgt,
                                                        const float* __restrict__ bias, T* __restrict__ out) {
    using V8 = typename Op<T>::v8;
    __shared__ float sw[PS_C * 27];
    __shared__ float sx[3][2 * PS_MAXW + 2][3];
    const int y = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int OW = (W + 1) / 2;
    for (int i = tid; i < PS_C * 27; i += 256) sw[i] = wgt[i];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const int row_elems = (W + 2) * 3;
    for (int i = tid; i < 3 * row_elems; i += 256) {
        const int r = i / row_elems, rem = i - r * row_elems, px = rem / 3, c = rem - px * 3;
        const int iy = 2 * y - 1 + r, ix = px - 1;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
            if constexpr (U8) {
                const float u = (float)((const uint8_t*)x)[(((long long)b * H + iy) * W + ix) * 3 + c];
                v = (u / 255.f - mean[c]) / stdv[c];
            } else {
                v = ((const float*)x)[(((long long)b * 3 + c) * H + iy) * W + ix];
            }
        }
        sx[r][px][c] = v;
    }
    __syncthreads();
    for (int t = tid; t < OW * 8; t += 256) {
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
                    const float xv = sx[ky][2 * px + kx][ci];
                    const int tap = (ky * 3 + kx) * 3 + ci;
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(xv, sw[(c0 + k) * 27 + tap], acc[k]);
                }
        V8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = from_f32<T>(fmaxf(acc[k], 0.f));
        *(V8*)(out + (((long long)b * ((H + 1) / 2) + y) * OW + px) * PS_C + c0) = o;
    }
}

// ---- head --------------------------------------------------------------------------------------------------------------------
// One workgroup per image.  Thread t owns channels 8t' .. 8t'+7 for t' = t, t + 256, ...: the pixel mean in ascending pixel order,
// then its share of the 6 dot products; a fixed shuffle tree and the 4 wave sums in wave order finish them (deterministic).
// Thread 0 then runs the 6D head in fp32: x = a / max(|a|, 1e-8), z = normalize(x cross b), y = z cross x, R = [x y z] (columns),
// sy = sqrt(R00^2 + R10^2); pitch = atan2(R21, R22), yaw = atan2(-R20, sy), roll = atan2(R10, R00), or when sy < 1e-6
// pitch = atan2(-R12, R11), roll = 0; degrees.
template <typename T>
__global__ __launch_bounds__(256) void pose_head_kernel(const T* __restrict__ x, int HW, int C, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ R, float* __restrict__ ang) {
    using V8 = typename Op<T>::v8;
    __shared__ float red[4][6];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const T* xb = x + (long long)b * HW * C;
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int cg = tid; cg < C / 8; cg += 256) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < HW; ++p) {
            const V8 v = *(const V8*)(xb + (long long)p * C + cg * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += to_f32<T>(v[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float m = s[e] / (float)HW;
#pragma unroll
            for (int j = 0; j < 6; ++j) d[j] = __builtin_fmaf(m, w[(long long)j * C + cg * 8 + e], d[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) d[j] += __shfl_xor(d[j], o, 64);
        if (lane == 0) red[wv][j] = d[j];
    }
    __syncthreads();
    if (tid != 0) return;
    float o6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) o6[j] = ((red[0][j] + red[1][j]) + (red[2][j] + red[3][j])) + bias[j];
    float xv[3] = {o6[0], o6[1], o6[2]}, bv[3] = {o6[3], o6[4], o6[5]};
    float n = fmaxf(sqrtf(xv[0] * xv[0] + xv[1] * xv[1] + xv[2] * xv[2]), 1e-8f);
#pragma unroll
    for (int e = 0; e < 3; ++e) xv[e] /= n;
    float z[3] = {xv[1] * bv[2] - xv[2] * bv[1], xv[2] * bv[0] - xv[0] * bv[2], xv[0] * bv[1] - xv[1] * bv[0]};
    n = fmaxf(sqrtf(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]), 1e-8f);
#pragma unroll
    for (int e = 0; e < 3; ++e) z[e] /= n;
    const float y[3] = {z[1] * xv[2] - z[2] * xv[1], z[2] * xv[0] - z[0] * xv[2], z[0] * xv[1] - z[1] * xv[0]};
    float* r = R + (long long)b * 9;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r[i * 3 + 0] = xv[i];
        r[i * 3 + 1] = y[i];
        r[i * 3 + 2] = z[i];
    }
    const float sy = sqrtf(xv[0] * xv[0] + xv[1] * xv[1]);
    const float deg = 180.f / 3.14159265358979323846f;
    float pitch, roll;
    if (sy < 1e-6f) {
        pitch = atan2f(-z[1], y[1]);
        roll = 0.f;
    } else {
        pitch = atan2f(y[2], z[2]);
        roll = atan2f(xv[1], xv[0]);
    }
    const float yaw = atan2f(-xv[2], sy);
    ang[(long long)b * 3 + 0] = pitch * deg;
    ang[(long long)b * 3 + 1] = yaw * deg;
    ang[(long long)b * 3 + 2] = roll * deg;
}

}  // namespace

// filter: the taps one output sample reads are at most ceil(support) * 2 + 1 (Resample.c's ksize), support = (1 or 2) max(P / d, 1)
template <int FILTER>
static int resize_launch(const char* api, const void* src, int32_t batch, int32_t s, int32_t pad, int32_t d, void* dst, void* stream) {
    IDB_REQUIRE(src && dst, "%s: null pointer", api);
    IDB_REQUIRE(batch > 0 && batch <= 65535 && s > 0 && pad >= 0 && d > 0 && d <= RS_DMAX && (long long)s * s * 3 * batch < (1LL << 40),
                "%s: batch 1..65535, s > 0, pad >= 0, d 1..%d", api, RS_DMAX);
    const long long P = (long long)s + 2LL * pad;
    const double fs = (double)P / d < 1.0 ? 1.0 : (double)P / d;
    const double support = (FILTER == RS_BICUBIC ? 2.0 : 1.0) * fs;
    IDB_REQUIRE(P < 65536 && (int)ceil(support) * 2 + 1 <= RS_KMAX, "%s: reduction %lld -> %d needs more than %d taps", api, P, d, RS_KMAX);
    hipLaunchKernelGGL((resize_aa_kernel<FILTER>), dim3(d, batch), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src, s, pad, d,
                       (unsigned char*)dst);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

extern "C" int idb_resize_aa_u8(const void* src, int32_t batch, int32_t s, int32_t pad, int32_t d, void* dst, void* stream) {
    return resize_launch<RS_BILINEAR>("idb_resize_aa_u8", src, batch, s, pad, d, dst, stream);
}

extern "C" int idb_resize_bicubic_aa_u8(const void* src, int32_t batch, int32_t s, int32_t d, void* dst, void* stream) {
    return resize_launch<RS_BICUBIC>("idb_resize_bicubic_aa_u8", src, batch, s, 0, d, dst, stream);
}

extern "C" int idb_pose_stem(const void* x, int32_t x_u8, int32_t batch, int32_t h, int32_t w, const float* weight, const float* bias,
                             void* out, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_pose_stem: dtype must be bf16/f16");
    IDB_REQUIRE(x && weight && bias && out && idb_aligned16(out), "idb_pose_stem: null or unaligned pointer");
    IDB_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && w > 0 && w <= 2 * PS_MAXW, "idb_pose_stem: batch 1..65535, width 1..%d", 2 * PS_MAXW);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((h + 1) / 2, batch);
#define IDB_PSTEM(T, U) hipLaunchKernelGGL((pose_stem_kernel<T, U>), grid, dim3(256), 0, st, x, h, w, weight, bias, (T*)out)
    if (dtype == IDB_BF16) {
        if (x_u8) IDB_PSTEM(__bf16, true);
        else IDB_PSTEM(__bf16, false);
    } else {
        if (x_u8) IDB_PSTEM(_Float16, true);
        else IDB_PSTEM(_Float16, false);
    }
#undef IDB_PSTEM
    IDB_CHECK_LAUNCH("idb_pose_stem");
    return IDB_OK;
}

extern "C" int idb_pose_head(const void* x, int32_t batch, int32_t hw, int32_t c, const float* weight, const float* bias, float* rot,
                             float* angles, int32_t dtype, void* stream) {
    IDB_REQUIRE(idb_is_operand_dtype(dtype), "idb_pose_head: dtype must be bf16/f16");
    IDB_REQUIRE(x && weight && bias && rot && angles && idb_aligned16(x), "idb_pose_head: null or unaligned pointer");
    IDB_REQUIRE(batch > 0 && hw > 0 && c > 0 && c % 8 == 0, "idb_pose_head: batch > 0, hw > 0, c %% 8 == 0");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL((pose_head_kernel<__bf16>), dim3(batch), dim3(256), 0, st, (const __bf16*)x, hw, c, weight, bias, rot, angles);
    else
        hipLaunchKernelGGL((pose_head_kernel<_Float16>), dim3(batch), dim3(256), 0, st, (const _Float16*)x, hw, c, weight, bias, rot, angles);
    IDB_CHECK_LAUNCH("idb_pose_head");
    return IDB_OK;
}
