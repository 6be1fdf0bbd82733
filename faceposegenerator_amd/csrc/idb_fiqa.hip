// CR-FIQA face-image quality (ID-Booth's Evaluation/CR-FIQA/getQualityScore_FR_ID-Booth_12-2024.py): the two pieces around the
// IResNet that the ArcFace kernels do not serve.  The network itself is idb_arcface_stem / idb_gemm / idb_arcface_head;
// faceposegenerator_amd/fiqa.py drives them.
//   resize: OpenCV's cv2.resize(img, (dw, dh)) with INTER_LINEAR on 8-bit data, bit-exact with its fixed-point arithmetic, and the
//           BGR order of cv2.imread as a channel swap on the way out
//   tail:   the qs linear head on the embeddings and sklearn's l2 normalize of them, accumulated in double
#include "idb_common.h"

namespace {

// ---- resize ------------------------------------------------------------------------------------------------------------------
// OpenCV (imgproc resize.cpp: HResizeLinear / VResizeLinear for uchar, int, short), restated.  Per axis the caller supplies, for every
// destination index, the first source index o and the int16 coefficient pair (c0, c1) on an 11-bit scale; the second tap is
// min(o + 1, size - 1) and its coefficient is 0 wherever that clamp acts.  The tables are built on the host (fiqa.coef_tables) with
// OpenCV's float32 / float64 types, so nothing here depends on how the device compiler contracts float expressions: the kernel is
// integer arithmetic only.
//   horizontal, int32:  r(y, x) = S[y][o_x] c0_x + S[y][o_x + 1] c1_x                 (<= 255 * 2048 < 2^20)
//   vertical:           out = (((b0 (r(o_y, x) >> 4)) >> 16) + ((b1 (r(o_y + 1, x) >> 4)) >> 16) + 2) >> 2, saturated to 8 bits
// One thread per destination pixel (3 channels): 4 source pixels of 3 adjacent bytes each.  Neighbouring threads read neighbouring
// source pixels of the same two rows, so a wave touches every cache line of the row segment it covers once, and the two rows of a
// destination row are the only ones read (512 -> 112 reads about 2 of every 4.57 rows).  Offsets are clamped to the image: a bad
// table cannot make the kernel read outside the source.
__global__ __launch_bounds__(256) void resize_linear_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                            const int* __restrict__ ofs_x, const short2* __restrict__ coef_x,
                                                            const int* __restrict__ ofs_y, const short2* __restrict__ coef_y, int dh,
                                                            int dw, int swap, unsigned char* __restrict__ dst) {
    const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (p >= dh * dw) return;
    const int oy = p / dw, ox = p - oy * dw;
    const int x0 = min(max(ofs_x[ox], 0), W - 1), x1 = min(x0 + 1, W - 1);
    const int y0 = min(max(ofs_y[oy], 0), H - 1), y1 = min(y0 + 1, H - 1);
    const short2 a = coef_x[ox], bb = coef_y[oy];
    const unsigned char* img = src + (long long)b * H * W * 3;
    const unsigned char* r0 = img + (long long)y0 * W * 3;
    const unsigned char* r1 = img + (long long)y1 * W * 3;
    unsigned char* out = dst + ((long long)b * dh * dw + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = (int)r0[x0 * 3 + c] * a.x + (int)r0[x1 * 3 + c] * a.y;
        const int h1 = (int)r1[x0 * 3 + c] * a.x + (int)r1[x1 * 3 + c] * a.y;
        const int v = (((bb.x * (h0 >> 4)) >> 16) + ((bb.y * (h1 >> 4)) >> 16) + 2) >> 2;
        out[swap ? 2 - c : c] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
}

// H == 2 dh and W == 2 dw: OpenCV turns INTER_LINEAR into its fast area path, the 2x2 box (a + b + c + d + 2) >> 2.
__global__ __launch_bounds__(256) void resize_box2_kernel(const unsigned char* __restrict__ src, int dh, int dw, int swap,
                                                          unsigned char* __restrict__ dst) {
    const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (p >= dh * dw) return;
    const int oy = p / dw, ox = p - oy * dw;
    const long long row = (long long)dw * 6;                    // source row: 2 dw pixels of 3 bytes
    const unsigned char* r0 = src + (long long)b * dh * 2 * row + (long long)oy * 2 * row + ox * 6;
    const unsigned char* r1 = r0 + row;
    unsigned char* out = dst + ((long long)b * dh * dw + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[swap ? 2 - c : c] = (unsigned char)(((int)r0[c] + r0[3 + c] + r1[c] + r1[3 + c] + 2) >> 2);
}

// ---- tail --------------------------------------------------------------------------------------------------------------------
// One wave per embedding row, four rows per workgroup.  Lane l takes elements l, l + 64, ... in ascending order: the dot product with
// the qs weight and the sum of squares in double (a product of two fp32 numbers is exact in double), then a fixed shuffle tree over
// the 64 lanes.  qs = fp32(dot + bias): one rounding.  x / sqrt(sum x^2) in double, rounded to fp32 once; a zero row stays zero
// (sklearn's normalize divides such a row by 1).  No atomics: bit-identical from run to run.
__global__ __launch_bounds__(256) void fiqa_tail_kernel(const float* __restrict__ emb, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int B, int D, float* __restrict__ qs,
                                                        float* __restrict__ emb_norm) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                          // whole waves leave together: no shuffle crosses a row
    const float* e = emb + (long long)b * D;
    double dot = 0.0, ss = 0.0;
    for (int i = lane; i < D; i += 64) {
        const double v = (double)e[i];
        dot += v * (double)w[i];
        ss += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dot += __shfl_xor(dot, o, 64);
        ss += __shfl_xor(ss, o, 64);
    }
    if (lane == 0) qs[b] = (float)(dot + (double)bias[0]);
    const double n = ss == 0.0 ? 1.0 : sqrt(ss);
    float* o = emb_norm + (long long)b * D;
    for (int i = lane; i < D; i += 64) o[i] = (float)((double)e[i] / n);
}

static inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

extern "C" int idb_resize_linear_u8(const void* src, int32_t batch, int32_t h, int32_t w, const int32_t* ofs_x, const int16_t* coef_x,
                                    const int32_t* ofs_y, const int16_t* coef_y, int32_t dh, int32_t dw, int32_t swap_rb, void* dst,
                                    void* stream) {
    IDB_REQUIRE(src && dst && ofs_x && coef_x && ofs_y && coef_y, "idb_resize_linear_u8: null pointer");
    IDB_REQUIRE(aligned4(ofs_x) && aligned4(coef_x) && aligned4(ofs_y) && aligned4(coef_y),
                "idb_resize_linear_u8: the coefficient tables must be 4-byte aligned");
    IDB_REQUIRE(batch > 0 && batch <= 65535 && h > 0 && h <= 32768 && w > 0 && w <= 32768 && dh > 0 && dh <= 32768 && dw > 0 && dw <= 32768,
                "idb_resize_linear_u8: batch 1..65535, h, w, dh, dw 1..32768");
    const dim3 grid((unsigned)(((long long)dh * dw + 255) / 256), batch);
    hipStream_t st = (hipStream_t)stream;
    if (h == 2 * dh && w == 2 * dw)
        hipLaunchKernelGGL(resize_box2_kernel, grid, dim3(256), 0, st, (const unsigned char*)src, dh, dw, swap_rb != 0, (unsigned char*)dst);
    else
        hipLaunchKernelGGL(resize_linear_kernel, grid, dim3(256), 0, st, (const unsigned char*)src, h, w, ofs_x, (const short2*)coef_x, ofs_y,
                           (const short2*)coef_y, dh, dw, swap_rb != 0, (unsigned char*)dst);
    IDB_CHECK_LAUNCH("idb_resize_linear_u8");
    return IDB_OK;
}

extern "C" int idb_fiqa_tail(const float* emb, const float* weight, const float* bias, int32_t batch, int32_t d, float* qs,
                             float* emb_norm, void* stream) {
    IDB_REQUIRE(emb && weight && bias && qs && emb_norm, "idb_fiqa_tail: null pointer");
    IDB_REQUIRE(aligned4(emb) && aligned4(weight) && aligned4(bias) && aligned4(qs) && aligned4(emb_norm), "idb_fiqa_tail: unaligned pointer");
    IDB_REQUIRE(batch > 0 && batch <= (1 << 30) && d > 0 && d <= 8192, "idb_fiqa_tail: batch 1..2^30, d 1..8192");
    hipLaunchKernelGGL(fiqa_tail_kernel, dim3((batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, emb, weight, bias, batch, d, qs, emb_norm);
    IDB_CHECK_LAUNCH("idb_fiqa_tail");
    return IDB_OK;
}
