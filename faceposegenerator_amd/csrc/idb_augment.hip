// The FR-training input stage of the reference (FR_training/utils/augmentation.py: RandomHorizontalFlip -> RandAugment -> ToTensor ->
// Normalize(0.5, 0.5); FR_training/utils/rand_augment.py:_apply_op on PIL images) for a whole uint8 batch in one launch.
// faceposegenerator_amd/augment.py draws the plan and turns (op, bin, sign) into the per-slot arguments; every op below is Pillow's
// arithmetic restated (tests/randaug_oracle.py holds the same restatement in numpy, proven equal to Pillow on the CPU).
//
// One workgroup of 1024 threads per image.  The image lives in LDS for the whole chain: two ping-pong buffers of h*w*3 bytes, three
// 256-bin histograms, three 256-entry byte LUTs and the 256 values of the final normalisation; only `in` is read from global memory
// and only the requested outputs are written.  The op id of a slot is the same for the whole workgroup (read through
// readfirstlane): a scalar branch per slot.  Histogram, min / max and sums are integer LDS atomics and the prefix sum is a fixed
// shuffle tree, so results are bit-identical from run to run.  Geometry is 16.16 fixed point; the float ops are single multiplies,
// adds and divisions with contraction off (Pillow's x86-64 build has no FMA).  No per-lane arrays: nothing can land in scratch.
#include "idb_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RA_THREADS = 1024;
constexpr int RA_MAX_BYTES = 49152;                               // one image; 128 x 128 x 3
constexpr int RA_TAIL_BYTES = 768 * 4 + 768 + 256 * 4 + 32 * 4;    // hist, lut, the normalisation table, scalars
constexpr int RA_MAX_LDS = 2 * RA_MAX_BYTES + RA_TAIL_BYTES;

enum { OP_IDENTITY = 0, OP_SHEARX, OP_TRANSLATEX, OP_ROTATE, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_POSTERIZE,
       OP_SOLARIZE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_GRAYSCALE };
// scal[]: 0 the luma sum; 1..3 lowest and 4..6 highest non-empty bin per channel; 7..9 non-empty bins per channel; 10..21 the
// histogram totals of the 12 waves that scan it
enum { S_SUM = 0, S_LO = 1, S_HI = 4, S_NZ = 7, S_WAVE = 10 };

struct RandAugParams {
    const uint8_t* in;
    int h, w;
    const uint8_t* flip;
    const int* slot_op;
    const int* slot_iarg;
    const float* slot_farg;
    int num_ops;
    uint8_t* out_u8;
    float* out_f32;
};

// Pillow's L24: ITU-R 601-2 luma on a 16-bit scale, rounded
__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, f): float32, one rounding per operation; truncated for 0 <= f <= 1 (the result then lies between the
// two operands), clipped to [0, 255] first otherwise
__device__ __forceinline__ uint8_t blend(float deg, float img, float f, bool inside) {
    float t = deg + f * (img - deg);
    if (!inside) t = fminf(fmaxf(t, 0.0f), 255.0f);
    return (uint8_t)(int)t;
}

// one tap row of ImageFilter.SMOOTH
__device__ __forceinline__ float smooth_row(float acc, const uint8_t* r, float k0, float k1, float k2) {
    acc = acc + (float)r[-3] * k0;
    acc = acc + (float)r[0] * k1;
    acc = acc + (float)r[3] * k2;
    return acc;
}

__global__ __launch_bounds__(RA_THREADS) void randaug_kernel(RandAugParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, img = blockIdx.x;
    const int h = p.h, w = p.w, npix = h * w, nbytes = npix * 3, stride = (nbytes + 15) & ~15;
    uint8_t* cur = smem;
    uint8_t* nxt = smem + stride;
    uint32_t* hist = (uint32_t*)(smem + 2 * stride);             // [3][256]
    uint8_t* lut = (uint8_t*)(hist + 768);                       // [3][256]
    float* norm = (float*)(lut + 768);                           // [256]
    uint32_t* scal = (uint32_t*)(norm + 256);                    // [32]

    // ---- load (with the flip) ------------------------------------------------------------------------------------------------
    const uint8_t* src = p.in + (size_t)img * nbytes;
    if (p.flip != nullptr && p.flip[img] != 0) {
        for (int i = tid; i < npix; i += RA_THREADS) {
            const int y = i / w, x = i - y * w;
            const uint8_t* s = src + (size_t)(y * w + (w - 1 - x)) * 3;
            cur[i * 3 + 0] = s[0];
            cur[i * 3 + 1] = s[1];
            cur[i * 3 + 2] = s[2];
        }
    } else if ((((uintptr_t)src) & 3) == 0 && (nbytes & 3) == 0) {
        for (int i = tid; i < (nbytes >> 2); i += RA_THREADS) ((uint32_t*)cur)[i] = ((const uint32_t*)src)[i];
    } else {
        for (int i = tid; i < nbytes; i += RA_THREADS) cur[i] = src[i];
    }
    // ToTensor + Normalize of the 256 byte values: x / 255, - 0.5, / 0.5, each rounded once
    if (tid < 256) norm[tid] = (((float)tid / 255.0f) - 0.5f) / 0.5f;
    __syncthreads();

    // ---- the chain -----------------------------------------------------------------------------------------------------------
    for (int s = 0; s < p.num_ops; ++s) {
        const size_t slot = (size_t)img * p.num_ops + s;
        const int op = __builtin_amdgcn_readfirstlane(p.slot_op[slot]);
        const int* ia = p.slot_iarg + slot * 6;
        const float f = p.slot_farg[slot];
        const bool inside = f >= 0.0f && f <= 1.0f;
        if (op == OP_SHEARX || op == OP_TRANSLATEX || op == OP_ROTATE) {
            // Pillow's affine_fixed, nearest: the source of (x, y) is ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x) >> 16), black outside.
            // Unsigned products wrap instead of overflowing; the range check below is what keeps the read inside the image.
            const uint32_t a0 = ia[0], a1 = ia[1], a2 = ia[2], a3 = ia[3], a4 = ia[4], a5 = ia[5];
            for (int i = tid; i < npix; i += RA_THREADS) {
                const int y = i / w, x = i - y * w;
                const int xi = (int)(a2 + a1 * (uint32_t)y + a0 * (uint32_t)x) >> 16;
                const int yi = (int)(a5 + a4 * (uint32_t)y + a3 * (uint32_t)x) >> 16;
                uint8_t r = 0, g = 0, b = 0;
                if (xi >= 0 && xi < w && yi >= 0 && yi < h) {
                    const uint8_t* q = cur + (yi * w + xi) * 3;
                    r = q[0], g = q[1], b = q[2];
                }
                nxt[i * 3 + 0] = r;
                nxt[i * 3 + 1] = g;
                nxt[i * 3 + 2] = b;
            }
        } else if (op == OP_BRIGHTNESS) {
            for (int i = tid; i < nbytes; i += RA_THREADS) nxt[i] = blend(0.0f, (float)cur[i], f, inside);
        } else if (op == OP_COLOR || op == OP_GRAYSCALE) {
            for (int i = tid; i < npix; i += RA_THREADS) {
                const int r = cur[i * 3], g = cur[i * 3 + 1], b = cur[i * 3 + 2], l = luma(r, g, b);
                if (op == OP_GRAYSCALE) {
                    nxt[i * 3] = nxt[i * 3 + 1] = nxt[i * 3 + 2] = (uint8_t)l;
                } else {
                    nxt[i * 3 + 0] = blend((float)l, (float)r, f, inside);
                    nxt[i * 3 + 1] = blend((float)l, (float)g, f, inside);
                    nxt[i * 3 + 2] = blend((float)l, (float)b, f, inside);
                }
            }
        } else if (op == OP_CONTRAST) {
            // degenerate = the constant int(mean(L) + 0.5) = (2 sum + count) / (2 count) in integers
            if (tid == 0) scal[S_SUM] = 0;
            __syncthreads();
            uint32_t part = 0;
            for (int i = tid; i < npix; i += RA_THREADS) part += luma(cur[i * 3], cur[i * 3 + 1], cur[i * 3 + 2]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if ((tid & 63) == 0) atomicAdd(&scal[S_SUM], part);
            __syncthreads();
            const float mean = (float)((2u * scal[S_SUM] + (uint32_t)npix) / (2u * (uint32_t)npix));
            for (int i = tid; i < nbytes; i += RA_THREADS) nxt[i] = blend(mean, (float)cur[i], f, inside);
        } else if (op == OP_SHARPNESS) {
            // degenerate = ImageFilter.SMOOTH: [1 1 1; 1 5 1; 1 1 1] / 13 in float32, taps accumulated in row-major order from 0.5,
            // clipped and truncated; the one-pixel border is the input
            const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
            for (int i = tid; i < npix; i += RA_THREADS) {
                const int y = i / w, x = i - y * w;
                const bool interior = x > 0 && x < w - 1 && y > 0 && y < h - 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* q = cur + i * 3 + c;
                    float deg = (float)q[0];
                    if (interior) {
                        float acc = 0.5f;
                        acc = smooth_row(acc, q - w * 3, k1, k1, k1);
                        acc = smooth_row(acc, q, k1, k5, k1);
                        acc = smooth_row(acc, q + w * 3, k1, k1, k1);
                        deg = (float)(int)fminf(fmaxf(acc, 0.0f), 255.0f);
                    }
                    nxt[i * 3 + c] = blend(deg, (float)q[0], f, inside);
                }
            }
        } else if (op == OP_POSTERIZE) {
            const uint8_t mask = (uint8_t)ia[0];
            for (int i = tid; i < nbytes; i += RA_THREADS) nxt[i] = cur[i] & mask;
        } else if (op == OP_SOLARIZE) {
            for (int i = tid; i < nbytes; i += RA_THREADS) {
                const uint8_t v = cur[i];
                nxt[i] = (float)v < f ? v : (uint8_t)(255 - v);
            }
        } else if (op == OP_AUTOCONTRAST || op == OP_EQUALIZE) {
            if (tid < 768) hist[tid] = 0;
            if (tid < 32) scal[tid] = (tid >= S_LO && tid < S_LO + 3) ? 255u : 0u;
            __syncthreads();
            for (int i = tid; i < npix; i += RA_THREADS) {
                atomicAdd(&hist[cur[i * 3]], 1u);
                atomicAdd(&hist[256 + cur[i * 3 + 1]], 1u);
                atomicAdd(&hist[512 + cur[i * 3 + 2]], 1u);
            }
            __syncthreads();
            const int c = tid >> 8, bin = tid & 255;
            uint32_t hv = 0, below = 0;                          // this bin's count; the count of all lower bins of the channel
            if (tid < 768) {
                hv = hist[tid];
                if (hv != 0) {
                    atomicMin(&scal[S_LO + c], (uint32_t)bin);
                    atomicMax(&scal[S_HI + c], (uint32_t)bin);
                    atomicAdd(&scal[S_NZ + c], 1u);
                }
                uint32_t incl = hv;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, 64);
                    if ((tid & 63) >= o) incl += up;
                }
                if ((tid & 63) == 63) scal[S_WAVE + (tid >> 6)] = incl;
                below = incl - hv;
            }
            __syncthreads();
            if (tid < 768) {
                const int lo = (int)scal[S_LO + c], hi = (int)scal[S_HI + c];
                int v = bin;
                if (op == OP_AUTOCONTRAST) {
                    // ImageOps.autocontrast: lut[i] = clip(int(i scale + offset)) in double, identity for a flat channel
                    if (hi > lo) {
                        const double scale = 255.0 / (double)(hi - lo), off = -(double)lo * scale;
                        const double t = (double)bin * scale + off;
                        v = t <= 0.0 ? 0 : t >= 255.0 ? 255 : (int)t;
                    }
                } else {
                    // ImageOps.equalize: step = (sum - last non-empty bin) / 255; lut[i] = (step / 2 + sum of the lower bins) / step
                    const int wv = tid >> 6;
                    for (int k = wv & ~3; k < wv; ++k) below += scal[S_WAVE + k];
                    const uint32_t step = ((uint32_t)npix - hist[c * 256 + hi]) / 255u;
                    if (scal[S_NZ + c] > 1u && step != 0u) v = (int)min(255u, (step / 2u + below) / step);
                }
                lut[tid] = (uint8_t)v;
            }
            __syncthreads();
            for (int i = tid; i < npix; i += RA_THREADS) {
                nxt[i * 3 + 0] = lut[cur[i * 3]];
                nxt[i * 3 + 1] = lut[256 + cur[i * 3 + 1]];
                nxt[i * 3 + 2] = lut[512 + cur[i * 3 + 2]];
            }
        } else {
            continue;                                            // Identity (and any id outside the table): the image stays
        }
        uint8_t* t = cur;
        cur = nxt;
        nxt = t;
        __syncthreads();
    }

    // ---- outputs -------------------------------------------------------------------------------------------------------------
    if (p.out_u8 != nullptr) {
        uint8_t* dst = p.out_u8 + (size_t)img * nbytes;
        if ((((uintptr_t)dst) & 3) == 0 && (nbytes & 3) == 0) {
            for (int i = tid; i < (nbytes >> 2); i += RA_THREADS) ((uint32_t*)dst)[i] = ((const uint32_t*)cur)[i];
        } else {
            for (int i = tid; i < nbytes; i += RA_THREADS) dst[i] = cur[i];
        }
    }
    if (p.out_f32 != nullptr) {
        float* dst = p.out_f32 + (size_t)img * nbytes;           // NCHW: three planes of npix
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int i = tid; i < npix; i += RA_THREADS) dst[c * npix + i] = norm[cur[i * 3 + c]];
    }
}

static inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

extern "C" int idb_randaug(const uint8_t* in, int32_t n, int32_t h, int32_t w, const uint8_t* flip, const int32_t* slot_op,
                           const int32_t* slot_iarg, const float* slot_farg, int32_t num_ops, uint8_t* out_u8, float* out_f32_nchw,
                           void* stream) {
    IDB_REQUIRE(in != nullptr, "idb_randaug: null input");
    IDB_REQUIRE(out_u8 != nullptr || out_f32_nchw != nullptr, "idb_randaug: no output requested (out_u8 and out_f32_nchw are both null)");
    IDB_REQUIRE(n >= 1, "idb_randaug: n must be >= 1, got %d", n);
    IDB_REQUIRE(h >= 8 && w >= 8, "idb_randaug: h and w must be >= 8, got %d x %d", h, w);
    IDB_REQUIRE(num_ops >= 0 && (int64_t)n * num_ops * 6 < (1ll << 31), "idb_randaug: num_ops must be >= 0 and n * num_ops * 6 < 2^31, got %d", num_ops);
    IDB_REQUIRE(num_ops == 0 || (slot_op && slot_iarg && slot_farg), "idb_randaug: null slot arguments with num_ops = %d", num_ops);
    IDB_REQUIRE(aligned4(slot_op) && aligned4(slot_iarg) && aligned4(slot_farg) && aligned4(out_f32_nchw),
                "idb_randaug: the slot arguments and out_f32_nchw must be 4-byte aligned");
    if ((int64_t)h * w * 3 > RA_MAX_BYTES) {
        idb_set_error("idb_randaug: %d x %d images are not supported: h * w * 3 must be <= %d bytes (128 x 128), the image stays in LDS", h,
                      w, RA_MAX_BYTES);
        return IDB_EUNSUPPORTED;
    }
    RandAugParams p;
    p.in = in, p.h = h, p.w = w, p.flip = flip, p.slot_op = slot_op, p.slot_iarg = slot_iarg, p.slot_farg = slot_farg;
    p.num_ops = num_ops, p.out_u8 = out_u8, p.out_f32 = out_f32_nchw;
    const int stride = (h * w * 3 + 15) & ~15;
    return idb_launch<randaug_kernel>("idb_randaug", "randaug_kernel", dim3((unsigned)n), dim3(RA_THREADS), (size_t)(2 * stride + RA_TAIL_BYTES),
                                      RA_MAX_LDS, (hipStream_t)stream, p);
}
