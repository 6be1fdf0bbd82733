// GroupNorm's input gradient over NHWC, with the SiLU that follows it in the resnets, the two-source channel concatenation of the up
// path, and an added tensor (the shortcut's or residual's gradient): what lorastage.py needs to carry a gradient through
// ResnetBlock2D and Transformer2DModel.norm.  f16 / bf16 operands, fp32 arithmetic, one rounding per result.
//
// Two launches in idb_groupnorm's two-pass geometry (channel slices of whole groups x up to 64 pixel chunks x batch), restated here
// because idb_norm.hip's own copy is pinned by its test matrix (the large-tensor 128-byte-line rule of the forward is left out: the
// plan query idb_groupnorm_bwd_plan says what is launched):
//   pass 1  gnb_sums_kernel    {sum g, sum g xhat} per (sample, pixel chunk, group) into the workspace, by fixed-order trees
//   pass 2  gnb_apply_kernel   merges the chunks in a fixed order in double, recomputes g, dx = rstd (g - m1 - xhat m2) (+ add)
// Both passes form mean and rstd from the forward's statistics partials with gn_apply_kernel's own expressions.  No atomics, no
// workgroup waits for another, every sum in an order the shape alone decides: repeats are bit-identical.  Loads are issued in batches
// from clamped addresses, as in idb_norm.hip.  A thread of pass 2 has read the elements it stores, so dx0 may be dy or add (c1 == 0).
#include "idb_common.h"
#include <math.h>

namespace {

constexpr int GNB_THREADS = 256;
constexpr int GNB_GSLOT = 4;         // groups one 8-channel vector can touch (at least 2 channels per group)
constexpr int GNB_MAXCHUNKS = 64;
constexpr int GNB_BATCH = 4;         // pixels a thread has in flight

struct GnbGeom {
    int C, C0, C1, HW, groups, cpg;
    int SW, cols, PR, nslices, gps, nchunks, chunk_len, ppb, apply_blocks;
};

inline int gnb_gcd(int a, int b) { return b ? gnb_gcd(b, a % b) : a; }

// idb_groupnorm's two-launch geometry below its large-tensor threshold: slices of lcm(cpg, 8) channels, doubled up to 8 vector
// columns; enough pixel chunks for ~1024 workgroups with at least two pixels per thread row; pass 2 in ~2048 pixel blocks.
inline GnbGeom gnb_geometry(int c0, int c1, int batch, int hw, int groups) {
    GnbGeom g;
    g.C0 = c0; g.C1 = c1; g.C = c0 + c1; g.HW = hw; g.groups = groups; g.cpg = g.C / groups;
    int sw = g.cpg / gnb_gcd(g.cpg, 8) * 8;
    while (sw / 8 < 8 && g.C % (sw * 2) == 0) sw *= 2;
    g.SW = sw; g.cols = sw / 8; g.PR = GNB_THREADS / g.cols; g.nslices = g.C / sw; g.gps = sw / g.cpg;
    const int pr2 = 2 * (g.PR > 0 ? g.PR : 1);                   // PR == 0 is refused by gnb_check_dims
    const int want = (1024 + batch * g.nslices - 1) / (batch * g.nslices);
    const int by_hw = (hw + pr2 - 1) / pr2;
    int n = want < by_hw ? want : by_hw;
    if (n < 1) n = 1;
    if (n > GNB_MAXCHUNKS) n = GNB_MAXCHUNKS;
    g.nchunks = n;
    g.chunk_len = (hw + n - 1) / n;
    const int want2 = (2048 + batch * g.nslices - 1) / (batch * g.nslices);
    g.ppb = (hw + want2 - 1) / want2;
    if (g.ppb < pr2) g.ppb = pr2;
    g.apply_blocks = (hw + g.ppb - 1) / g.ppb;
    return g;
}

template <typename T>
__device__ __forceinline__ typename Op<T>::v8 gnb_load_raw(const T* x0, const T* x1, const GnbGeom& g, long long pix, int c) {
    const T* src = c < g.C0 ? x0 + pix * g.C0 + c : x1 + pix * g.C1 + (c - g.C0);      // address select, no branch
    return *(const typename Op<T>::v8*)src;
}

// g = d gamma with d = dy, or dy SiLU'(y), y = xhat gamma + beta, SiLU'(y) = s (1 + y (1 - s)), s = 1 / (1 + exp(-y)): silu_f's
// v_exp_f32 / v_rcp_f32 pair
__device__ __forceinline__ float gnb_g(float dy, float xhat, float gamma, float beta, int silu) {
    float d = dy;
    if (silu) {
        const float y = xhat * gamma + beta;
        const float s = __builtin_amdgcn_rcpf(1.0f + __expf(-y));
        d = dy * (s * (1.0f + y * (1.0f - s)));
    }
    return d * gamma;
}

// mean and rstd of this slice's groups from the forward's partials, gn_apply_kernel's expressions: 8 lanes per group sum the chunks
// sub, sub + 8, ... in that order, a three-stage exchange, then mean, variance and rstd in double.  MERGE: the same lanes sum this
// backward's {sum g, sum g xhat} partials in double and leave m1 = sum g / n, m2 = sum g xhat / n.  All 256 threads call it.
template <bool MERGE>
__device__ __forceinline__ void gnb_group_terms(const GnbGeom& g, const float* stat, int stat_chunks, const float* sums, int slice, int b, float eps,
                                                float* gmean, float* grstd, float* gm1, float* gm2) {
    const int tid = threadIdx.x, gl = tid >> 3, sub = tid & 7;
    for (int g0 = 0; g0 < g.gps; g0 += GNB_THREADS / 8) {
        const int gi = g0 + gl;
        const int ga = slice * g.gps + min(gi, g.gps - 1);
        f32x2 pv[GNB_MAXCHUNKS / 8], sv[GNB_MAXCHUNKS / 8];
#pragma unroll
        for (int u = 0; u < GNB_MAXCHUNKS / 8; ++u) {
            const int ch = min(sub + 8 * u, stat_chunks - 1);
            pv[u] = *(const f32x2*)(stat + (((long long)b * stat_chunks + ch) * g.groups + ga) * 2);
            if (MERGE) {
                const int cw = min(sub + 8 * u, g.nchunks - 1);
                sv[u] = *(const f32x2*)(sums + (((long long)b * g.nchunks + cw) * g.groups + ga) * 2);
            }
        }
        float a = 0.f, q = 0.f;
        double sa = 0.0, sq = 0.0;
#pragma unroll
        for (int u = 0; u < GNB_MAXCHUNKS / 8; ++u) {
            if (gi < g.gps && sub + 8 * u < stat_chunks) {
                a += pv[u][0];
                q += pv[u][1];
            }
            if (MERGE && gi < g.gps && sub + 8 * u < g.nchunks) {
                sa += (double)sv[u][0];
                sq += (double)sv[u][1];
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            a += __shfl_xor(a, o, 64);
            q += __shfl_xor(q, o, 64);
            if (MERGE) {
                sa += __shfl_xor(sa, o, 64);
                sq += __shfl_xor(sq, o, 64);
            }
        }
        if (gi < g.gps && sub == 0) {
            const double cnt = (double)g.HW * g.cpg;
            const double mean = (double)a / cnt;
            double var = (double)q / cnt - mean * mean;
            if (var < 0.0) var = 0.0;
            gmean[gi] = (float)mean;
            grstd[gi] = (float)(1.0 / sqrt(var + (double)eps));
            if (MERGE) {
                gm1[gi] = (float)(sa / cnt);
                gm2[gi] = (float)(sq / cnt);
            }
        }
    }
}

// pass 1: {sum g, sum g xhat} per (sample, pixel chunk, group); grid = (pixel chunks, slices, batch)
template <typename T>
__global__ __launch_bounds__(GNB_THREADS) void gnb_sums_kernel(const T* x0, const T* x1, const T* dy, GnbGeom g, const float* stat, int stat_chunks,
                                                               const float* gamma, const float* beta, float eps, int silu, float* sums) {
    __shared__ float part[GNB_THREADS][GNB_GSLOT][2];
    __shared__ float gmean[64], grstd[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, slice = blockIdx.y, b = blockIdx.z;
    const int col = tid % g.cols, row = tid / g.cols;
    const int c = slice * g.SW + col * 8;                 // first channel of this thread's vector (inside the slice for every thread)
    const f32x4 ga0 = *(const f32x4*)(gamma + c), ga1 = *(const f32x4*)(gamma + c + 4);
    const f32x4 be0 = *(const f32x4*)(beta + c), be1 = *(const f32x4*)(beta + c + 4);
    gnb_group_terms<false>(g, stat, stat_chunks, nullptr, slice, b, eps, gmean, grstd, nullptr, nullptr);
    __syncthreads();
    float mu[8], rs[8], gm[8], bt[8], s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int gi = (c + e) / g.cpg - slice * g.gps;
        mu[e] = gmean[gi];
        rs[e] = grstd[gi];
        gm[e] = e < 4 ? ga0[e & 3] : ga1[e & 3];
        bt[e] = e < 4 ? be0[e & 3] : be1[e & 3];
        s1[e] = s2[e] = 0.f;
    }
    const int p0 = chunk * g.chunk_len, p1 = min(p0 + g.chunk_len, g.HW);
    if (row < g.PR) {
        for (int pb = p0 + row; pb < p1; pb += GNB_BATCH * g.PR) {
            typename Op<T>::v8 rx[GNB_BATCH], rd[GNB_BATCH];
#pragma unroll
            for (int u = 0; u < GNB_BATCH; ++u) {
                const long long pix = (long long)b * g.HW + min(pb + u * g.PR, p1 - 1);
                rx[u] = gnb_load_raw<T>(x0, x1, g, pix, c);
                rd[u] = *(const typename Op<T>::v8*)(dy + pix * g.C + c);
            }
#pragma unroll
            for (int u = 0; u < GNB_BATCH; ++u) {
                if (pb + u * g.PR < p1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float xh = (to_f32<T>(rx[u][e]) - mu[e]) * rs[e];
                        const float gg = gnb_g(to_f32<T>(rd[u][e]), xh, gm[e], bt[e], silu);
                        s1[e] += gg;
                        s2[e] += gg * xh;
                    }
                }
            }
        }
    }
    // fold the 8 channels into the (<= GNB_GSLOT) groups they belong to, then per group a lane-strided sum over the threads and a wave tree
    const int g_first = c / g.cpg;
    float gs[GNB_GSLOT], gq[GNB_GSLOT];
#pragma unroll
    for (int k = 0; k < GNB_GSLOT; ++k) gs[k] = gq[k] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = (c + e) / g.cpg - g_first;
#pragma unroll
        for (int kk = 0; kk < GNB_GSLOT; ++kk)
            if (kk == k) {
                gs[kk] += s1[e];
                gq[kk] += s2[e];
            }
    }
#pragma unroll
    for (int k = 0; k < GNB_GSLOT; ++k) {
        part[tid][k][0] = gs[k];
        part[tid][k][1] = gq[k];
    }
    __syncthreads();
    const int nact = g.cols * g.PR;
    const int slice_g0 = slice * g.gps;
    for (int gl = wave; gl < g.gps; gl += GNB_THREADS / 64) {
        const int ga = slice_g0 + gl;
        float a = 0.f, q = 0.f;
        for (int t = lane; t < nact; t += 64) {
            const int tc = slice * g.SW + (t % g.cols) * 8;
            const int k = ga - tc / g.cpg;
            if (k >= 0 && k < GNB_GSLOT) {
                a += part[t][k][0];
                q += part[t][k][1];
            }
        }
        a = wave_sum(a);
        q = wave_sum(q);
        if (lane == 0) {
            float* dst = sums + (((long long)b * g.nchunks + chunk) * g.groups + ga) * 2;
            dst[0] = a;
            dst[1] = q;
        }
    }
}

// pass 2: dx = rstd (g - m1 - xhat m2) (+ add); grid = (pixel blocks, slices, batch)
template <typename T, bool ADD>
__global__ __launch_bounds__(GNB_THREADS) void gnb_apply_kernel(const T* x0, const T* x1, const T* dy, const T* add, GnbGeom g, const float* stat,
                                                                int stat_chunks, const float* sums, const float* gamma, const float* beta, float eps,
                                                                int silu, T* dx0, T* dx1) {
    __shared__ float gmean[64], grstd[64], gm1[64], gm2[64];
    const int tid = threadIdx.x;
    const int slice = blockIdx.y, b = blockIdx.z;
    const int col = tid % g.cols, row = tid / g.cols;
    const int c = slice * g.SW + col * 8;
    const f32x4 ga0 = *(const f32x4*)(gamma + c), ga1 = *(const f32x4*)(gamma + c + 4);
    const f32x4 be0 = *(const f32x4*)(beta + c), be1 = *(const f32x4*)(beta + c + 4);
    gnb_group_terms<true>(g, stat, stat_chunks, sums, slice, b, eps, gmean, grstd, gm1, gm2);
    __syncthreads();
    if (row >= g.PR) return;
    float mu[8], rs[8], gm[8], bt[8], m1[8], m2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int gi = (c + e) / g.cpg - slice * g.gps;
        mu[e] = gmean[gi];
        rs[e] = grstd[gi];
        m1[e] = gm1[gi];
        m2[e] = gm2[gi];
        gm[e] = e < 4 ? ga0[e & 3] : ga1[e & 3];
        bt[e] = e < 4 ? be0[e & 3] : be1[e & 3];
    }
    const int p0 = blockIdx.x * g.ppb, p1 = min(p0 + g.ppb, g.HW);
    for (int pb = p0 + row; pb < p1; pb += GNB_BATCH * g.PR) {
        typename Op<T>::v8 rx[GNB_BATCH], rd[GNB_BATCH], ra[GNB_BATCH];
#pragma unroll
        for (int u = 0; u < GNB_BATCH; ++u) {
            const long long pix = (long long)b * g.HW + min(pb + u * g.PR, p1 - 1);
            rx[u] = gnb_load_raw<T>(x0, x1, g, pix, c);
            rd[u] = *(const typename Op<T>::v8*)(dy + pix * g.C + c);
            if (ADD) ra[u] = *(const typename Op<T>::v8*)(add + pix * g.C + c);
        }
#pragma unroll
        for (int u = 0; u < GNB_BATCH; ++u) {
            const int p = pb + u * g.PR;
            if (p < p1) {
                typename Op<T>::v8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xh = (to_f32<T>(rx[u][e]) - mu[e]) * rs[e];
                    const float gg = gnb_g(to_f32<T>(rd[u][e]), xh, gm[e], bt[e], silu);
                    float r = rs[e] * (gg - m1[e] - xh * m2[e]);
                    if (ADD) r += to_f32<T>(ra[u][e]);
                    o[e] = from_f32<T>(r);
                }
                const long long pix = (long long)b * g.HW + p;
                T* dst = c < g.C0 ? dx0 + pix * g.C0 + c : dx1 + pix * g.C1 + (c - g.C0);
                *(typename Op<T>::v8*)dst = o;
            }
        }
    }
}

// gn_check_dims' limits, restated
int gnb_check_dims(const char* api, int c0, int c1, int batch, int hw, int groups) {
    IDB_REQUIRE(batch > 0, "%s: batch must be positive", api);
    IDB_REQUIRE(hw > 0, "%s: hw must be positive", api);
    IDB_REQUIRE(groups > 0, "%s: groups must be positive", api);
    IDB_REQUIRE(c0 > 0 && c0 % 8 == 0, "%s: c0=%d must be a positive multiple of 8", api, c0);
    IDB_REQUIRE(c1 >= 0 && c1 % 8 == 0, "%s: c1=%d must be 0 or a positive multiple of 8", api, c1);
    IDB_REQUIRE((long long)c0 + c1 < (1 << 24), "%s: c0 + c1 too large", api);
    const int C = c0 + c1;
    IDB_REQUIRE(C % groups == 0, "%s: groups=%d does not divide the %d channels", api, groups, C);
    IDB_REQUIRE(C / groups >= 2, "%s: groups=%d leaves fewer than 2 channels per group", api, groups);
    IDB_REQUIRE((long long)batch * hw < (1LL << 31), "%s: batch * hw too large", api);
    const GnbGeom g = gnb_geometry(c0, c1, batch, hw, groups);
    IDB_REQUIRE(g.cols <= GNB_THREADS && g.gps <= 64 && batch <= 65535 && g.nslices <= 65535,
                "%s: unsupported geometry for %d channels in groups=%d (slice of %d channels, %d groups per slice)", api, C, groups, g.SW, g.gps);
    return IDB_OK;
}

template <typename T>
int gnb_run(const char* api, const void* x0, const void* x1, const float* stat, int stat_chunks, const void* dy, const void* add, const float* gamma,
            const float* beta, float eps, int silu, void* dx0, void* dx1, const GnbGeom& g, int batch, float* sums, hipStream_t st) {
    hipLaunchKernelGGL((gnb_sums_kernel<T>), dim3(g.nchunks, g.nslices, batch), dim3(GNB_THREADS), 0, st, (const T*)x0, (const T*)x1, (const T*)dy, g, stat,
                       stat_chunks, gamma, beta, eps, silu, sums);
    IDB_CHECK_LAUNCH("idb_groupnorm_bwd(sums)");
    if (add)
        hipLaunchKernelGGL((gnb_apply_kernel<T, true>), dim3(g.apply_blocks, g.nslices, batch), dim3(GNB_THREADS), 0, st, (const T*)x0, (const T*)x1,
                           (const T*)dy, (const T*)add, g, stat, stat_chunks, (const float*)sums, gamma, beta, eps, silu, (T*)dx0, (T*)dx1);
    else
        hipLaunchKernelGGL((gnb_apply_kernel<T, false>), dim3(g.apply_blocks, g.nslices, batch), dim3(GNB_THREADS), 0, st, (const T*)x0, (const T*)x1,
                           (const T*)dy, (const T*)nullptr, g, stat, stat_chunks, (const float*)sums, gamma, beta, eps, silu, (T*)dx0, (T*)dx1);
    IDB_CHECK_LAUNCH("idb_groupnorm_bwd(apply)");
    return IDB_OK;
}

}  // namespace

extern "C" size_t idb_groupnorm_bwd_workspace_bytes(int32_t batch, int32_t hw, int32_t groups) {
    if (batch <= 0 || hw <= 0 || groups <= 0) return 0;
    return (size_t)batch * GNB_MAXCHUNKS * groups * 2 * sizeof(float);
}

extern "C" int idb_groupnorm_bwd_plan(int32_t c0, int32_t c1, int32_t batch, int32_t hw, int32_t groups, int32_t* slice_channels, int32_t* slices,
                                      int32_t* chunks, int32_t* chunk_len, int32_t* apply_blocks) {
    const char* api = "idb_groupnorm_bwd_plan";
    IDB_REQUIRE(slice_channels && slices && chunks && chunk_len && apply_blocks, "%s: null output pointer", api);
    if (const int rc = gnb_check_dims(api, c0, c1, batch, hw, groups)) return rc;
    const GnbGeom g = gnb_geometry(c0, c1, batch, hw, groups);
    *slice_channels = g.SW;
    *slices = g.nslices;
    *chunks = g.nchunks;
    *chunk_len = g.chunk_len;
    *apply_blocks = g.apply_blocks;
    return IDB_OK;
}

extern "C" int idb_groupnorm_bwd(const void* x0, int32_t c0, const void* x1, int32_t c1, const float* stat_partials, int32_t stat_chunks, const void* dy,
                                 const void* add, const float* gamma, const float* beta, float eps, int32_t silu, void* dx0, void* dx1, int32_t batch,
                                 int32_t hw, int32_t groups, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
    const char* api = "idb_groupnorm_bwd";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be f16 or bf16", api);
        return IDB_EUNSUPPORTED;
    }
    const void* ptrs[] = {x0, stat_partials, dy, gamma, beta, dx0, workspace};
    const char* names[] = {"x0", "stat_partials", "dy", "gamma", "beta", "dx0", "workspace"};
    for (int i = 0; i < 7; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        IDB_REQUIRE(idb_aligned16(ptrs[i]), "%s: %s is not aligned (16 bytes)", api, names[i]);
    }
    IDB_REQUIRE(idb_aligned16(add), "%s: add is not aligned (16 bytes)", api);
    IDB_REQUIRE(idb_aligned16(x1), "%s: x1 is not aligned (16 bytes)", api);
    IDB_REQUIRE(idb_aligned16(dx1), "%s: dx1 is not aligned (16 bytes)", api);
    if (const int rc = gnb_check_dims(api, c0, c1, batch, hw, groups)) return rc;
    IDB_REQUIRE((c1 == 0) == (x1 == nullptr), "%s: x1 must be given exactly when c1 > 0", api);
    IDB_REQUIRE((c1 == 0) == (dx1 == nullptr), "%s: dx1 must be given exactly when c1 > 0", api);
    IDB_REQUIRE(stat_chunks >= 1 && stat_chunks <= GNB_MAXCHUNKS, "%s: stat_chunks=%d must be 1..%d", api, stat_chunks, GNB_MAXCHUNKS);
    IDB_REQUIRE(eps > 0.f && eps < INFINITY, "%s: eps must be positive and finite", api);
    IDB_REQUIRE(silu == 0 || silu == 1, "%s: silu must be 0 or 1", api);
    const size_t need = idb_groupnorm_bwd_workspace_bytes(batch, hw, groups);
    IDB_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes too small (%zu < %zu)", api, workspace_bytes, need);
    // dx0 may be dy or add themselves when there is one source; every other overlap of an output with an input or the other output
    // would be read after another thread's store
    const size_t pixels = (size_t)batch * hw, b0 = pixels * c0 * 2, b1 = pixels * c1 * 2, bc = b0 + b1;
    auto overlaps = [](const void* a, size_t na, const void* b, size_t nb) {
        return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    const void* outs[] = {dx0, dx1};
    const size_t out_bytes[] = {b0, b1};
    const char* out_names[] = {"dx0", "dx1"};
    for (int i = 0; i < 2; ++i) {
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], x0, b0), "%s: %s aliases x0", api, out_names[i]);
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], x1, b1), "%s: %s aliases x1", api, out_names[i]);
        const bool whole = i == 0 && c1 == 0;
        IDB_REQUIRE((whole && dx0 == dy) || !overlaps(outs[i], out_bytes[i], dy, bc), "%s: %s aliases dy (dx0 may be dy itself when c1 == 0)", api, out_names[i]);
        IDB_REQUIRE((whole && dx0 == add) || !overlaps(outs[i], out_bytes[i], add, bc), "%s: %s aliases add (dx0 may be add itself when c1 == 0)", api,
                    out_names[i]);
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], gamma, (size_t)(c0 + c1) * 4), "%s: %s aliases gamma", api, out_names[i]);
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], beta, (size_t)(c0 + c1) * 4), "%s: %s aliases beta", api, out_names[i]);
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], workspace, need), "%s: %s aliases workspace", api, out_names[i]);
        IDB_REQUIRE(!overlaps(outs[i], out_bytes[i], stat_partials, (size_t)batch * stat_chunks * groups * 8), "%s: %s aliases stat_partials", api,
                    out_names[i]);
    }
    IDB_REQUIRE(!overlaps(dx0, b0, dx1, b1), "%s: dx0 aliases dx1", api);
    const GnbGeom g = gnb_geometry(c0, c1, batch, hw, groups);
    hipStream_t st = (hipStream_t)stream;
    return dtype == IDB_BF16 ? gnb_run<__bf16>(api, x0, x1, stat_partials, stat_chunks, dy, add, gamma, beta, eps, silu, dx0, dx1, g, batch, (float*)workspace, st)
                             : gnb_run<_Float16>(api, x0, x1, stat_partials, stat_chunks, dy, add, gamma, beta, eps, silu, dx0, dx1, g, batch, (float*)workspace,
                                                 st);
}
