// Identity-verification statistics over ArcFace embeddings (ID-Booth's Evaluation/PyEER_analysis): the cosine score of a list of
// row pairs, and pyeer's ROC quantities from the two sorted score sets.  Everything is double: the scores are compared against
// scipy / numpy to the last bits, and the ROC points are selected by exact comparisons of IEEE quotients.
//
// The ROC never builds pyeer's merged (score, label) array.  With G and I ascending, the thresholds are the run heads of G plus the
// run heads of I whose value is not in G, and for a threshold t
//     fnm(t) = #{genuine < t} = lower_bound(G, t)         fm(t) = #{impostor >= t} = ni - lower_bound(I, t).
// Every selected point is the minimum of a (key, threshold) pair under a total order (thresholds are distinct), so the reductions
// give the same bits in any order; the only float sums (the score moments) run in a fixed order over a grid that depends on
// (ng, ni) alone.  No atomics at all: per-block partials go to a slab in the workspace and one block finishes.
#include "idb_common.h"
#include <math.h>

// numpy rounds every product and sum on its own: no fused multiply-add where a product is inexact (the Matthews numerator)
#pragma clang fp contract(off)

namespace {

constexpr int VERIF_MAX_N = 1 << 30;
constexpr int VERIF_MAX_BLOCKS = 1024;
constexpr int VP = IDB_VERIF_POINTS;
constexpr int SLAB_WORDS = 2 * VP + 5;          // keys, thresholds, auc, thresholds counted, of them diff <= 0, sum(G), sum(I)
constexpr int DEV_WORDS = 2;                    // sum (g - gmean)^2, sum (i - imean)^2

// ---- scores ------------------------------------------------------------------------------------------------------------------------
// 16 lanes per pair, 4 pairs per wave: a 512-d row is 8 dwordx4 loads per lane, the gather hits L2 / Infinity Cache (a data set's
// embeddings are a few MB).  uv, uu and vv take the same elements in the same order, so identical rows give uv == uu == vv exactly.
constexpr int COS_LANES = 16;
constexpr int COS_PAIRS_PER_BLOCK = 256 / COS_LANES;

template <bool VEC>
__global__ __launch_bounds__(256) void verif_cos_kernel(const float* __restrict__ a, int na, const float* __restrict__ b, int nb, int d,
                                                        const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int n_pairs,
                                                        double* __restrict__ out) {
    const int sub = threadIdx.x & (COS_LANES - 1);
    const int grp = threadIdx.x / COS_LANES;
    for (int64_t base = (int64_t)blockIdx.x * COS_PAIRS_PER_BLOCK; base < n_pairs; base += (int64_t)gridDim.x * COS_PAIRS_PER_BLOCK) {
        const int64_t pair = base + grp;
        const bool live = pair < n_pairs;
        const int ra = live ? idx_a[pair] : 0, rb = live ? idx_b[pair] : 0;
        const bool in_range = ra >= 0 && ra < na && rb >= 0 && rb < nb;       // an index out of range reads nothing and gives NaN
        const float* pa = a + (size_t)(in_range ? ra : 0) * d;
        const float* pb = b + (size_t)(in_range ? rb : 0) * d;
        double uv, uu, vv;
        if (VEC) {
            double suv[4] = {0, 0, 0, 0}, suu[4] = {0, 0, 0, 0}, svv[4] = {0, 0, 0, 0};
            const f32x4* va = reinterpret_cast<const f32x4*>(pa);
            const f32x4* vb = reinterpret_cast<const f32x4*>(pb);
            for (int k = sub; k < d / 4; k += COS_LANES) {
                const f32x4 x = va[k], y = vb[k];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double u = (double)x[c], v = (double)y[c];
                    suv[c] += u * v;
                    suu[c] += u * u;
                    svv[c] += v * v;
                }
            }
            uv = (suv[0] + suv[1]) + (suv[2] + suv[3]);
            uu = (suu[0] + suu[1]) + (suu[2] + suu[3]);
            vv = (svv[0] + svv[1]) + (svv[2] + svv[3]);
        } else {
            uv = uu = vv = 0;
            for (int k = sub; k < d; k += COS_LANES) {
                const double u = (double)pa[k], v = (double)pb[k];
                uv += u * v;
                uu += u * u;
                vv += v * v;
            }
        }
#pragma unroll
        for (int o = COS_LANES / 2; o > 0; o >>= 1) {
            uv += __shfl_xor(uv, o, COS_LANES);
            uu += __shfl_xor(uu, o, COS_LANES);
            vv += __shfl_xor(vv, o, COS_LANES);
        }
        if (live && sub == 0) {
            // scipy: dist = 1 - uv / sqrt(uu vv), clipped to [0, 2] (a NaN stays one); the reference returns 1 - dist
            const double dist = 1.0 - uv / sqrt(uu * vv);
            const double clipped = dist < 0.0 ? 0.0 : (dist > 2.0 ? 2.0 : dist);
            out[pair] = in_range ? 1.0 - clipped : __builtin_nan("");
        }
    }
}

// ---- ROC ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int verif_lower_bound(const double* __restrict__ x, int n, double t) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// points whose ties go to the largest threshold (EER t1, the FNMR operating points); every other point takes the smallest
__host__ __device__ constexpr bool verif_takes_last(int p) { return p == IDB_VERIF_EER_T1 || (p >= IDB_VERIF_FNMR0 && p <= IDB_VERIF_FNMR1000); }

// (key, t) of a candidate replaces the best so far: smaller key, or the same finite key and the preferred threshold.  Selects, not
// branches: 13 of these per candidate and per shuffle step as control flow take the compiler more than half an hour
__device__ __forceinline__ void verif_take(int p, double key, double t, double& bk, double& bt) {
    const bool tie = (key == bk) & (key < INFINITY) & (verif_takes_last(p) ? t > bt : t < bt);
    const bool win = (key < bk) | tie;
    bk = win ? key : bk;
    bt = win ? t : bt;
}

// fixed-order block sum: xor butterfly in the wave, then the four wave totals in order; every thread gets the total
__device__ __forceinline__ double verif_block_sum(double v, double* lds4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// the sum of word `w` of every block's slab, in a fixed order: thread i takes blocks i, i + 256, ... and the block sums the threads
__device__ __forceinline__ double verif_slab_sum(const double* slab, int stride, int w, int blocks, double* lds4) {
    double s = 0;
    for (int j = threadIdx.x; j < blocks; j += 256) s += slab[(size_t)j * stride + w];
    return verif_block_sum(s, lds4);
}

__global__ __launch_bounds__(256) void verif_roc_partial_kernel(const double* __restrict__ g, int ng, const double* __restrict__ im, int ni,
                                                                double* __restrict__ slab) {
    __shared__ double s_key[4][VP], s_t[4][VP], s_sum[4][2];
    __shared__ unsigned long long s_int[4][3];
    double bk[VP], bt[VP];
#pragma unroll
    for (int p = 0; p < VP; ++p) {
        bk[p] = INFINITY;
        bt[p] = 0;
    }
    unsigned long long auc = 0, count = 0, count_le0 = 0;
    double gsum = 0, isum = 0;
    const int64_t total = (int64_t)ng + ni;
    const double dng = (double)ng, dni = (double)ni;
    for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < total; pos += (int64_t)gridDim.x * 256) {
        const bool from_g = pos < ng;
        const double* own = from_g ? g : im;
        const int k = from_g ? (int)pos : (int)(pos - ng);
        const double t = own[k];
        if (from_g) gsum += t; else isum += t;
        if (k > 0 && own[k - 1] == t) continue;                                   // not a run head
        int lg, li;
        if (from_g) {
            lg = k;
            li = verif_lower_bound(im, ni, t);
        } else {
            li = k;
            lg = verif_lower_bound(g, ng, t);
            if (lg < ng && g[lg] == t) continue;                                  // the run head of G stands for this value
        }
        const int fnm = lg, fm = ni - li;
        // the threshold before this one is the largest score below t in either set
        bool has_prev = false;
        double tp = 0;
        if (lg > 0) {
            tp = g[lg - 1];
            has_prev = true;
        }
        if (li > 0) {
            const double x = im[li - 1];
            if (!has_prev || x > tp) tp = x;
            has_prev = true;
        }
        if (has_prev) {
            const int fnm1 = verif_lower_bound(g, ng, tp), fm1 = ni - verif_lower_bound(im, ni, tp);
            auc += (unsigned long long)(fm1 - fm) * (unsigned long long)(2ll * ng - fnm1 - fnm);
        }
        const double dfm = (double)fm, dfnm = (double)fnm;
        const double fmr = dfm / dni, fnmr = dfnm / dng, diff = fmr - fnmr;
        count += 1;
        count_le0 += diff <= 0.0 ? 1 : 0;
        // pyeer's get_matthews_ccoef: separate square roots, a zero denominator replaced by 1
        const double tn = dni - dfm, tpos = dng - dfnm;
        const double numerator = tpos * tn - dfm * dfnm;
        const double den_a = sqrt(tpos + dfm) * sqrt(tpos + dfnm), den_b = sqrt(tn + dfm) * sqrt(tn + dfnm);
        double den = den_a * den_b;
        if (den == 0.0) den = 1.0;
        double key[VP];
        key[IDB_VERIF_EER_T2] = diff <= 0.0 ? 0.0 : INFINITY;
        key[IDB_VERIF_EER_T1] = diff > 0.0 ? 0.0 : INFINITY;
        key[IDB_VERIF_FMR0] = fabs(fmr - 0.0);
        key[IDB_VERIF_FMR1000] = fabs(fmr - 0.001);
        key[IDB_VERIF_FMR100] = fabs(fmr - 0.01);
        key[IDB_VERIF_FMR20] = fabs(fmr - 0.05);
        key[IDB_VERIF_FMR10] = fabs(fmr - 0.1);
        key[IDB_VERIF_FNMR0] = fabs(fnmr - 0.0);
        key[IDB_VERIF_FNMR100] = fabs(fnmr - 0.01);
        key[IDB_VERIF_FNMR1000] = fabs(fnmr - 0.001);
        key[IDB_VERIF_YOUDEN] = -((1.0 - fnmr) - fmr);
        key[IDB_VERIF_MCC] = -(numerator / den);
        key[IDB_VERIF_FIRST] = 0.0;
#pragma unroll
        for (int p = 0; p < VP; ++p) verif_take(p, key[p], t, bk[p], bt[p]);
    }
    // wave, then block
#pragma unroll 1
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int p = 0; p < VP; ++p) {
            const double ok = __shfl_xor(bk[p], o, 64), ot = __shfl_xor(bt[p], o, 64);
            verif_take(p, ok, ot, bk[p], bt[p]);
        }
        auc += __shfl_xor(auc, o, 64);
        count += __shfl_xor(count, o, 64);
        count_le0 += __shfl_xor(count_le0, o, 64);
        gsum += __shfl_xor(gsum, o, 64);
        isum += __shfl_xor(isum, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int p = 0; p < VP; ++p) {
            s_key[wave][p] = bk[p];
            s_t[wave][p] = bt[p];
        }
        s_int[wave][0] = auc;
        s_int[wave][1] = count;
        s_int[wave][2] = count_le0;
        s_sum[wave][0] = gsum;
        s_sum[wave][1] = isum;
    }
    __syncthreads();
    double* mine = slab + (size_t)blockIdx.x * SLAB_WORDS;
    const int p = threadIdx.x;
    if (p < VP) {
        double k0 = s_key[0][p], t0 = s_t[0][p];
        for (int w = 1; w < 4; ++w) verif_take(p, s_key[w][p], s_t[w][p], k0, t0);
        mine[p] = k0;
        mine[VP + p] = t0;
    } else if (p < VP + 3) {
        const int i = p - VP;
        reinterpret_cast<unsigned long long*>(mine)[2 * VP + i] = s_int[0][i] + s_int[1][i] + s_int[2][i] + s_int[3][i];
    } else if (p < VP + 5) {
        const int i = p - VP - 3;
        mine[2 * VP + 3 + i] = ((s_sum[0][i] + s_sum[1][i]) + s_sum[2][i]) + s_sum[3][i];
    }
}

// second pass of the moments: every block forms the two means from the slab (the same order everywhere, so the same bits), then its
// share of the squared deviations
__global__ __launch_bounds__(256) void verif_roc_dev_kernel(const double* __restrict__ g, int ng, const double* __restrict__ im, int ni,
                                                            const double* __restrict__ slab, double* __restrict__ dev) {
    __shared__ double lds4[4];
    const double gmean = verif_slab_sum(slab, SLAB_WORDS, 2 * VP + 3, gridDim.x, lds4) / (double)ng;
    const double imean = verif_slab_sum(slab, SLAB_WORDS, 2 * VP + 4, gridDim.x, lds4) / (double)ni;
    double gd = 0, id = 0;
    const int64_t total = (int64_t)ng + ni;
    for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < total; pos += (int64_t)gridDim.x * 256) {
        if (pos < ng) {
            const double x = g[pos] - gmean;
            gd += x * x;
        } else {
            const double x = im[pos - ng] - imean;
            id += x * x;
        }
    }
    gd = verif_block_sum(gd, lds4);
    id = verif_block_sum(id, lds4);
    if (threadIdx.x == 0) {
        dev[(size_t)blockIdx.x * DEV_WORDS] = gd;
        dev[(size_t)blockIdx.x * DEV_WORDS + 1] = id;
    }
}

__global__ __launch_bounds__(256) void verif_roc_final_kernel(const double* __restrict__ g, int ng, const double* __restrict__ im, int ni,
                                                              const double* __restrict__ slab, const double* __restrict__ dev, int blocks,
                                                              double* __restrict__ points, int64_t* __restrict__ ints,
                                                              double* __restrict__ moments) {
    __shared__ double lds4[4];
    __shared__ unsigned long long s_int[3][256];
    const int tid = threadIdx.x;
    if (tid < VP) {
        double bk = INFINITY, bt = 0;
        for (int j = 0; j < blocks; ++j) verif_take(tid, slab[(size_t)j * SLAB_WORDS + tid], slab[(size_t)j * SLAB_WORDS + VP + tid], bk, bt);
        const bool found = bk < INFINITY;
        points[tid] = found ? bt : __builtin_nan("");
        ints[2 * tid] = found ? (int64_t)ni - verif_lower_bound(im, ni, bt) : -1;
        ints[2 * tid + 1] = found ? (int64_t)verif_lower_bound(g, ng, bt) : -1;
    }
    for (int i = 0; i < 3; ++i) {
        unsigned long long s = 0;
        for (int j = tid; j < blocks; j += 256) s += reinterpret_cast<const unsigned long long*>(slab)[(size_t)j * SLAB_WORDS + 2 * VP + i];
        s_int[i][tid] = s;
    }
    __syncthreads();
    if (tid < 3) {
        unsigned long long s = 0;
        for (int j = 0; j < 256; ++j) s += s_int[tid][j];
        // thresholds, thresholds with fmr - fnmr <= 0, 2 ni ng AUC; stored in the order of the header
        ints[2 * VP + (tid == 0 ? 2 : tid - 1)] = (int64_t)s;
    }
    const double gmean = verif_slab_sum(slab, SLAB_WORDS, 2 * VP + 3, blocks, lds4) / (double)ng;
    const double imean = verif_slab_sum(slab, SLAB_WORDS, 2 * VP + 4, blocks, lds4) / (double)ni;
    const double gvar = verif_slab_sum(dev, DEV_WORDS, 0, blocks, lds4) / (double)ng;
    const double ivar = verif_slab_sum(dev, DEV_WORDS, 1, blocks, lds4) / (double)ni;
    if (tid == 0) {
        moments[0] = gmean;
        moments[1] = sqrt(gvar);
        moments[2] = imean;
        moments[3] = sqrt(ivar);
    }
}

inline int verif_blocks(int ng, int ni) {
    const int64_t want = ((int64_t)ng + ni + 255) / 256;
    return (int)(want < VERIF_MAX_BLOCKS ? want : VERIF_MAX_BLOCKS);
}
inline bool verif_counts_ok(int ng, int ni) { return ng >= 1 && ng <= VERIF_MAX_N && ni >= 1 && ni <= VERIF_MAX_N; }
inline size_t verif_ws_bytes(int ng, int ni) { return sizeof(double) * (size_t)verif_blocks(ng, ni) * (SLAB_WORDS + DEV_WORDS); }

}  // namespace

extern "C" int idb_verif_cos_scores(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const int32_t* idx_a, const int32_t* idx_b,
                                    int32_t n_pairs, double* out, void* stream) {
    IDB_REQUIRE(na >= 1 && nb >= 1 && d >= 1, "idb_verif_cos_scores: na, nb and d at least 1");
    IDB_REQUIRE(n_pairs >= 1 && n_pairs <= VERIF_MAX_N, "idb_verif_cos_scores: n_pairs in 1..2^30");
    IDB_REQUIRE(a && b && idx_a && idx_b && out, "idb_verif_cos_scores: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int want = (n_pairs + COS_PAIRS_PER_BLOCK - 1) / COS_PAIRS_PER_BLOCK;
    const int grid = want < 8192 ? want : 8192;
    if (d % 4 == 0 && idb_aligned16(a) && idb_aligned16(b))
        hipLaunchKernelGGL(verif_cos_kernel<true>, dim3(grid), dim3(256), 0, st, a, na, b, nb, d, idx_a, idx_b, n_pairs, out);
    else
        hipLaunchKernelGGL(verif_cos_kernel<false>, dim3(grid), dim3(256), 0, st, a, na, b, nb, d, idx_a, idx_b, n_pairs, out);
    IDB_CHECK_LAUNCH("idb_verif_cos_scores");
    return IDB_OK;
}

extern "C" size_t idb_verif_workspace_bytes(int32_t ng, int32_t ni) { return verif_counts_ok(ng, ni) ? verif_ws_bytes(ng, ni) : 0; }

extern "C" int idb_verif_roc(const double* g_sorted, int32_t ng, const double* i_sorted, int32_t ni, double* points, int64_t* ints,
                             double* moments, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(verif_counts_ok(ng, ni), "idb_verif_roc: ng and ni in 1..2^30");
    IDB_REQUIRE(g_sorted && i_sorted && points && ints && moments && ws, "idb_verif_roc: null pointer");
    IDB_REQUIRE(ws_bytes >= verif_ws_bytes(ng, ni) && idb_aligned16(ws), "idb_verif_roc: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = verif_blocks(ng, ni);
    double* slab = (double*)ws;
    double* dev = slab + (size_t)blocks * SLAB_WORDS;
    hipLaunchKernelGGL(verif_roc_partial_kernel, dim3(blocks), dim3(256), 0, st, g_sorted, ng, i_sorted, ni, slab);
    IDB_CHECK_LAUNCH("idb_verif_roc(partial)");
    hipLaunchKernelGGL(verif_roc_dev_kernel, dim3(blocks), dim3(256), 0, st, g_sorted, ng, i_sorted, ni, (const double*)slab, dev);
    IDB_CHECK_LAUNCH("idb_verif_roc(deviations)");
    hipLaunchKernelGGL(verif_roc_final_kernel, dim3(1), dim3(256), 0, st, g_sorted, ng, i_sorted, ni, (const double*)slab, (const double*)dev, blocks,
                       points, ints, moments);
    IDB_CHECK_LAUNCH("idb_verif_roc");
    return IDB_OK;
}
