// The LFW-style pair benchmark of a face-recognition backbone (ID-Booth's FR_training/utils/verification.py): the flip-fused,
// L2-normalised squared distance of every image pair, and the counts behind the 10-fold threshold search.  Everything is double.
//
// Distances: pair p is rows 2p and 2p + 1 of e0 (images) and e1 (their mirrors).  One pass forms the three row sums of each row
// (e0^2, e1^2, (e0 + e1)^2; the products and the sum e0 + e1 of fp32 operands are exact in double), a second pass reads the rows
// again (from L2) for the difference of the normalised rows: no row is held in registers.  Both rows of a pair take the same
// elements in the same order through the same code, so identical inputs give exactly 0.
//
// Counts: a pair with distance x counts for exactly the thresholds t with x < thresholds[t]; with non-decreasing thresholds those
// are the indices >= u, u = #{t : thresholds[t] <= x}, found by one binary search.  So a histogram over u per (fold, label), n_pairs
// integer atomics, and a prefix sum over t give counts[f][t][label] in O(n_pairs log n_thr + nfolds n_thr) instead of upstream's
// n_pairs x n_thr comparisons per fold and pass.  Integer sums do not depend on order; the only float sums (the row sums) run in an
// order fixed by d alone, so two runs give the same bits.
#include "idb_common.h"
#include <math.h>

// numpy rounds every product, quotient and sum on its own
#pragma clang fp contract(off)

namespace {

constexpr int FRB_MAX_PAIRS = 1 << 30;
constexpr int FRB_MAX_D = 8192;
constexpr int FRB_MAX_FOLDS = 64;
constexpr int FRB_MAX_THR = 16384;

// ---- distances ---------------------------------------------------------------------------------------------------------------------
// 16 lanes per pair, 16 pairs per block, the lane layout of verif_cos_kernel: a 512-d row is 8 dwordx4 loads per lane and matrix.
constexpr int FRB_LANES = 16;
constexpr int FRB_PAIRS_PER_BLOCK = 256 / FRB_LANES;

__device__ __forceinline__ double frb_lanes_sum(double v) {
#pragma unroll
    for (int o = FRB_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, FRB_LANES);
    return v;                                                // every lane of the group holds the same bits
}

// sum e0^2, sum e1^2 and sum (e0 + e1)^2 of one row: lane `sub` takes elements sub, sub + 16, ... (groups of four when VEC)
template <bool VEC>
__device__ __forceinline__ void frb_row_sums(const float* __restrict__ p0, const float* __restrict__ p1, int d, int sub, double& n0, double& n1,
                                             double& ns) {
    if (VEC) {
        double a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0}, as[4] = {0, 0, 0, 0};
        const f32x4* v0 = reinterpret_cast<const f32x4*>(p0);
        const f32x4* v1 = reinterpret_cast<const f32x4*>(p1);
        for (int k = sub; k < d / 4; k += FRB_LANES) {
            const f32x4 x = v0[k], y = v1[k];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double u = (double)x[c], v = (double)y[c], s = u + v;
                a0[c] += u * u;
                a1[c] += v * v;
                as[c] += s * s;
            }
        }
        n0 = (a0[0] + a0[1]) + (a0[2] + a0[3]);
        n1 = (a1[0] + a1[1]) + (a1[2] + a1[3]);
        ns = (as[0] + as[1]) + (as[2] + as[3]);
    } else {
        n0 = n1 = ns = 0;
        for (int k = sub; k < d; k += FRB_LANES) {
            const double u = (double)p0[k], v = (double)p1[k], s = u + v;
            n0 += u * u;
            n1 += v * v;
            ns += s * s;
        }
    }
    n0 = frb_lanes_sum(n0);
    n1 = frb_lanes_sum(n1);
    ns = frb_lanes_sum(ns);
}

template <bool VEC>
__global__ __launch_bounds__(256) void frb_pair_dist_kernel(const float* __restrict__ e0, const float* __restrict__ e1, int n_pairs, int d,
                                                            double* __restrict__ dist, double* __restrict__ norms) {
    const int sub = threadIdx.x & (FRB_LANES - 1);
    const int grp = threadIdx.x / FRB_LANES;
    const size_t rows = 2 * (size_t)n_pairs;
    for (int64_t base = (int64_t)blockIdx.x * FRB_PAIRS_PER_BLOCK; base < n_pairs; base += (int64_t)gridDim.x * FRB_PAIRS_PER_BLOCK) {
        const int64_t pair = base + grp;
        const bool live = pair < n_pairs;
        const size_t ra = live ? 2 * (size_t)pair : 0, rb = ra + 1;            // a dead group rereads pair 0 and stores nothing
        const float *a0 = e0 + ra * d, *a1 = e1 + ra * d, *b0 = e0 + rb * d, *b1 = e1 + rb * d;
        double na0, na1, nas, nb0, nb1, nbs;
        frb_row_sums<VEC>(a0, a1, d, sub, na0, na1, nas);
        frb_row_sums<VEC>(b0, b1, d, sub, nb0, nb1, nbs);
        // sklearn.preprocessing.normalize: x / ||x||, a zero norm replaced by 1
        double da = sqrt(nas), db = sqrt(nbs);
        da = da == 0.0 ? 1.0 : da;
        db = db == 0.0 ? 1.0 : db;
        double acc;
        if (VEC) {
            double s4[4] = {0, 0, 0, 0};
            const f32x4 *va0 = reinterpret_cast<const f32x4*>(a0), *va1 = reinterpret_cast<const f32x4*>(a1);
            const f32x4 *vb0 = reinterpret_cast<const f32x4*>(b0), *vb1 = reinterpret_cast<const f32x4*>(b1);
            for (int k = sub; k < d / 4; k += FRB_LANES) {
                const f32x4 xa = va0[k], ya = va1[k], xb = vb0[k], yb = vb1[k];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double fa = ((double)xa[c] + (double)ya[c]) / da, fb = ((double)xb[c] + (double)yb[c]) / db;
                    const double df = fa - fb;
                    s4[c] += df * df;
                }
            }
            acc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        } else {
            acc = 0;
            for (int k = sub; k < d; k += FRB_LANES) {
                const double fa = ((double)a0[k] + (double)a1[k]) / da, fb = ((double)b0[k] + (double)b1[k]) / db;
                const double df = fa - fb;
                acc += df * df;
            }
        }
        acc = frb_lanes_sum(acc);
        if (live && sub == 0) {
            dist[pair] = acc;
            norms[ra] = sqrt(na0);
            norms[rb] = sqrt(nb0);
            norms[rows + ra] = sqrt(na1);
            norms[rows + rb] = sqrt(nb1);
        }
    }
}

// ---- counts ------------------------------------------------------------------------------------------------------------------------
// hist [nfolds][2][n_thr + 1] in the workspace: bin u of (fold, label), label 0 = same, 1 = different; bin n_thr is "below no threshold"
__global__ __launch_bounds__(256) void frb_zero_kernel(int32_t* __restrict__ hist, int words) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) hist[i] = 0;
}

__global__ __launch_bounds__(256) void frb_hist_kernel(const double* __restrict__ dist, const uint8_t* __restrict__ issame, int n_pairs,
                                                       const int32_t* __restrict__ fold_start, int nfolds, const double* __restrict__ thr,
                                                       int n_thr, int32_t* __restrict__ hist) {
    __shared__ int32_t s_start[FRB_MAX_FOLDS + 1];
    if (threadIdx.x <= nfolds) s_start[threadIdx.x] = fold_start[threadIdx.x];
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * 256) {
        if (p < s_start[0] || p >= s_start[nfolds]) continue;                  // in no fold
        int lo = 0, hi = nfolds;                                               // the last f in [0, nfolds) with s_start[f] <= p
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (s_start[mid] <= p) lo = mid; else hi = mid;
        }
        const int f = lo;
        const double x = dist[p];
        int u = 0, end = n_thr;                                                // the first t with x < thr[t] (np.less; a NaN is below nothing)
        while (u < end) {
            const int mid = u + ((end - u) >> 1);
            if (x < thr[mid]) end = mid; else u = mid + 1;
        }
        const int label = issame[p] ? 0 : 1;
        atomicAdd(&hist[((size_t)f * 2 + label) * (n_thr + 1) + u], 1);
    }
}

// one block per (fold, label): counts[f][t][label] = sum of bins 0..t.  Thread i owns the contiguous bins [i c, (i + 1) c)
__global__ __launch_bounds__(256) void frb_scan_kernel(const int32_t* __restrict__ hist, int n_thr, int32_t* __restrict__ counts) {
    __shared__ int32_t s_tot[256];
    const int f = blockIdx.x >> 1, label = blockIdx.x & 1, tid = threadIdx.x;
    const int32_t* h = hist + (size_t)blockIdx.x * (n_thr + 1);
    const int chunk = (n_thr + 255) / 256;
    const int t0 = tid * chunk, t1 = min(t0 + chunk, n_thr);
    int32_t own = 0;
    for (int t = t0; t < t1; ++t) own += h[t];
    s_tot[tid] = own;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                                        // inclusive scan of the 256 totals
        const int32_t v = tid >= o ? s_tot[tid - o] : 0;
        __syncthreads();
        s_tot[tid] += v;
        __syncthreads();
    }
    int32_t run = s_tot[tid] - own;
    for (int t = t0; t < t1; ++t) {
        run += h[t];
        counts[((size_t)f * n_thr + t) * 2 + label] = run;
    }
}

inline bool frb_counts_ok(int n_pairs, int nfolds, int n_thr) {
    return n_pairs >= 1 && n_pairs <= FRB_MAX_PAIRS && nfolds >= 1 && nfolds <= FRB_MAX_FOLDS && nfolds <= n_pairs && n_thr >= 1 &&
           n_thr <= FRB_MAX_THR;
}
inline size_t frb_ws_bytes(int nfolds, int n_thr) { return (sizeof(int32_t) * (size_t)nfolds * 2 * (n_thr + 1) + 15) & ~(size_t)15; }

}  // namespace

extern "C" int idb_frb_pair_dist(const float* e0, const float* e1, int32_t n_pairs, int32_t d, double* dist, double* norms, void* stream) {
    IDB_REQUIRE(n_pairs >= 1 && n_pairs <= FRB_MAX_PAIRS, "idb_frb_pair_dist: n_pairs in 1..2^30");
    IDB_REQUIRE(d >= 1 && d <= FRB_MAX_D, "idb_frb_pair_dist: d in 1..8192");
    IDB_REQUIRE(e0 && e1 && dist && norms, "idb_frb_pair_dist: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int want = (n_pairs + FRB_PAIRS_PER_BLOCK - 1) / FRB_PAIRS_PER_BLOCK;
    const int grid = want < 8192 ? want : 8192;
    if (d % 4 == 0 && idb_aligned16(e0) && idb_aligned16(e1))
        hipLaunchKernelGGL(frb_pair_dist_kernel<true>, dim3(grid), dim3(256), 0, st, e0, e1, n_pairs, d, dist, norms);
    else
        hipLaunchKernelGGL(frb_pair_dist_kernel<false>, dim3(grid), dim3(256), 0, st, e0, e1, n_pairs, d, dist, norms);
    IDB_CHECK_LAUNCH("idb_frb_pair_dist");
    return IDB_OK;
}

extern "C" size_t idb_frb_workspace_bytes(int32_t n_pairs, int32_t nfolds, int32_t n_thr) {
    return frb_counts_ok(n_pairs, nfolds, n_thr) ? frb_ws_bytes(nfolds, n_thr) : 0;
}

extern "C" int idb_frb_fold_counts(const double* dist, const uint8_t* issame, int32_t n_pairs, const int32_t* fold_start, int32_t nfolds,
                                   const double* thresholds, int32_t n_thr, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(n_pairs >= 1 && n_pairs <= FRB_MAX_PAIRS, "idb_frb_fold_counts: n_pairs in 1..2^30");
    IDB_REQUIRE(nfolds >= 1 && nfolds <= FRB_MAX_FOLDS && nfolds <= n_pairs, "idb_frb_fold_counts: nfolds in 1..64 and at most n_pairs");
    IDB_REQUIRE(n_thr >= 1 && n_thr <= FRB_MAX_THR, "idb_frb_fold_counts: n_thr in 1..16384");
    IDB_REQUIRE(dist && issame && fold_start && thresholds && counts && ws, "idb_frb_fold_counts: null pointer");
    IDB_REQUIRE(ws_bytes >= frb_ws_bytes(nfolds, n_thr) && idb_aligned16(ws), "idb_frb_fold_counts: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* hist = (int32_t*)ws;
    const int words = nfolds * 2 * (n_thr + 1);
    hipLaunchKernelGGL(frb_zero_kernel, dim3((words + 255) / 256 < 1024 ? (words + 255) / 256 : 1024), dim3(256), 0, st, hist, words);
    IDB_CHECK_LAUNCH("idb_frb_fold_counts(zero)");
    const int want = (n_pairs + 255) / 256;
    hipLaunchKernelGGL(frb_hist_kernel, dim3(want < 1024 ? want : 1024), dim3(256), 0, st, dist, issame, n_pairs, fold_start, nfolds, thresholds,
                       n_thr, hist);
    IDB_CHECK_LAUNCH("idb_frb_fold_counts(histogram)");
    hipLaunchKernelGGL(frb_scan_kernel, dim3(2 * nfolds), dim3(256), 0, st, (const int32_t*)hist, n_thr, counts);
    IDB_CHECK_LAUNCH("idb_frb_fold_counts");
    return IDB_OK;
}
