// The loss head of the face-recognition training loop (ID-Booth's FR_training/utils/losses.py CosFace / ArcFace / AdaFace, then
// CrossEntropyLoss and multi_class_acc of train_FR.py): the [B, D] x [D, C] cosine product on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32), whose B x C result the loss path never writes.  The loss needs one log-sum-exp and one target logit per row,
// the accuracy one argmax per row.
//   pack   kernel [D][C] -> Wn [C][D], every column divided by its double norm (one rounding), and the double norms themselves
//   prep   one wave per embedding row: its norm, the normalised row (fp32, one rounding) and the target cosine
//          <e_i, kernel[:, label_i]> / (|e_i| |kernel[:, label_i]|) as a gathered dot product in double; the margin is applied to it in
//          double, so the one ill-conditioned entry of a row (acos near +-1) never goes through fp32
//   loss   the tile engine of idb_pair.hip with the operands swapped: a wave owns 32 embedding rows, so every lane owns ONE row and
//          meets 16 of each 32 classes of the tile.  Running maximum, sum of exp(z - max) and argmax stay in the lane's registers; the
//          two half-waves of a row are merged in a fixed order and one partial per (row, column block) goes to the workspace
//   merge  up to a wave of lanes per row take its column blocks in ascending order and meet in a fixed butterfly
//   mean   one block: the mean loss as a fixed-order double sum and the count of correct rows
//   logits the same tile loop with the operands the usual way round (a lane owns a class, stores are coalesced) and a store epilogue
//   grad   the backward (idb_head_loss_grad): the cosine tile is recomputed on the MFMA, G = (softmax - one-hot) s d mask / B is formed
//          in the accumulator registers from the forward's log-sum-exp, and the accumulator tile is the A operand of the second product
//          as it stands (its column is on the lane, its rows are the reduction index): dX = G Wn per (row tile, class block) with the
//          blocks merged in ascending order, dW = G^T X per class tile over all row tiles, projected and written as kernel.grad
//   sgd    clip_grad_norm_ and SGD with momentum on the kernel (idb_head_sgd_step): squared-sum partials, then the norm and the step in
//          one launch, both made of idb_sgd.h's device functions (the arithmetic of idb_sgd.hip), then pack
// No floating-point atomics, every sum in a fixed order that depends on the shapes alone: results are bit-identical from run to run.
#include "idb_sgd.h"
#include <math.h>

namespace {

constexpr int HB = 128;            // rows of the wave-owned operand per workgroup (4 waves x 32)
constexpr int HK = 32;             // K per LDS stage
constexpr int HLD = HK + 1;        // LDS row stride in floats (idb_pair.hip: 33 r mod 64 is injective over a half-wave)
constexpr int HEAD_MAX_B = 65536, HEAD_MAX_D = 4096, HEAD_MAX_C = 1 << 20;
constexpr int HEAD_FILL = 256;     // workgroups that fill the machine (CUs)
constexpr int HEAD_MAX_WGS = 2048; // column blocks x row tiles stays near this: bounds the workspace at the largest shapes
constexpr double ADA_EPS = 1e-3;

// Thread t stages columns 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i, i < T, of an operand: 8 lanes read 128 contiguous bytes of a row.
template <int T>
__device__ __forceinline__ void head_fetch(const float* const (&row)[T], int D, bool vec, int k0, f32x4 (&v)[T]) {
    const int k = k0 + (threadIdx.x & 7) * 4;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};                // rows past the end and columns past D are zero
        if (row[i]) {
            if (vec) {
                if (k < D) x = *(const f32x4*)(row[i] + k);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < D) x[e] = row[i][k + e];
            }
        }
        v[i] = x;
    }
}

template <int T>
__device__ __forceinline__ void head_stash(float* lds, const f32x4 (&v)[T]) {
    const int c = (threadIdx.x & 7) * 4, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[(r + 32 * i) * HLD + c + e] = v[i][e];
}

// acc[t] = rows m0 + 32 t .., t < TA, of a [na][D] times rows n0 + 32 wave .. of b [nb][D], over all of D.  vec: D % 4 == 0 and 16-byte
// aligned bases.  sA holds 32 TA rows, sB 128.  Ends with a barrier.
template <int TA>
__device__ __forceinline__ void head_tile(const float* a, int na, const float* b, int nb, int D, bool vec, int m0, int n0, float* sA, float* sB,
                                          f32x16 (&acc)[TA]) {
    const float* ra[TA];
    const float* rb[4];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
        const int r = (threadIdx.x >> 3) + 32 * i;
        ra[i] = m0 + r < na ? a + (long long)(m0 + r) * D : nullptr;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (threadIdx.x >> 3) + 32 * i;
        rb[i] = n0 + r < nb ? b + (long long)(n0 + r) * D : nullptr;
    }
#pragma unroll
    for (int t = 0; t < TA; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
    f32x4 va[TA], vb[4];
    head_fetch<TA>(ra, D, vec, 0, va);
    head_fetch<4>(rb, D, vec, 0, vb);
    for (int k0 = 0; k0 < D; k0 += HK) {
        __syncthreads();                               // the previous stage has been read
        head_stash<TA>(sA, va);
        head_stash<4>(sB, vb);
        __syncthreads();
        if (k0 + HK < D) {                             // the next stage's loads fly during this stage's MFMAs
            head_fetch<TA>(ra, D, vec, k0 + HK, va);
            head_fetch<4>(rb, D, vec, k0 + HK, vb);
        }
#pragma unroll
        for (int kk = 0; kk < HK; kk += 2) {           // A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
            const float bv = sB[(w * 32 + r) * HLD + kk + h];
#pragma unroll
            for (int t = 0; t < TA; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[(t * 32 + r) * HLD + kk + h], bv, acc[t], 0, 0, 0);
        }
    }
    __syncthreads();
}

// torch.clamp keeps a NaN; fminf / fmaxf would not
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- pack -------------------------------------------------------------------------------------------------------------------------
// One workgroup per 64 columns (classes).  Pass 1: thread (g = t >> 6, c = t & 63) sums kernel[k][c]^2 over k = g, g + 4, ... in double
// (reads coalesced along c), the four partial sums are added in order.  Pass 2: 32 x 64 blocks are divided, rounded once and written
// transposed through LDS (writes coalesced along k).
__global__ __launch_bounds__(256) void head_pack_kernel(const float* __restrict__ kernel, int D, int C, float* __restrict__ wn,
                                                        double* __restrict__ col_norm, int32_t* __restrict__ bad_cols) {
    __shared__ double part[4][64];
    __shared__ double nrm[64];
    __shared__ float tile[64][HLD];
    const int c0 = blockIdx.x * 64, c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool live = c0 + c < C;
    double s = 0.0;
    if (live)
        for (int k = g; k < D; k += 4) {
            const double v = (double)kernel[(long long)k * C + c0 + c];
            s += v * v;
        }
    part[g][c] = s;
    __syncthreads();
    if (g == 0) {
        const double n = sqrt(((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]);
        nrm[c] = n;
        if (live) {
            col_norm[c0 + c] = n;
            if (!(n > 0.0 && n < __builtin_inf())) atomicAdd(bad_cols, 1);      // an integer count: any order gives the same value
        }
    }
    __syncthreads();
    for (int k0 = 0; k0 < D; k0 += HK) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int kk = g + 4 * r;
            tile[c][kk] = live && k0 + kk < D ? (float)((double)kernel[(long long)(k0 + kk) * C + c0 + c] / nrm[c]) : 0.f;
        }
        __syncthreads();
        const int kx = threadIdx.x & 31, cy = threadIdx.x >> 5;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int cc = cy + 8 * r;
            if (c0 + cc < C && k0 + kx < D) wn[(long long)(c0 + cc) * D + k0 + kx] = tile[cc][kx];
        }
        __syncthreads();
    }
}

// ---- AdaFace batch statistics -----------------------------------------------------------------------------------------------------
// One workgroup: mean and unbiased standard deviation of clip(norms, 0.001, 100) (thread t takes rows t, t + 256, ... in order, then the
// fixed block sum), then the EMA update of state = {batch_mean, batch_std} in place.
__global__ __launch_bounds__(256) void head_ada_stats_kernel(const float* __restrict__ norms, int B, double t_alpha, double* __restrict__ state) {
    __shared__ double lds4[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) s += clampd((double)norms[i], 0.001, 100.0);
    const double mean = block_sum_d(s, lds4) / (double)B;
    double q = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const double d = clampd((double)norms[i], 0.001, 100.0) - mean;
        q += d * d;
    }
    const double std = sqrt(block_sum_d(q, lds4) / (double)(B - 1));
    if (threadIdx.x == 0 && mean - mean == 0.0) {          // a NaN norm leaves the buffers as they were (and gives its row a NaN target)
        state[0] = mean * t_alpha + (1.0 - t_alpha) * state[0];
        state[1] = std * t_alpha + (1.0 - t_alpha) * state[1];
    }
}

// ---- per-row prep -----------------------------------------------------------------------------------------------------------------
struct HeadMargin {
    int kind;
    double s, m, h;
};

// rows [0] lse, [1] loss, [2] target logit, [3] target cosine (before the clamp), [4] margin scaler (AdaFace, else 0); all [B] double.
// A label outside [0, C) reads nothing and gives a NaN target (the host refuses such labels where it can see them).
__global__ __launch_bounds__(256) void head_prep_kernel(const float* __restrict__ emb, const float* __restrict__ norms,
                                                        const int32_t* __restrict__ label, const float* __restrict__ kernel,
                                                        const double* __restrict__ col_norm, const double* __restrict__ ada_state, int B, int D,
                                                        int C, HeadMargin mg, float* __restrict__ en, float* __restrict__ zt32,
                                                        double* __restrict__ rows) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= B) return;
    const float* e = emb + (long long)i * D;
    const int lab = label[i];
    const bool ok = lab >= 0 && lab < C;
    const float* w = kernel + (ok ? lab : 0);
    double uu = 0.0, uw = 0.0;
    for (int k = l; k < D; k += 64) {
        const double x = (double)e[k];
        uu += x * x;
        uw += x * (double)w[(long long)k * C];
    }
    uu = wave_sum_d(uu);
    uw = wave_sum_d(uw);
    // AdaFace takes its embeddings as they are (upstream normalises them in the loop, not in the header)
    const double n = mg.kind == IDB_HEAD_ADAFACE ? 1.0 : sqrt(uu);
    if (mg.kind != IDB_HEAD_ADAFACE)
        for (int k = l; k < D; k += 64) en[(long long)i * D + k] = (float)((double)e[k] / n);
    if (l != 0) return;
    const double c = ok ? uw / (n * col_norm[lab]) : __builtin_nan("");
    double z, scaler = 0.0;
    if (mg.kind == IDB_HEAD_COSFACE) {
        z = clampd(c, -1.0, 1.0) - mg.m;
    } else if (mg.kind == IDB_HEAD_ARCFACE) {
        z = cos(acos(clampd(c, -1.0, 1.0)) + mg.m);
    } else {
        const double safe = clampd((double)norms[i], 0.001, 100.0);
        scaler = clampd((safe - ada_state[0]) / (ada_state[1] + ADA_EPS) * mg.h, -1.0, 1.0);
        const double theta = acos(clampd(c, -1.0 + ADA_EPS, 1.0 - ADA_EPS)) + mg.m * scaler * -1.0;
        z = cos(clampd(theta, ADA_EPS, M_PI - ADA_EPS)) - (mg.m + mg.m * scaler);
    }
    z = c - c == 0.0 ? z * mg.s : __builtin_nan("");   // a zero or non-finite row (0 / 0, inf / inf) marks its target: the caller refuses
    zt32[i] = (float)z;
    rows[2LL * B + i] = z;
    rows[3LL * B + i] = c;
    rows[4LL * B + i] = scaler;
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------
// grid (column blocks, row tiles).  Column block cb takes class tiles cb per .. of 32 TA classes.  ws_m / ws_s / ws_a [B][column blocks].
template <int TA>
__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ x, const float* __restrict__ wn, const int32_t* __restrict__ label,
                                                        const float* __restrict__ zt32, int B, int D, int C, int vec, float lo, float hi,
                                                        float s, int per, float* __restrict__ ws_m, double* __restrict__ ws_s,
                                                        int32_t* __restrict__ ws_a) {
    __shared__ float sA[32 * TA * HLD], sB[HB * HLD];
    const int n0 = blockIdx.y * HB, tiles = (C + 32 * TA - 1) / (32 * TA);
    const int t0 = blockIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    const int lab = j < B ? label[j] : -1;
    const float zt = j < B ? zt32[j] : 0.f;
    const float ninf = -__builtin_inff();
    float m = ninf;
    double S = 0.0;
    int arg = 0x7fffffff;
    for (int tile = t0; tile < t1; ++tile) {
        const int m0 = tile * 32 * TA;
        f32x16 acc[TA];
        head_tile<TA>(wn, C, x, B, D, vec != 0, m0, n0, sA, sB, acc);
        float mt = ninf;
        int at = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < TA; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = m0 + tile_row(t, e, h);
                float z = s * clampf(acc[t][e], lo, hi);
                z = i == lab ? zt : z;                 // the target column is replaced, not adjusted
                z = i < C ? z : ninf;
                acc[t][e] = z;
                const bool win = z > mt || (z == mt && i < at);
                mt = win ? z : mt;
                at = win ? i : at;
            }
        if (mt > m) {                                  // rescale in double: once per tile, so its error does not compound in fp32
            S = m > ninf ? S * exp((double)m - (double)mt) : 0.0;
            m = mt;
            arg = at;
        }                                              // mt == m keeps arg: a later tile's classes all have higher indices
#pragma unroll
        for (int t = 0; t < TA; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) S += acc[t][e] > ninf ? (double)expf(acc[t][e] - m) : 0.0;
    }
    // the two half-waves of a row: the lower half's term first
    const float mo = __shfl_xor(m, 32, 64);
    const double So = __shfl_xor(S, 32, 64);
    const int ao = __shfl_xor(arg, 32, 64);
    if (h == 0 && j < B) {
        const float M = mo > m ? mo : m;
        const double sum = (m > ninf ? S * exp((double)m - (double)M) : 0.0) + (mo > ninf ? So * exp((double)mo - (double)M) : 0.0);
        const bool other = mo > m || (mo == m && ao < arg);
        const long long o = (long long)j * gridDim.x + blockIdx.x;
        ws_m[o] = M;
        ws_s[o] = sum;
        ws_a[o] = other ? ao : arg;
    }
}

// G lanes (a power of two, chosen by the host from the number of column blocks) share a row,
// 1024 / G rows per workgroup: lane q takes blocks q, q + G, ... in ascending order (the partials of a row are contiguous), then the G
// partial results are merged by an xor butterfly, the lower lane's term first.  The order depends on (B, blocks) alone.
constexpr int MERGE_THREADS = 1024;

__global__ __launch_bounds__(MERGE_THREADS) void head_merge_kernel(const float* __restrict__ ws_m, const double* __restrict__ ws_s,
                                                                   const int32_t* __restrict__ ws_a, int blocks, int B, int G,
                                                                   double* __restrict__ rows, int32_t* __restrict__ pred) {
    const float ninf = -__builtin_inff();
    const int q = threadIdx.x & (G - 1), i = blockIdx.x * (MERGE_THREADS / G) + threadIdx.x / G;
    const bool live = i < B;
    const long long base = (long long)(live ? i : 0) * blocks;
    float M = ninf;
    int arg = 0x7fffffff;
    if (live)
        for (int b = q; b < blocks; b += G) {
            const float mb = ws_m[base + b];
            const int ab = ws_a[base + b];
            const bool win = mb > M || (mb == M && ab < arg);
            M = win ? mb : M;
            arg = win ? ab : arg;
        }
    double S = 0.0;
    if (live)
        for (int b = q; b < blocks; b += G) S += ws_s[base + b] * exp((double)ws_m[base + b] - (double)M);
    for (int o = 1; o < G; o <<= 1) {                      // every lane of the wave takes part, live or not
        const float Mo = __shfl_xor(M, o, 64);
        const double So = __shfl_xor(S, o, 64);
        const int ao = __shfl_xor(arg, o, 64);
        const float Mn = Mo > M ? Mo : M;
        const double mine = M > ninf ? S * exp((double)M - (double)Mn) : 0.0, theirs = Mo > ninf ? So * exp((double)Mo - (double)Mn) : 0.0;
        S = (threadIdx.x & o) ? theirs + mine : mine + theirs;
        arg = (Mo > M || (Mo == M && ao < arg)) ? ao : arg;
        M = Mn;
    }
    if (live && q == 0) {
        const double lse = (double)M + log(S);
        rows[i] = lse;
        rows[(long long)B + i] = lse - rows[2LL * B + i];
        pred[i] = arg;
    }
}

// one workgroup: the mean loss as a fixed-order double sum (thread t takes rows t, t + 256, ...), and the count of pred == label
__global__ __launch_bounds__(256) void head_mean_kernel(const double* __restrict__ rows, const int32_t* __restrict__ pred,
                                                        const int32_t* __restrict__ label, int B, double* __restrict__ mean_loss,
                                                        int32_t* __restrict__ correct) {
    __shared__ double lds4[4];
    double total = 0.0, hits = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        total += rows[(long long)B + i];
        hits += pred[i] == label[i] ? 1.0 : 0.0;
    }
    total = block_sum_d(total, lds4);
    hits = block_sum_d(hits, lds4);                        // integers below 2^53: exact in any order
    if (threadIdx.x == 0) {
        *mean_loss = total / (double)B;
        *correct = (int32_t)hits;
    }
}

// ---- logits -----------------------------------------------------------------------------------------------------------------------
// grid (class blocks of 128, row tiles of 128): a lane owns a class, its 64 values are rows of the batch; stores are coalesced along C.
__global__ __launch_bounds__(256) void head_logits_kernel(const float* __restrict__ x, const float* __restrict__ wn, const int32_t* __restrict__ label,
                                                          const float* __restrict__ zt32, int B, int D, int C, int vec, float lo, float hi,
                                                          float s, float* __restrict__ out) {
    __shared__ float sA[HB * HLD], sB[HB * HLD];
    __shared__ int sL[HB];
    __shared__ float sZ[HB];
    const int m0 = blockIdx.y * HB, n0 = blockIdx.x * HB;
    if (threadIdx.x < HB) {
        const int i = m0 + threadIdx.x;
        sL[threadIdx.x] = i < B ? label[i] : -1;
        sZ[threadIdx.x] = i < B ? zt32[i] : 0.f;
    }
    f32x16 acc[4];
    head_tile<4>(x, B, wn, C, D, vec != 0, m0, n0, sA, sB, acc);     // its barriers publish sL / sZ
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    if (j >= C) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = tile_row(t, e, h), i = m0 + il;
            const float z = s * clampf(acc[t][e], lo, hi);
            if (i < B) out[(long long)i * C + j] = j == sL[il] ? sZ[il] : z;
        }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
constexpr int GK = 4;                  // 32-column chunks of D per gradient workgroup: 128 columns, 4 accumulator tiles per wave
constexpr int GRAD_WGS = 256;          // class blocks x row tiles of the dX launch stays near this: bounds its partials
constexpr long long GRAD_MAX_PART = 1LL << 27;     // floats of dX partials (blocks x B x D) the backward accepts: 512 MiB

// grad_rows [3][B] double: [0] the target's slope d_i = dz_t / (s dr_t) with the clamp (and AdaFace's clip) folded in: 0 where the
// target is clamped away, [1] that mask, [2] |e_i| (AdaFace: 1, its rows are taken as they are).  From the double target cosine and
// margin scaler the forward's prep left in rows[3], rows[4]; the norm is summed in the order the prep sums it.
__global__ __launch_bounds__(256) void head_grad_prep_kernel(const float* __restrict__ emb, const double* __restrict__ rows, int B, int D,
                                                             HeadMargin mg, double* __restrict__ grad_rows) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= B) return;
    double uu = 0.0;
    if (mg.kind != IDB_HEAD_ADAFACE) {
        const float* e = emb + (long long)i * D;
        for (int k = l; k < D; k += 64) {
            const double x = (double)e[k];
            uu += x * x;
        }
        uu = wave_sum_d(uu);
    }
    if (l != 0) return;
    const double c = rows[3LL * B + i];
    double slope, mask;
    if (mg.kind == IDB_HEAD_COSFACE) {
        mask = c >= -1.0 && c <= 1.0 ? 1.0 : 0.0;      // inclusive, as torch's clamp backward; a NaN gives 0
        slope = mask;
    } else if (mg.kind == IDB_HEAD_ARCFACE) {
        mask = c >= -1.0 && c <= 1.0 ? 1.0 : 0.0;
        slope = mask != 0.0 ? sin(acos(c) + mg.m) / sqrt(1.0 - c * c) : 0.0;       // c = +-1 exactly: not finite, the caller refuses
    } else {
        mask = c >= -1.0 + ADA_EPS && c <= 1.0 - ADA_EPS ? 1.0 : 0.0;
        const double cc = clampd(c, -1.0 + ADA_EPS, 1.0 - ADA_EPS);
        const double theta = acos(cc) + mg.m * rows[4LL * B + i] * -1.0;
        slope = mask != 0.0 && theta >= ADA_EPS && theta <= M_PI - ADA_EPS ? sin(theta) / sqrt(1.0 - cc * cc) : 0.0;
    }
    grad_rows[i] = slope;
    grad_rows[(long long)B + i] = mask;
    grad_rows[2LL * B + i] = mg.kind == IDB_HEAD_ADAFACE ? 1.0 : sqrt(uu);
}

// Both gradient products.  A lane owns one row of P and meets, in its 64 accumulator registers, 64 of the 128 rows of each tile of Q:
//   DW = false (dX = G Wn):   P = the embeddings, Q = Wn; grid (class blocks, row tiles, D chunks); class block b takes class tiles
//                             b per .. of 128 and writes its partial dX rows and <x_i, dX_i> = sum_j G_ij r_ij to the workspace
//   DW = true  (dW = G^T X):  P = Wn, Q = the embeddings; grid (class tiles of 128, 1, D chunks); a workgroup takes every row tile in
//                             ascending order, so it holds the finished dW_j and <w_j, dW_j> = sum_i G_ij r_ij, projects and writes
//                             kernel.grad [D][C] (transposed through LDS: stores coalesced along C)
// The cosine tile acc[t][e] = <Q[m0 + tile_row(t, e, h)], P[lane's row]> is turned into G in place; it then is the A operand of
// out[p][k] += sum_q G[p][q] Q[q][k] with no lane movement: MFMA step (t, e) reduces over q = tile_row(t, e, h), h the half-wave,
// and reads Q[q][k] from the LDS stage as B.  A wave holds the accumulators of one chunk of 128 columns of D.
//   MULTI = false: the workgroup owns chunk blockIdx.z and keeps its accumulators in registers across its tiles of Q (D <= 128, where
//                  there is one chunk; and dW over several row tiles, where every chunk's workgroup recomputes the cosines)
//   MULTI = true:  the workgroup walks all chunks after each cosine tile, so the cosines are computed once.  dX: a chunk's accumulators
//                  are reloaded from the block's own partial, which the same lanes stored at the previous tile: the fma chain is the
//                  one a register-resident accumulator would run.  dW: chosen only where one row tile holds the whole batch.
template <bool DW, bool MULTI>
__global__ __launch_bounds__(256) void head_grad_kernel(const float* __restrict__ x, const float* __restrict__ wn, const int32_t* __restrict__ label,
                                                        const double* __restrict__ rows, const double* __restrict__ grad_rows, int B, int D,
                                                        int C, int vec, float lo, float hi, float s, double s_over_b, int per,
                                                        float* __restrict__ part, double* __restrict__ part_dot,
                                                        const float* __restrict__ kernel, const double* __restrict__ col_norm,
                                                        float* __restrict__ d_kernel) {
    __shared__ float sA[HB * HLD], sB[HB * HLD];
    __shared__ double sLse[HB];
    __shared__ float sGt[HB];
    __shared__ int sLab[HB];
    const float* Q = DW ? x : wn;
    const float* P = DW ? wn : x;
    const int nq = DW ? B : C, np = DW ? C : B;
    const int n0 = (DW ? blockIdx.x : blockIdx.y) * HB;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, r = l & 31, pj = n0 + w * 32 + r;
    const int tiles = (nq + HB - 1) / HB, chunks = (D + 32 * GK - 1) / (32 * GK);
    const int t0 = DW ? 0 : blockIdx.x * per, t1 = DW ? tiles : (t0 + per < tiles ? t0 + per : tiles);
    const int c0 = MULTI ? 0 : blockIdx.z, c1 = MULTI ? chunks : blockIdx.z + 1;
    const float s_over_b_f = (float)s_over_b;
    // the target's entry of G, per row: (p_t - 1) s d_t / B in double, p_t from the fp32 rounding of the target logit that the forward's
    // log-sum-exp saw (so the row's softmax sums to 1, and a single class gives exactly 0)
    int lab = -1;
    double lse = 0.0;
    float gt = 0.f;
    if (!DW && pj < B) {
        lab = label[pj];
        lse = rows[pj];
        gt = (float)((exp((double)(float)rows[2LL * B + pj] - lse) - 1.0) * s_over_b * grad_rows[pj]);
    }
    const double cn = DW && pj < C ? col_norm[pj] : 1.0;
    f32x16 out[GK];
#pragma unroll
    for (int kc = 0; kc < GK; ++kc)
#pragma unroll
        for (int e = 0; e < 16; ++e) out[kc][e] = 0.f;
    double dot = 0.0;

    // dX: the chunk's rows of this block's partial.  LOAD = false stores them, LOAD = true takes them back (zero where nothing is stored)
    auto partial = [&](int kbase, bool load) {
#pragma unroll
        for (int kc = 0; kc < GK; ++kc)
            if (kbase + 32 * kc < D) {
                const int k = kbase + 32 * kc + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int p = n0 + w * 32 + tile_row(0, e, h);
                    const long long o = ((long long)blockIdx.x * B + p) * D + k;
                    if (load) out[kc][e] = p < B && k < D ? part[o] : 0.f;
                    else if (p < B && k < D) part[o] = out[kc][e];
                }
            }
    };
    // dW: the chunk's finished sums, projected, divided and written as kernel.grad [D][C], transposed through LDS
    auto project = [&](int kbase, double total) {
#pragma unroll
        for (int kc = 0; kc < GK; ++kc)
            if (kbase + 32 * kc < D) {
                __syncthreads();                           // the previous transpose has been read
#pragma unroll
                for (int e = 0; e < 16; ++e) sB[(w * 32 + r) * HLD + tile_row(0, e, h)] = out[kc][e];     // [k][class]
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int k = kbase + 32 * kc + h * 16 + e;
                    if (pj < C && k < D) {
                        const long long o = (long long)k * C + pj;
                        const double wv = (double)kernel[o] / cn;
                        d_kernel[o] = (float)(((double)sB[(w * 32 + h * 16 + e) * HLD + r] - wv * total) / cn);
                    }
                }
            }
    };

    for (int tile = t0; tile < t1; ++tile) {
        const int m0 = tile * HB;
        if (DW && threadIdx.x < HB) {                      // published by head_tile's barriers; the last readers passed the barriers below
            const int i = m0 + threadIdx.x;
            const bool ok = i < B;
            sLab[threadIdx.x] = ok ? label[i] : -1;
            sLse[threadIdx.x] = ok ? rows[i] : 0.0;
            sGt[threadIdx.x] = ok ? (float)((exp((double)(float)rows[2LL * B + i] - rows[i]) - 1.0) * s_over_b * grad_rows[i]) : 0.f;
        }
        f32x16 acc[4];
        head_tile<4>(Q, nq, P, np, D, vec != 0, m0, n0, sA, sB, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ql = tile_row(t, e, h), qi = m0 + ql;
                const int cls = DW ? pj : qi, row = DW ? qi : pj;
                const float rr = acc[t][e];
                float g = 0.f;
                if (cls < C && row < B) {
                    const int rlab = DW ? sLab[ql] : lab;
                    const double rlse = DW ? sLse[ql] : lse;
                    const float z = s * clampf(rr, lo, hi);
                    const float p = expf((float)((double)z - rlse));
                    g = rr >= lo && rr <= hi ? p * s_over_b_f : 0.f;
                    g = cls == rlab ? (DW ? sGt[ql] : gt) : g;
                }
                dot += (double)g * (double)rr;
                acc[t][e] = g;
                if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four expf chains in flight, not sixty-four: registers
            }
        const float* rq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qr = (threadIdx.x >> 3) + 32 * i;
            rq[i] = m0 + qr < nq ? Q + (long long)(m0 + qr) * D : nullptr;
        }
        for (int c = c0; c < c1; ++c) {
            const int kbase = c * 32 * GK;
            if (MULTI) {
                if (!DW && tile > t0) partial(kbase, true);
                else {
#pragma unroll
                    for (int kc = 0; kc < GK; ++kc)
#pragma unroll
                        for (int e = 0; e < 16; ++e) out[kc][e] = 0.f;
                }
            }
#pragma unroll
            for (int kc = 0; kc < GK; ++kc)
                if (kbase + 32 * kc < D) {                 // uniform
                    f32x4 v[4];
                    head_fetch<4>(rq, D, vec != 0, kbase + 32 * kc, v);
                    __syncthreads();                       // the previous stage has been read
                    head_stash<4>(sA, v);
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            out[kc] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[t][e], sA[tile_row(t, e, h) * HLD + r], out[kc], 0, 0, 0);
                }
            if (MULTI) {
                if (DW) {                                  // the one row tile: the column's sum over the batch is complete
                    const double other = __shfl_xor(dot, 32, 64);
                    project(kbase, h == 0 ? dot + other : other + dot);
                } else {
                    partial(kbase, false);
                }
            }
        }
        __syncthreads();
    }
    // the two half-waves of a row of P: the lower half's term first
    const double other = __shfl_xor(dot, 32, 64);
    const double total = h == 0 ? dot + other : other + dot;
    if (!DW) {
        if (!MULTI) partial(c0 * 32 * GK, false);
        if (blockIdx.z == 0 && h == 0 && pj < B) part_dot[(long long)blockIdx.x * B + pj] = total;
    } else if (!MULTI) {
        project(c0 * 32 * GK, total);
    }
}

// One workgroup per embedding row: the class blocks' partials in ascending order (double), then the projection onto the tangent of
// the unit sphere and the division by |e_i|, one rounding.  AdaFace's rows are taken as they are: dX_i is the gradient.
__global__ __launch_bounds__(256) void head_grad_rows_kernel(const float* __restrict__ part, const double* __restrict__ part_dot,
                                                             const float* __restrict__ emb, const double* __restrict__ grad_rows, int blocks,
                                                             int B, int D, int ada, float* __restrict__ d_emb) {
    const int i = blockIdx.x;
    double rd = 0.0;
    for (int b = 0; b < blocks; ++b) rd += part_dot[(long long)b * B + i];
    const double n = grad_rows[2LL * B + i];
    for (int k = threadIdx.x; k < D; k += 256) {
        double acc = 0.0;
        for (int b = 0; b < blocks; ++b) acc += (double)part[((long long)b * B + i) * D + k];
        const long long o = (long long)i * D + k;
        d_emb[o] = ada ? (float)acc : (float)((acc - (double)emb[o] / n * rd) / n);
    }
}

// ---- clip_grad_norm_ and SGD (idb_sgd.h's arithmetic on one tensor) ------------------------------------------------------------------
// one workgroup per part
__global__ __launch_bounds__(256) void head_sqsum_kernel(const float* __restrict__ g, long long n, double* __restrict__ parts) {
    __shared__ double lds4[4];
    const double s = sgd_sqsum_part(g, n, gridDim.x, lds4);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// every workgroup adds the partials in the same fixed order (no launch of one workgroup between the two), then steps its part
__global__ __launch_bounds__(256) void head_sgd_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ buf, long long n,
                                                       const double* __restrict__ parts, double lr, double momentum, double wd,
                                                       double max_norm, int first, double* __restrict__ total_norm) {
    __shared__ double lds4[4];
    const double norm = sqrt(sgd_sum_parts(parts, gridDim.x, lds4));
    if (blockIdx.x == 0 && threadIdx.x == 0) *total_norm = norm;
    sgd_step_part(w, g, buf, n, gridDim.x, sgd_clip_coef(max_norm, norm), lr, momentum, wd, first);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct HeadPlan {
    int ta, row_tiles, tiles, per, col_blocks;
    size_t en, zt, m, s, a, total;                     // workspace offsets
};

// The widest class tile that still gives HEAD_FILL workgroups (B = 128, C = 10 572: 32-wide, 331 workgroups); past HEAD_MAX_WGS
// workgroups a column block takes several class tiles, so the partials stay small at the largest shapes.
HeadPlan head_plan(int b, int d, int c) {
    HeadPlan p;
    p.row_tiles = (b + HB - 1) / HB;
    p.ta = 1;
    for (int ta = 4; ta > 1; ta >>= 1)
        if ((long long)((c + 32 * ta - 1) / (32 * ta)) * p.row_tiles >= HEAD_FILL) {
            p.ta = ta;
            break;
        }
    p.tiles = (c + 32 * p.ta - 1) / (32 * p.ta);
    const int cap = HEAD_MAX_WGS / p.row_tiles > 1 ? HEAD_MAX_WGS / p.row_tiles : 1;
    p.per = (p.tiles + cap - 1) / cap;
    p.col_blocks = (p.tiles + p.per - 1) / p.per;
    size_t o = 0;
    p.en = o, o += align256(sizeof(float) * (size_t)b * d);
    p.zt = o, o += align256(sizeof(float) * (size_t)b);
    p.m = o, o += align256(sizeof(float) * (size_t)p.col_blocks * b);
    p.s = o, o += align256(sizeof(double) * (size_t)p.col_blocks * b);
    p.a = o, o += align256(sizeof(int32_t) * (size_t)p.col_blocks * b);
    p.total = o;
    return p;
}

inline bool head_dims_ok(int b, int d, int c) { return b >= 1 && b <= HEAD_MAX_B && d >= 1 && d <= HEAD_MAX_D && c >= 1 && c <= HEAD_MAX_C; }

int head_check(const char* api, const idb_head_desc* h, const void* ws, size_t ws_bytes) {
    IDB_REQUIRE(h, "%s: null descriptor", api);
    IDB_REQUIRE(h->kind == IDB_HEAD_COSFACE || h->kind == IDB_HEAD_ARCFACE || h->kind == IDB_HEAD_ADAFACE,
                "%s: loss kind %d, expected IDB_HEAD_COSFACE, IDB_HEAD_ARCFACE or IDB_HEAD_ADAFACE", api, h->kind);
    IDB_REQUIRE(head_dims_ok(h->b, h->d, h->c), "%s: b in 1..%d, d in 1..%d and c in 1..%d", api, HEAD_MAX_B, HEAD_MAX_D, HEAD_MAX_C);
    IDB_REQUIRE(h->kind != IDB_HEAD_ADAFACE || h->b >= 2, "%s: AdaFace needs b >= 2 (the unbiased std of one norm is NaN)", api);
    IDB_REQUIRE(h->s > 0.0 && h->s <= 1e4 && h->m == h->m && h->h == h->h && h->t_alpha >= 0.0 && h->t_alpha <= 1.0,
                "%s: s in (0, 1e4], finite m and h, t_alpha in [0, 1]", api);
    IDB_REQUIRE(h->wn && h->col_norm, "%s: the header is not packed (wn / col_norm are null): call idb_head_pack first", api);
    IDB_REQUIRE(h->emb && h->label && h->kernel, "%s: null pointer", api);
    IDB_REQUIRE(h->kind != IDB_HEAD_ADAFACE || (h->norms && h->ada_state), "%s: AdaFace needs norms and ada_state", api);
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= head_plan(h->b, h->d, h->c).total, "%s: workspace too small or unaligned", api);
    return IDB_OK;
}

// the launches loss and logits share: AdaFace statistics, then the per-row prep.  rows: [5][b] double.
int head_prep(const char* api, const idb_head_desc* h, const HeadPlan& p, char* ws, double* rows, hipStream_t st) {
    if (h->kind == IDB_HEAD_ADAFACE) {
        hipLaunchKernelGGL(head_ada_stats_kernel, dim3(1), dim3(256), 0, st, h->norms, h->b, h->t_alpha, h->ada_state);
        IDB_CHECK_LAUNCH(api);
    }
    hipLaunchKernelGGL(head_prep_kernel, dim3((h->b + 3) / 4), dim3(256), 0, st, h->emb, h->norms, h->label, h->kernel, h->col_norm,
                       (const double*)h->ada_state, h->b, h->d, h->c, HeadMargin{h->kind, h->s, h->m, h->h}, (float*)(ws + p.en),
                       (float*)(ws + p.zt), rows);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

// the launches of idb_head_loss, after its checks
int head_loss_run(const idb_head_desc* h, double* rows, int32_t* pred, double* mean_loss, int32_t* correct, char* w, hipStream_t st) {
    const HeadPlan p = head_plan(h->b, h->d, h->c);
    const int rc = head_prep("idb_head_loss(prep)", h, p, w, rows, st);
    if (rc != IDB_OK) return rc;
    const bool ada = h->kind == IDB_HEAD_ADAFACE;
    const float* x = ada ? h->emb : (const float*)(w + p.en);
    const float lo = ada ? (float)(-1.0 + ADA_EPS) : -1.f, hi = ada ? (float)(1.0 - ADA_EPS) : 1.f;
    const int vec = h->d % 4 == 0 && idb_aligned16(x) && idb_aligned16(h->wn);
    const dim3 grid(p.col_blocks, p.row_tiles);
#define HEAD_LOSS(TA)                                                                                                                   \
    hipLaunchKernelGGL(head_loss_kernel<TA>, grid, dim3(256), 0, st, x, h->wn, h->label, (const float*)(w + p.zt), h->b, h->d, h->c, vec, lo, \
                       hi, (float)h->s, p.per, (float*)(w + p.m), (double*)(w + p.s), (int32_t*)(w + p.a))
    if (p.ta == 4) HEAD_LOSS(4);
    else if (p.ta == 2) HEAD_LOSS(2);
    else HEAD_LOSS(1);
#undef HEAD_LOSS
    IDB_CHECK_LAUNCH("idb_head_loss");
    int lanes = 1;                                     // lanes that share a row in the merge: the column blocks, up to a wave
    while (lanes < 64 && lanes < p.col_blocks) lanes <<= 1;
    const int rows_per_wg = MERGE_THREADS / lanes;
    hipLaunchKernelGGL(head_merge_kernel, dim3((h->b + rows_per_wg - 1) / rows_per_wg), dim3(MERGE_THREADS), 0, st, (const float*)(w + p.m),
                       (const double*)(w + p.s), (const int32_t*)(w + p.a), p.col_blocks, h->b, lanes, rows, pred);
    IDB_CHECK_LAUNCH("idb_head_loss(merge)");
    hipLaunchKernelGGL(head_mean_kernel, dim3(1), dim3(256), 0, st, (const double*)rows, (const int32_t*)pred, h->label, h->b, mean_loss,
                       correct);
    IDB_CHECK_LAUNCH("idb_head_loss(mean)");
    return IDB_OK;
}

struct HeadGradPlan {
    int row_tiles, per, blocks, chunks;                // the dX launch's grid is (blocks, row_tiles), the dW launch's (class tiles, 1, 1 or chunks)
    size_t part, dot, total;                           // workspace offsets, after the forward's
    bool ok;                                           // the dX partials fit GRAD_MAX_PART
};

// Class blocks of the dX launch: about GRAD_WGS workgroups per D chunk (B = 128, C = 10 572: 83 blocks of one 128-class tile), so
// the partials are blocks x B x D floats, 64 MiB at B = 1024, C = 2^17, D = 512.
HeadGradPlan head_grad_plan(int b, int d, int c) {
    HeadGradPlan g;
    g.row_tiles = (b + HB - 1) / HB;
    const int tiles = (c + HB - 1) / HB, cap = GRAD_WGS / g.row_tiles > 1 ? GRAD_WGS / g.row_tiles : 1;
    g.per = (tiles + cap - 1) / cap;
    g.blocks = (tiles + g.per - 1) / g.per;
    g.chunks = (d + 32 * GK - 1) / (32 * GK);
    g.ok = (long long)g.blocks * b * d <= GRAD_MAX_PART;
    size_t o = head_plan(b, d, c).total;
    g.part = o, o += align256(sizeof(float) * (size_t)g.blocks * b * d);
    g.dot = o, o += align256(sizeof(double) * (size_t)g.blocks * b);
    g.total = o;
    return g;
}

}  // namespace

extern "C" int idb_head_pack(const float* kernel, int32_t d, int32_t c, float* wn, double* col_norm, int32_t* bad_cols, void* stream) {
    IDB_REQUIRE(head_dims_ok(1, d, c), "idb_head_pack: d in 1..%d and c in 1..%d", HEAD_MAX_D, HEAD_MAX_C);
    IDB_REQUIRE(kernel && wn && col_norm && bad_cols, "idb_head_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad_cols, 0, sizeof(int32_t), st) != hipSuccess) {
        idb_set_error("idb_head_pack: hipMemsetAsync failed");
        return IDB_EHIP;
    }
    hipLaunchKernelGGL(head_pack_kernel, dim3((c + 63) / 64), dim3(256), 0, st, kernel, d, c, wn, col_norm, bad_cols);
    IDB_CHECK_LAUNCH("idb_head_pack");
    return IDB_OK;
}

extern "C" size_t idb_head_workspace_bytes(int32_t b, int32_t d, int32_t c, int32_t* row_tiles, int32_t* col_blocks) {
    if (!head_dims_ok(b, d, c)) return 0;
    const HeadPlan p = head_plan(b, d, c);
    if (row_tiles) *row_tiles = p.row_tiles;
    if (col_blocks) *col_blocks = p.col_blocks;
    return p.total;
}

extern "C" int idb_head_loss(const idb_head_desc* h, double* rows, int32_t* pred, double* mean_loss, int32_t* correct, void* ws,
                             size_t ws_bytes, void* stream) {
    const int rc0 = head_check("idb_head_loss", h, ws, ws_bytes);
    if (rc0 != IDB_OK) return rc0;
    IDB_REQUIRE(rows && pred && mean_loss && correct, "idb_head_loss: null output pointer");
    return head_loss_run(h, rows, pred, mean_loss, correct, (char*)ws, (hipStream_t)stream);
}

extern "C" int idb_head_logits(const idb_head_desc* h, float* thetas, double* rows, void* ws, size_t ws_bytes, void* stream) {
    const int rc0 = head_check("idb_head_logits", h, ws, ws_bytes);
    if (rc0 != IDB_OK) return rc0;
    IDB_REQUIRE(thetas && rows, "idb_head_logits: null output pointer");
    hipStream_t st = (hipStream_t)stream;
    const HeadPlan p = head_plan(h->b, h->d, h->c);
    char* w = (char*)ws;
    const int rc = head_prep("idb_head_logits(prep)", h, p, w, rows, st);
    if (rc != IDB_OK) return rc;
    const bool ada = h->kind == IDB_HEAD_ADAFACE;
    const float* x = ada ? h->emb : (const float*)(w + p.en);
    const float lo = ada ? (float)(-1.0 + ADA_EPS) : -1.f, hi = ada ? (float)(1.0 - ADA_EPS) : 1.f;
    const int vec = h->d % 4 == 0 && idb_aligned16(x) && idb_aligned16(h->wn);
    hipLaunchKernelGGL(head_logits_kernel, dim3((h->c + HB - 1) / HB, (h->b + HB - 1) / HB), dim3(256), 0, st, x, h->wn, h->label,
                       (const float*)(w + p.zt), h->b, h->d, h->c, vec, lo, hi, (float)h->s, thetas);
    IDB_CHECK_LAUNCH("idb_head_logits");
    return IDB_OK;
}

extern "C" size_t idb_head_grad_workspace_bytes(int32_t b, int32_t d, int32_t c, int32_t* row_tiles, int32_t* class_blocks, int32_t* d_chunks) {
    if (!head_dims_ok(b, d, c)) return 0;
    const HeadGradPlan g = head_grad_plan(b, d, c);
    if (!g.ok) return 0;
    if (row_tiles) *row_tiles = g.row_tiles;
    if (class_blocks) *class_blocks = g.blocks;
    if (d_chunks) *d_chunks = g.chunks;
    return g.total;
}

extern "C" int idb_head_loss_grad(const idb_head_desc* h, double* rows, int32_t* pred, double* mean_loss, int32_t* correct, double* grad_rows,
                                  float* d_emb, float* d_kernel, void* ws, size_t ws_bytes, void* stream) {
    const int rc0 = head_check("idb_head_loss_grad", h, ws, ws_bytes);
    if (rc0 != IDB_OK) return rc0;
    IDB_REQUIRE(rows && pred && mean_loss && correct && grad_rows && d_emb && d_kernel, "idb_head_loss_grad: null output pointer");
    const HeadGradPlan g = head_grad_plan(h->b, h->d, h->c);
    if (!g.ok) {
        idb_set_error("idb_head_loss_grad: class blocks x b x d = %d x %d x %d floats of dX partials, the limit is 2^27 (512 MiB)", g.blocks,
                      h->b, h->d);
        return IDB_EUNSUPPORTED;
    }
    IDB_REQUIRE(ws_bytes >= g.total, "idb_head_loss_grad: workspace too small (idb_head_grad_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const int rc = head_loss_run(h, rows, pred, mean_loss, correct, w, st);
    if (rc != IDB_OK) return rc;
    const HeadPlan p = head_plan(h->b, h->d, h->c);
    const bool ada = h->kind == IDB_HEAD_ADAFACE;
    const float* x = ada ? h->emb : (const float*)(w + p.en);
    const float lo = ada ? (float)(-1.0 + ADA_EPS) : -1.f, hi = ada ? (float)(1.0 - ADA_EPS) : 1.f;
    const int vec = h->d % 4 == 0 && idb_aligned16(x) && idb_aligned16(h->wn);
    hipLaunchKernelGGL(head_grad_prep_kernel, dim3((h->b + 3) / 4), dim3(256), 0, st, h->emb, (const double*)rows, h->b, h->d,
                       HeadMargin{h->kind, h->s, h->m, h->h}, grad_rows);
    IDB_CHECK_LAUNCH("idb_head_loss_grad(prep)");
    const double s_over_b = h->s / (double)h->b;
    float* part = (float*)(w + g.part);
    double* dot = (double*)(w + g.dot);
#define HEAD_GRAD(DW, MULTI, GRID, PER)                                                                                                   \
    hipLaunchKernelGGL((head_grad_kernel<DW, MULTI>), GRID, dim3(256), 0, st, x, h->wn, h->label, (const double*)rows,                      \
                       (const double*)grad_rows, h->b, h->d, h->c, vec, lo, hi, (float)h->s, s_over_b, PER, part, dot, h->kernel, h->col_norm, \
                       d_kernel)
    // past one chunk of 128 columns a workgroup walks all chunks per cosine tile; dW can do so only where one row tile holds the batch
    if (g.chunks > 1) HEAD_GRAD(false, true, dim3(g.blocks, g.row_tiles, 1), g.per);
    else HEAD_GRAD(false, false, dim3(g.blocks, g.row_tiles, 1), g.per);
    IDB_CHECK_LAUNCH("idb_head_loss_grad(dX)");
    hipLaunchKernelGGL(head_grad_rows_kernel, dim3(h->b), dim3(256), 0, st, (const float*)part, (const double*)dot, h->emb,
                       (const double*)grad_rows, g.blocks, h->b, h->d, ada ? 1 : 0, d_emb);
    IDB_CHECK_LAUNCH("idb_head_loss_grad(rows)");
    if (g.chunks > 1 && g.row_tiles == 1) HEAD_GRAD(true, true, dim3((h->c + HB - 1) / HB, 1, 1), 0);
    else HEAD_GRAD(true, false, dim3((h->c + HB - 1) / HB, 1, g.chunks), 0);
#undef HEAD_GRAD
    IDB_CHECK_LAUNCH("idb_head_loss_grad(dW)");
    return IDB_OK;
}

extern "C" int idb_head_sgd_step(float* kernel, const float* grad, float* momentum_buf, int32_t d, int32_t c, double lr, double momentum,
                                 double weight_decay, double max_norm, int32_t first_step, float* wn, double* col_norm, int32_t* bad_cols,
                                 double* total_norm, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(head_dims_ok(1, d, c), "idb_head_sgd_step: d in 1..%d and c in 1..%d", HEAD_MAX_D, HEAD_MAX_C);
    IDB_REQUIRE(kernel && grad && momentum_buf && wn && col_norm && bad_cols && total_norm, "idb_head_sgd_step: null pointer");
    IDB_REQUIRE(lr >= 0.0 && lr <= 1e4 && momentum >= 0.0 && momentum < 1.0 && weight_decay >= 0.0 && weight_decay <= 1e4 && max_norm > 0.0 &&
                    max_norm <= 1e30,
                "idb_head_sgd_step: lr in [0, 1e4], momentum in [0, 1), weight_decay in [0, 1e4], max_norm in (0, 1e30]");
    IDB_REQUIRE(ws && idb_aligned16(ws) && ws_bytes >= IDB_HEAD_SGD_WS_BYTES, "idb_head_sgd_step: workspace too small or unaligned (%d bytes)",
                IDB_HEAD_SGD_WS_BYTES);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)d * c;
    const int nparts = sgd_parts(n);
    hipLaunchKernelGGL(head_sqsum_kernel, dim3(nparts), dim3(256), 0, st, grad, n, (double*)ws);
    IDB_CHECK_LAUNCH("idb_head_sgd_step(norm)");
    hipLaunchKernelGGL(head_sgd_kernel, dim3(nparts), dim3(256), 0, st, kernel, grad, momentum_buf, n, (const double*)ws, lr, momentum, weight_decay,
                       max_norm, first_step != 0, total_norm);
    IDB_CHECK_LAUNCH("idb_head_sgd_step");
    return idb_head_pack(kernel, d, c, wn, col_norm, bad_cols, stream);
}
