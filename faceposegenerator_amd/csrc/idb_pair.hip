// All-pairs work over fp32 feature matrices (the dgm-eval metrics ID-Booth's evaluation notebook runs on DINOv2 features: PRDC, KD,
// AuthPct) on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32): hard threshold comparisons on nearest-neighbour distances cannot be
// taken on 16-bit products.  One tile engine computes A[Na][D] . B[Nb][D]^T for a 128 x 128 tile per workgroup; the modes below are
// kernels over that main loop and none but the plain store mode writes the Na x Nb matrix.
//   d2(i, j) = max(|a_i - s|^2 + |b_j - s|^2 - 2 (a_i - s).(b_j - s), 0): the caller's shift s [D] is subtracted where the operands
//   are loaded (distances are translation invariant; with s = the mean of the data the two norms stop cancelling against the
//   product); the row norms of the shifted rows come from a prepass, fp32.
// Accumulator layout of the 32x32 tile: lane l holds column (l & 31) and rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), reg < 16.  A wave
// owns 32 columns (rows of B) and all 128 rows of the tile, so every lane owns ONE row of B: whatever is reduced per row of B (k
// nearest candidates of a query, the nearest neighbour, counts) stays in that lane's registers, and the two half-waves that share a
// column are merged afterwards.  Everything is deterministic: integer atomics only, float sums in a fixed order.
#include "idb_f32mma.h"

namespace {

constexpr int PT = 128;            // tile rows and columns
constexpr int PK = 32;             // K per LDS stage
constexpr int PLD = PK + 1;        // LDS row stride in floats: lanes of a half-wave read 32 rows at one k, 33 r mod 64 is injective
constexpr int KNN_MAX = 8;         // candidates kept per query (k + 1 <= 8)
constexpr int PAIR_MAX_SPLITS = 8; // workgroups that share the rows of A for one block of columns

// rows of a feature matrix, gathered through idx when it is not null
struct Operand {
    const float* x;
    const int32_t* idx;
    int n;
};

__device__ __forceinline__ float dist2_of(float na, float nb, float dot) {
    const float d = (na + nb) - 2.f * dot;
    return d > 0.f ? d : 0.f;      // never -0: the bits of a distance order as unsigned integers
}

// Thread t stages columns 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i, i < 4, of each operand: 8 lanes read 128 contiguous bytes of a row.
__device__ __forceinline__ void pair_fetch(const float* const (&row)[4], const float* shift, int D, bool vec, int k0, f32x4 (&v)[4]) {
    const int k = k0 + (threadIdx.x & 7) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (shift) {
        if (vec) {
            if (k < D) s = *(const f32x4*)(shift + k);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k + e < D) s[e] = shift[k + e];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};                // rows past the end and columns past D are zero AFTER the shift
        if (row[i]) {
            if (vec) {
                if (k < D) x = *(const f32x4*)(row[i] + k) - s;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < D) x[e] = row[i][k + e] - s[e];
            }
        }
        v[i] = x;
    }
}

__device__ __forceinline__ void pair_stash(float* lds, const f32x4 (&v)[4]) {
    const int c = (threadIdx.x & 7) * 4, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[(r + 32 * i) * PLD + c + e] = v[i][e];
}

// acc[t] (+)= rows m0 + 32 t .. of a times columns n0 + 32 wave .. of b, over all of D.  vec: D % 4 == 0 and 16-byte aligned bases.
// Ends with a barrier, so the caller may reuse its own shared arrays after the epilogue only behind one more barrier.
__device__ __forceinline__ void pair_tile(const Operand& a, const Operand& b, const float* shift, int D, bool vec, int m0, int n0,
                                          float* sA, float* sB, f32x16 (&acc)[4]) {
    const float* ra[4];
    const float* rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (threadIdx.x >> 3) + 32 * i;
        ra[i] = m0 + r < a.n ? a.x + (long long)(a.idx ? a.idx[m0 + r] : m0 + r) * D : nullptr;
        rb[i] = n0 + r < b.n ? b.x + (long long)(b.idx ? b.idx[n0 + r] : n0 + r) * D : nullptr;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
    f32x4 va[4], vb[4];
    pair_fetch(ra, shift, D, vec, 0, va);
    pair_fetch(rb, shift, D, vec, 0, vb);
    for (int k0 = 0; k0 < D; k0 += PK) {
        __syncthreads();                               // the previous stage has been read
        pair_stash(sA, va);
        pair_stash(sB, vb);
        __syncthreads();
        if (k0 + PK < D) {                             // the next stage's loads fly during this stage's MFMAs
            pair_fetch(ra, shift, D, vec, k0 + PK, va);
            pair_fetch(rb, shift, D, vec, k0 + PK, vb);
        }
#pragma unroll
        for (int kk = 0; kk < PK; kk += 2) {           // A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
            const float bv = sB[(w * 32 + r) * PLD + kk + h];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[(t * 32 + r) * PLD + kk + h], bv, acc[t], 0, 0, 0);
        }
    }
    __syncthreads();
}

// |x_r - s|^2 of every row, one wave per row, lane l takes columns l, l + 64, ...; fixed order.
__global__ __launch_bounds__(256) void pair_norms_kernel(const float* __restrict__ x, const float* __restrict__ shift, int n, int D,
                                                         float* __restrict__ out) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (r >= n) return;
    const float* xr = x + (long long)r * D;
    float s = 0.f;
    for (int k = l; k < D; k += 64) {
        const float v = xr[k] - (shift ? shift[k] : 0.f);
        s = __builtin_fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (l == 0) out[r] = s;
}

// ---- dist2 (store) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_dist2_kernel(Operand a, Operand b, const float* shift, int D, int vec, const float* na,
                                                         const float* nb, float* out) {
    __shared__ float sA[PT * PLD], sB[PT * PLD];
    const int m0 = blockIdx.y * PT, n0 = blockIdx.x * PT;
    f32x16 acc[4];
    pair_tile(a, b, shift, D, vec != 0, m0, n0, sA, sB, acc);
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    if (j >= b.n) return;
    const float nbj = nb[j];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = m0 + tile_row(t, e, h);
            if (i < a.n) out[(long long)i * b.n + j] = dist2_of(na[i], nbj, acc[t][e]);
        }
}

// ---- k nearest: the KNN_MAX smallest of a column, ascending, in registers --------------------
// Statically indexed throughout (a dynamically indexed list would live in scratch).  Equal values are kept with their multiplicity.
__device__ __forceinline__ void knn_insert(float (&L)[KNN_MAX], float v) {
    if (v < L[KNN_MAX - 1]) {
#pragma unroll
        for (int t = KNN_MAX - 1; t > 0; --t) L[t] = v < L[t - 1] ? L[t - 1] : (v < L[t] ? v : L[t]);
        L[0] = v < L[0] ? v : L[0];
    }
}

// grid (column blocks, splits): split s takes row blocks s, s + splits, ...; the queries are the columns.  Each half-wave writes its
// list to ws[(2 s + h)][n][KNN_MAX].
__global__ __launch_bounds__(256) void pair_knn_kernel(Operand x, const float* shift, int D, int vec, const float* nx, float* ws) {
    __shared__ float sA[PT * PLD], sB[PT * PLD];
    __shared__ float sN[PT];
    const int n0 = blockIdx.x * PT, n = x.n, blocks = (n + PT - 1) / PT;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    const float nj = j < n ? nx[j] : 0.f;
    float L[KNN_MAX];
#pragma unroll
    for (int e = 0; e < KNN_MAX; ++e) L[e] = __builtin_inff();
    for (int mb = blockIdx.y; mb < blocks; mb += gridDim.y) {
        const int m0 = mb * PT;
        if (threadIdx.x < PT) sN[threadIdx.x] = m0 + threadIdx.x < n ? nx[m0 + threadIdx.x] : 0.f;
        f32x16 acc[4];
        pair_tile(x, x, shift, D, vec != 0, m0, n0, sA, sB, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = tile_row(t, e, h), i = m0 + il;
                if (i < n) knn_insert(L, i == j ? 0.f : dist2_of(sN[il], nj, acc[t][e]));   // the point itself: exactly 0
            }
        __syncthreads();                               // sN is rewritten by the next block
    }
    if (j < n) {
        float* o = ws + ((long long)(2 * blockIdx.y + h) * n + j) * KNN_MAX;
#pragma unroll
        for (int e = 0; e < KNN_MAX; ++e) o[e] = L[e];
    }
}

// one thread per query: merge the lists in a fixed order, take the kth smallest (kth = 1 is the point itself)
__global__ __launch_bounds__(256) void pair_knn_merge_kernel(const float* __restrict__ ws, int lists, int n, int kth, float* __restrict__ r2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float L[KNN_MAX];
#pragma unroll
    for (int e = 0; e < KNN_MAX; ++e) L[e] = __builtin_inff();
    for (int s = 0; s < lists; ++s) {
        const float* o = ws + ((long long)s * n + j) * KNN_MAX;
#pragma unroll
        for (int e = 0; e < KNN_MAX; ++e) knn_insert(L, o[e]);
    }
    float r = L[0];
#pragma unroll
    for (int e = 1; e < KNN_MAX; ++e) r = e == kth - 1 ? L[e] : r;
    r2[j] = r;
}

// ---- nearest neighbour of every column --------------------------------------------------------
// grid (column blocks, splits); ws_min / ws_idx [(2 s + h)][nb].  A lane meets its rows in ascending order, so the strict comparison
// alone keeps the lowest index on a tie; the index test makes that independent of the visiting order.
__global__ __launch_bounds__(256) void pair_nn_kernel(Operand a, Operand b, const float* shift, int D, int vec, const float* na,
                                                      const float* nb, int excl, float* ws_min, int32_t* ws_idx) {
    __shared__ float sA[PT * PLD], sB[PT * PLD];
    __shared__ float sN[PT];
    const int n0 = blockIdx.x * PT, blocks = (a.n + PT - 1) / PT;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    const float nbj = j < b.n ? nb[j] : 0.f;
    float best = __builtin_inff();
    int bi = 0x7fffffff;
    for (int mb = blockIdx.y; mb < blocks; mb += gridDim.y) {
        const int m0 = mb * PT;
        if (threadIdx.x < PT) sN[threadIdx.x] = m0 + threadIdx.x < a.n ? na[m0 + threadIdx.x] : 0.f;
        f32x16 acc[4];
        pair_tile(a, b, shift, D, vec != 0, m0, n0, sA, sB, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int il = tile_row(t, e, h), i = m0 + il;
                const float d = dist2_of(sN[il], nbj, acc[t][e]);
                const bool ok = i < a.n && !(excl && i == j) && (d < best || (d == best && i < bi));
                best = ok ? d : best;
                bi = ok ? i : bi;
            }
        __syncthreads();
    }
    if (j < b.n) {
        const long long o = (long long)(2 * blockIdx.y + h) * b.n + j;
        ws_min[o] = best;
        ws_idx[o] = bi;
    }
}

__global__ __launch_bounds__(256) void pair_nn_merge_kernel(const float* __restrict__ ws_min, const int32_t* __restrict__ ws_idx, int lists,
                                                            int nb, float* __restrict__ min_d2, int32_t* __restrict__ argmin) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    float best = __builtin_inff();
    int bi = 0x7fffffff;
    for (int s = 0; s < lists; ++s) {
        const float d = ws_min[(long long)s * nb + j];
        const int i = ws_idx[(long long)s * nb + j];
        if (i != 0x7fffffff && (d < best || (d == best && i < bi))) {
            best = d;
            bi = i;
        }
    }
    min_d2[j] = best;
    argmin[j] = bi == 0x7fffffff ? -1 : bi;
}

// ---- PRDC counts --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_prdc_init_kernel(int32_t* in_real, int ng, int32_t* covered, uint32_t* row_min, int nr) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < ng) in_real[t] = 0;
    if (t < nr) {
        covered[t] = 0;
        row_min[t] = 0x7f800000u;                      // +inf
    }
}

// grid (gen blocks, real blocks): rows = real, columns = gen, one tile per workgroup.  The per-column count stays in the lane; the
// per-row minimum and flag go through LDS integer atomics (the bits of a non-negative float order as unsigned integers), then one
// global integer atomic per row: the result does not depend on the order.
__global__ __launch_bounds__(256) void pair_prdc_kernel(Operand a, Operand b, const float* shift, int D, int vec, const float* na,
                                                        const float* nb, const float* r2a, const float* r2b, int32_t* in_real,
                                                        int32_t* covered, uint32_t* row_min) {
    __shared__ float sA[PT * PLD], sB[PT * PLD];
    __shared__ float sN[PT], sR[PT];
    __shared__ uint32_t sMin[PT];
    __shared__ int32_t sCov[PT];
    const int m0 = blockIdx.y * PT, n0 = blockIdx.x * PT;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    if (threadIdx.x < PT) {
        const int i = m0 + threadIdx.x;
        sN[threadIdx.x] = i < a.n ? na[i] : 0.f;
        sR[threadIdx.x] = i < a.n ? r2a[i] : 0.f;
        sMin[threadIdx.x] = 0x7f800000u;
        sCov[threadIdx.x] = 0;
    }
    f32x16 acc[4];
    pair_tile(a, b, shift, D, vec != 0, m0, n0, sA, sB, acc);
    const bool col = j < b.n;
    const float nbj = col ? nb[j] : 0.f, r2j = col ? r2b[j] : 0.f;
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = tile_row(t, e, h);
            if (col && m0 + il < a.n) {
                const float d = dist2_of(sN[il], nbj, acc[t][e]);
                cnt += d < sR[il] ? 1 : 0;
                atomicMin(&sMin[il], __float_as_uint(d));
                if (d < r2j) atomicOr(&sCov[il], 1);
            }
        }
    cnt += __shfl_xor(cnt, 32, 64);
    if (h == 0 && col && cnt) atomicAdd(&in_real[j], cnt);
    __syncthreads();
    if (threadIdx.x < PT && m0 + threadIdx.x < a.n) {
        atomicMin(&row_min[m0 + threadIdx.x], sMin[threadIdx.x]);
        if (sCov[threadIdx.x]) atomicOr(&covered[m0 + threadIdx.x], 1);
    }
}

// ---- polynomial-kernel sums -----------------------------------------------------------------
// grid (tiles, tiles, 3 S): matrix z = 3 s + which, which 0: x_s x x_s without the diagonal, 1: y_s x y_s without it, 2: x_s x y_s.
// partial[z][tile row][tile column] = the tile's sum of (gamma a.b + c0)^3, fp32: the lane's 64 values in register order, the
// shuffle tree of the wave, then the four waves left to right.
__global__ __launch_bounds__(256) void pair_poly_kernel(const float* x, const float* y, const int32_t* idx_x, const int32_t* idx_y, int m,
                                                        int D, int vec, float gamma, float c0, float* partial) {
    __shared__ float sA[PT * PLD], sB[PT * PLD];
    __shared__ float red[4];
    const int s = blockIdx.z / 3, which = blockIdx.z - 3 * s;
    const Operand a = {which == 1 ? y : x, (which == 1 ? idx_y : idx_x) + (long long)s * m, m};
    const Operand b = {which == 0 ? x : y, (which == 0 ? idx_x : idx_y) + (long long)s * m, m};
    const int m0 = blockIdx.y * PT, n0 = blockIdx.x * PT;
    f32x16 acc[4];
    pair_tile(a, b, nullptr, D, vec != 0, m0, n0, sA, sB, acc);
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, h = l >> 5, j = n0 + w * 32 + (l & 31);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = m0 + tile_row(t, e, h);
            const float v = __builtin_fmaf(gamma, acc[t][e], c0);
            const bool ok = i < m && j < m && !(which != 2 && i == j);
            sum += ok ? v * v * v : 0.f;
        }
    sum = wave_sum(sum);
    if (l == 0) red[w] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one thread per matrix: the tile sums in row-major tile order, in double
__global__ __launch_bounds__(64) void pair_poly_reduce_kernel(const float* __restrict__ partial, int mats, int tiles, double* __restrict__ sums) {
    const int z = blockIdx.x * 64 + threadIdx.x;
    if (z >= mats) return;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += (double)partial[(long long)z * tiles + t];
    sums[z] = s;
}

// ---- host ---------------------------------------------------------------------------------------
constexpr int PAIR_MAX_N = 1 << 22, PAIR_MAX_D = 1 << 16;
inline int pair_blocks(int n) { return (n + PT - 1) / PT; }
inline int pair_splits(int rows) { return pair_blocks(rows) < PAIR_MAX_SPLITS ? pair_blocks(rows) : PAIR_MAX_SPLITS; }
inline bool pair_vec(int d, const void* a, const void* b, const void* s) {
    return d % 4 == 0 && idb_aligned16(a) && idb_aligned16(b) && (!s || idb_aligned16(s));
}
inline bool pair_dims_ok(int na, int nb, int d) { return na > 0 && nb > 0 && d > 0 && na <= PAIR_MAX_N && nb <= PAIR_MAX_N && d <= PAIR_MAX_D; }

size_t pair_ws_bytes(int mode, int na, int nb, int subsets) {
    const size_t norms = align256(sizeof(float) * na) + align256(sizeof(float) * nb);
    switch (mode) {
        case IDB_PAIR_DIST2:
        case IDB_PAIR_PRDC: return norms;
        case IDB_PAIR_KNN: return align256(sizeof(float) * na) + align256(sizeof(float) * 2 * pair_splits(na) * (size_t)na * KNN_MAX);
        case IDB_PAIR_NEAREST: return norms + 2 * align256(sizeof(float) * 2 * pair_splits(na) * (size_t)nb);
        case IDB_PAIR_POLY: return align256(sizeof(float) * 3 * (size_t)subsets * pair_blocks(na) * pair_blocks(na));
    }
    return 0;
}

int pair_norms(const char* api, const float* x, const float* shift, int n, int d, float* out, hipStream_t st) {
    hipLaunchKernelGGL(pair_norms_kernel, dim3((n + 3) / 4), dim3(256), 0, st, x, shift, n, d, out);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

}  // namespace

extern "C" size_t idb_pair_workspace_bytes(int32_t mode, int32_t na, int32_t nb, int32_t subsets) {
    if (mode < IDB_PAIR_DIST2 || mode > IDB_PAIR_POLY || na <= 0 || na > PAIR_MAX_N) return 0;
    if (mode == IDB_PAIR_POLY) return subsets > 0 && subsets <= 21845 ? pair_ws_bytes(mode, na, na, subsets) : 0;
    if (mode == IDB_PAIR_KNN) return pair_ws_bytes(mode, na, na, 0);
    return nb > 0 && nb <= PAIR_MAX_N ? pair_ws_bytes(mode, na, nb, 0) : 0;
}

extern "C" int idb_pair_dist2(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const float* shift, float* out, void* ws,
                              size_t ws_bytes, void* stream) {
    IDB_REQUIRE(pair_dims_ok(na, nb, d), "idb_pair_dist2: na, nb in 1..%d and d in 1..%d", PAIR_MAX_N, PAIR_MAX_D);
    IDB_REQUIRE(a && b && out && ws, "idb_pair_dist2: null pointer");
    IDB_REQUIRE(ws_bytes >= pair_ws_bytes(IDB_PAIR_DIST2, na, nb, 0) && idb_aligned16(ws), "idb_pair_dist2: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    float* nra = (float*)ws;
    float* nrb = (float*)((char*)ws + align256(sizeof(float) * na));
    int rc = pair_norms("idb_pair_dist2", a, shift, na, d, nra, st);
    if (rc == IDB_OK) rc = pair_norms("idb_pair_dist2", b, shift, nb, d, nrb, st);
    if (rc != IDB_OK) return rc;
    hipLaunchKernelGGL(pair_dist2_kernel, dim3(pair_blocks(nb), pair_blocks(na)), dim3(256), 0, st, Operand{a, nullptr, na},
                       Operand{b, nullptr, nb}, shift, d, (int)pair_vec(d, a, b, shift), (const float*)nra, (const float*)nrb, out);
    IDB_CHECK_LAUNCH("idb_pair_dist2");
    return IDB_OK;
}

extern "C" int idb_pair_knn_radii(const float* x, int32_t n, int32_t d, const float* shift, int32_t kth, float* r2, void* ws, size_t ws_bytes,
                                  void* stream) {
    IDB_REQUIRE(pair_dims_ok(n, n, d), "idb_pair_knn_radii: n in 1..%d and d in 1..%d", PAIR_MAX_N, PAIR_MAX_D);
    IDB_REQUIRE(kth >= 1 && kth <= KNN_MAX && kth <= n, "idb_pair_knn_radii: kth (= nearest_k + 1) in 1..min(%d, n)", KNN_MAX);
    IDB_REQUIRE(x && r2 && ws, "idb_pair_knn_radii: null pointer");
    IDB_REQUIRE(ws_bytes >= pair_ws_bytes(IDB_PAIR_KNN, n, n, 0) && idb_aligned16(ws), "idb_pair_knn_radii: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    float* nx = (float*)ws;
    float* lists = (float*)((char*)ws + align256(sizeof(float) * n));
    const int splits = pair_splits(n);
    int rc = pair_norms("idb_pair_knn_radii", x, shift, n, d, nx, st);
    if (rc != IDB_OK) return rc;
    hipLaunchKernelGGL(pair_knn_kernel, dim3(pair_blocks(n), splits), dim3(256), 0, st, Operand{x, nullptr, n}, shift, d,
                       (int)pair_vec(d, x, x, shift), (const float*)nx, lists);
    IDB_CHECK_LAUNCH("idb_pair_knn_radii");
    hipLaunchKernelGGL(pair_knn_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)lists, 2 * splits, n, kth, r2);
    IDB_CHECK_LAUNCH("idb_pair_knn_radii(merge)");
    return IDB_OK;
}

extern "C" int idb_pair_prdc_counts(const float* real, int32_t nr, const float* gen, int32_t ng, int32_t d, const float* shift,
                                    const float* r2_real, const float* r2_gen, int32_t* in_real_sphere, int32_t* covered, float* row_min,
                                    void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(pair_dims_ok(nr, ng, d), "idb_pair_prdc_counts: nr, ng in 1..%d and d in 1..%d", PAIR_MAX_N, PAIR_MAX_D);
    IDB_REQUIRE(real && gen && r2_real && r2_gen && in_real_sphere && covered && row_min && ws, "idb_pair_prdc_counts: null pointer");
    IDB_REQUIRE(ws_bytes >= pair_ws_bytes(IDB_PAIR_PRDC, nr, ng, 0) && idb_aligned16(ws), "idb_pair_prdc_counts: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    float* nra = (float*)ws;
    float* nrb = (float*)((char*)ws + align256(sizeof(float) * nr));
    int rc = pair_norms("idb_pair_prdc_counts", real, shift, nr, d, nra, st);
    if (rc == IDB_OK) rc = pair_norms("idb_pair_prdc_counts", gen, shift, ng, d, nrb, st);
    if (rc != IDB_OK) return rc;
    const int most = nr > ng ? nr : ng;
    hipLaunchKernelGGL(pair_prdc_init_kernel, dim3((most + 255) / 256), dim3(256), 0, st, in_real_sphere, ng, covered, (uint32_t*)row_min, nr);
    IDB_CHECK_LAUNCH("idb_pair_prdc_counts(init)");
    hipLaunchKernelGGL(pair_prdc_kernel, dim3(pair_blocks(ng), pair_blocks(nr)), dim3(256), 0, st, Operand{real, nullptr, nr},
                       Operand{gen, nullptr, ng}, shift, d, (int)pair_vec(d, real, gen, shift), (const float*)nra, (const float*)nrb, r2_real,
                       r2_gen, in_real_sphere, covered, (uint32_t*)row_min);
    IDB_CHECK_LAUNCH("idb_pair_prdc_counts");
    return IDB_OK;
}

extern "C" int idb_pair_nearest(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const float* shift, int32_t exclude_diag,
                                float* min_d2, int32_t* argmin, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(pair_dims_ok(na, nb, d), "idb_pair_nearest: na, nb in 1..%d and d in 1..%d", PAIR_MAX_N, PAIR_MAX_D);
    IDB_REQUIRE(!exclude_diag || na >= 2, "idb_pair_nearest: exclude_diag needs na >= 2");
    IDB_REQUIRE(a && b && min_d2 && argmin && ws, "idb_pair_nearest: null pointer");
    IDB_REQUIRE(ws_bytes >= pair_ws_bytes(IDB_PAIR_NEAREST, na, nb, 0) && idb_aligned16(ws), "idb_pair_nearest: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const int splits = pair_splits(na);
    const size_t part = align256(sizeof(float) * 2 * splits * (size_t)nb);
    char* p = (char*)ws;
    float* nra = (float*)p;
    p += align256(sizeof(float) * na);
    float* nrb = (float*)p;
    p += align256(sizeof(float) * nb);
    float* ws_min = (float*)p;
    int32_t* ws_idx = (int32_t*)(p + part);
    int rc = pair_norms("idb_pair_nearest", a, shift, na, d, nra, st);
    if (rc == IDB_OK) rc = pair_norms("idb_pair_nearest", b, shift, nb, d, nrb, st);
    if (rc != IDB_OK) return rc;
    hipLaunchKernelGGL(pair_nn_kernel, dim3(pair_blocks(nb), splits), dim3(256), 0, st, Operand{a, nullptr, na}, Operand{b, nullptr, nb}, shift, d,
                       (int)pair_vec(d, a, b, shift), (const float*)nra, (const float*)nrb, (int)(exclude_diag != 0), ws_min, ws_idx);
    IDB_CHECK_LAUNCH("idb_pair_nearest");
    hipLaunchKernelGGL(pair_nn_merge_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, (const float*)ws_min, (const int32_t*)ws_idx, 2 * splits,
                       nb, min_d2, argmin);
    IDB_CHECK_LAUNCH("idb_pair_nearest(merge)");
    return IDB_OK;
}

extern "C" int idb_pair_poly_sums(const float* x, int32_t nx, const float* y, int32_t ny, int32_t d, const int32_t* idx_x, const int32_t* idx_y,
                                  int32_t subsets, int32_t m, float gamma, float coef0, double* sums, void* ws, size_t ws_bytes, void* stream) {
    IDB_REQUIRE(pair_dims_ok(nx, ny, d), "idb_pair_poly_sums: nx, ny in 1..%d and d in 1..%d", PAIR_MAX_N, PAIR_MAX_D);
    IDB_REQUIRE(subsets > 0 && subsets <= 21845, "idb_pair_poly_sums: subsets in 1..21845");
    IDB_REQUIRE(m >= 2 && m <= nx && m <= ny, "idb_pair_poly_sums: subset size m in 2..min(nx, ny)");
    IDB_REQUIRE(x && y && idx_x && idx_y && sums && ws, "idb_pair_poly_sums: null pointer");
    IDB_REQUIRE(ws_bytes >= pair_ws_bytes(IDB_PAIR_POLY, m, m, subsets) && idb_aligned16(ws), "idb_pair_poly_sums: workspace too small or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = pair_blocks(m);
    hipLaunchKernelGGL(pair_poly_kernel, dim3(tiles, tiles, 3 * subsets), dim3(256), 0, st, x, y, idx_x, idx_y, m, d, (int)pair_vec(d, x, y, nullptr),
                       gamma, coef0, (float*)ws);
    IDB_CHECK_LAUNCH("idb_pair_poly_sums");
    hipLaunchKernelGGL(pair_poly_reduce_kernel, dim3((3 * subsets + 63) / 64), dim3(64), 0, st, (const float*)ws, 3 * subsets, tiles * tiles, sums);
    IDB_CHECK_LAUNCH("idb_pair_poly_sums(reduce)");
    return IDB_OK;
}
