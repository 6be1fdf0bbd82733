// Training attention for head_dim 64 on gfx950 MFMA: the forward that also saves the row statistic, and the flash-style backward.
//
// Replaces what autograd does behind F.scaled_dot_product_attention in the LoRA fine-tuning of the reference (train_ID-Booth.py: the
// adapters sit on to_q / to_k / to_v / to_out.0 of every UNet attention module, so every trainable parameter lies behind this kernel).
//
//   forward   idb_attention's 4-wave structure (S^T = K Q^T with the query on the lane, O^T = V^T P^T with the S accumulator as the
//             B operand) plus lse[b][h][q] = ln sum_j exp(scale q.k_j) = scale m + ln l.
//   backward  P is recomputed from lse: P = exp(scale S - lse), dP = dO V^T, dS = P o (dP - delta), delta = rowsum(dO o O).
//             -lse / scale and -delta are the INITIAL ACCUMULATORS of the S and dP chains, so p = exp2(scale log2e S') needs no
//             subtraction and no row maximum, and dS = p dP' is one multiply.
//     attn_bwd_delta   delta, fp32, once for both kernels below (workspace).
//     attn_bwd_dkv     owns key blocks: 4 waves x 32 keys; the KEY sits on the MFMA lane (S = Q K^T with Q rows from LDS as A and the
//                      wave's K rows, held in registers for the whole sweep, as B), so the S and dP accumulators, converted to 16
//                      bits, are directly the B operands of dV^T += dO^T P and dK^T += Q^T dS; the A operands dO^T / Q^T come from
//                      the SAME row-major LDS image the row reads use, through ds_read_b64_tr_b16.  dK and dV need no sum across
//                      workgroups unless the query range is cut into chunks (form 1, below).
//     attn_bwd_dq      owns query blocks and recomputes S and dP with the QUERY on the lane (the forward's orientation):
//                      dQ^T += K^T dS^T takes the dS^T accumulator as its B operand and K^T from the K tile by transposed reads.
//                      Seven products instead of five, and in exchange no sum of dQ across workgroups exists: no float atomics, no
//                      workgroup waits for another, no N/128 fp32 copies of dQ (335 MB at 4096 tokens, 5 heads, batch 2).
//     form 1           when the key blocks x heads x batch fill less than half the chip (cross-attention: ONE key block), the query
//                      range of attn_bwd_dkv is cut into chunks; each writes fp32 dK / dV slabs [chunk][b][h][n_kv][64] and
//                      attn_bwd_merge sums them in ascending chunk order (the slabs are n_kv rows: small exactly where this form runs).
// Every result is a fixed-order fp32 sum rounded once: bit-identical from run to run.
// LDS rows are 144 bytes (128 + one 16-byte access): conflict-free for the ds_read_b128 row reads, 2-way for the transposed reads.
#include "idb_common.h"
#include <math.h>

namespace {

constexpr int RS = 144;                 // LDS row stride of every [rows][64 x 16-bit] tile image
constexpr int KV_TILE = 64;             // keys per K/V tile of the query-owning kernels
constexpr int KV_BYTES = KV_TILE * RS;
constexpr int KEY_BLOCK = IDB_ATTN_BWD_KEY_BLOCK, SLICE = IDB_ATTN_BWD_SLICE, Q_BLOCK = 128;
constexpr float LOG2E = 1.44269504088896340736f;
constexpr float MASKED = -1e30f;        // initial accumulator of a query row past n_q: exp2 of it is exactly 0

template <typename T> using V8t = typename Op<T>::v8;
template <typename T> using V4t = typename Op<T>::v4;

// A^T fragment of a 32x32x16 product from a row-major [k][64] LDS image (stride RS): rows row0 .. row0+15 are the 16 k of the step,
// in the order the accumulator-as-operand imposes (element j of lane half h: k = 8 (j >> 2) + 4 h + (j & 3)); lane r gets column
// col0 + r.  The addressing of idb_attention's V^T fragments.
template <typename T>
__device__ __forceinline__ V8t<T> tr_frag(const char* img, int row0, int col0, int lane) {
    const int h = lane >> 5;
    const int tr_row = 4 * h + ((lane & 15) >> 2);
    const int tr_col = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const char* a = img + (row0 + tr_row) * RS + (col0 + tr_col) * 2;
    const V4t<T> lo = Op<T>::ds_read_tr(a);
    const V4t<T> hi = Op<T>::ds_read_tr(a + 8 * RS);
    V8t<T> f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[j] = lo[j];
        f[j + 4] = hi[j];
    }
    return f;
}

// row fragment (A operand, natural k order): lane (r, h) holds img[row0 + r][16 s + 8 h .. + 7]
template <typename T>
__device__ __forceinline__ V8t<T> row_frag(const char* img, int row0, int s, int lane) {
    return *(const V8t<T>*)(img + (row0 + (lane & 31)) * RS + (2 * s + (lane >> 5)) * 16);
}

__device__ __forceinline__ f32x16 splat16(float v) {
    f32x16 a;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = v;
    return a;
}

// ---- K/V tile staging of the query-owning kernels: 256 threads, 64 rows x 8 chunks of 16 bytes, two per thread and matrix; rows past
// n_kv - 1 repeat row n_kv - 1 (finite, masked later): the padding rows n_kv .. n_kv_alloc - 1 are never read
template <typename T>
struct KvStage {
    V8t<T> kreg[2], vreg[2];
    __device__ __forceinline__ void load(const T* kbase, const T* vbase, int kv_ld, int t, int n_kv, int tid) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = min(t * KV_TILE + (tid >> 3) + 32 * i, n_kv - 1);
            const long long o = (long long)row * kv_ld + (tid & 7) * 8;
            kreg[i] = *(const V8t<T>*)(kbase + o);
            vreg[i] = *(const V8t<T>*)(vbase + o);
        }
    }
    __device__ __forceinline__ void store(char* buf, int tid) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int o = ((tid >> 3) + 32 * i) * RS + (tid & 7) * 16;
            *(V8t<T>*)(buf + o) = kreg[i];
            *(V8t<T>*)(buf + KV_BYTES + o) = vreg[i];
        }
    }
};

// ---- forward with lse: one workgroup = 4 waves = 128 query rows of one (batch, head)
template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_train_kernel(const T* __restrict__ q, int q_ld, const T* __restrict__ k,
                                                            const T* __restrict__ v, int kv_ld, T* __restrict__ out, int out_ld,
                                                            float* __restrict__ lse, int n_q, int n_kv, int n_kv_alloc, float scale) {
    using V8 = V8t<T>;
    using V4 = V4t<T>;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * KV_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int q0 = blockIdx.x * Q_BLOCK + wave * 32;
    const float sl2 = scale * LOG2E;

    V8 qf[4];
    {
        const T* qp = q + ((long long)b * n_q + min(q0 + r, n_q - 1)) * q_ld + head * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const V8*)(qp + 16 * s);
    }
    const T* kbase = k + (long long)b * n_kv_alloc * kv_ld + head * 64;
    const T* vbase = v + (long long)b * n_kv_alloc * kv_ld + head * 64;
    const int ntiles = (n_kv + KV_TILE - 1) / KV_TILE;

    f32x16 oacc[2] = {splat16(0.f), splat16(0.f)};
    float m_run = -INFINITY, l_run = 0.f;
    KvStage<T> st;
    st.load(kbase, vbase, kv_ld, 0, n_kv, tid);
    st.store(smem, tid);
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) st.load(kbase, vbase, kv_ld, t + 1, n_kv, tid);
        const char* kt = smem + cur * 2 * KV_BYTES;
        const char* vt = kt + KV_BYTES;
        f32x16 sacc[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            sacc[kb] = splat16(0.f);
#pragma unroll
            for (int s = 0; s < 4; ++s) sacc[kb] = Op<T>::mfma32(row_frag<T>(kt, kb * 32, s, lane), qf[s], sacc[kb]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = t * KV_TILE + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (key >= n_kv) sacc[kb][i] = -INFINITY;
                mx = fmaxf(mx, sacc[kb][i]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);          // finite from tile 0 on: every tile holds at least one key below n_kv
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sl2);
        m_run = m_new;
        const float mb = m_new * sl2;
        float rs = 0.f;
        V8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][8 * s2 + j], sl2, -mb));
                    rs += pv;
                    pf[kb][s2][j] = from_f32<T>(pv);
                }
        l_run = l_run * alpha + rs;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[d][i] *= alpha;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int d = 0; d < 2; ++d) oacc[d] = Op<T>::mfma32(tr_frag<T>(vt, kb * 32 + 16 * s2, d * 32, lane), pf[kb][s2], oacc[d]);
        if (t + 1 < ntiles) st.store(smem + (cur ^ 1) * 2 * KV_BYTES, tid);
        __syncthreads();
    }
    // lane (q = r, half h) holds O[q][32 d + 8 (i >> 2) + 4 h + (i & 3)] and half of the row sum
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q0 + r < n_q) {
        T* op = out + ((long long)b * n_q + q0 + r) * out_ld + head * 64 + 4 * h;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                V4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = from_f32<T>(oacc[d][4 * g4 + e] * inv);
                *(V4*)(op + d * 32 + 8 * g4) = pk;
            }
        if (h == 0) lse[((long long)b * heads + head) * n_q + q0 + r] = __builtin_fmaf(m_run, scale, logf(l_tot));
    }
}

// ---- delta[b][h][q] = sum_d dout o out in fp32: 8 lanes per (row, head), 8 elements each, then the fixed 3-step exchange
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(const T* __restrict__ out, int out_ld, const T* __restrict__ dout, int dout_ld,
                                                            float* __restrict__ delta, int heads, int n_q, long long items) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;       // items is a multiple of 8: a group of 8 lanes is whole
    const long long it = g < items ? g : items - 8 + (g & 7);
    const int ch = (int)(it & 7);
    const long long rowhead = it >> 3;
    const int head = (int)(rowhead % heads);
    const long long row = rowhead / heads;                               // b * n_q + q
    const V8t<T> o = *(const V8t<T>*)(out + row * out_ld + head * 64 + ch * 8);
    const V8t<T> d = *(const V8t<T>*)(dout + row * dout_ld + head * 64 + ch * 8);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s = __builtin_fmaf(to_f32<T>(d[j]), to_f32<T>(o[j]), s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (g < items && ch == 0) {
        const long long b = row / n_q, qi = row % n_q;
        delta[(b * heads + head) * n_q + qi] = s;
    }
}

// ---- dK, dV: one workgroup = 4 waves = 128 keys of one (batch, head) and one chunk of the query range; wave w owns keys 32 w .. + 31
template <typename T, bool SLAB>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const T* __restrict__ q, int q_ld, const T* __restrict__ k, const T* __restrict__ v,
                                                          int kv_ld, const T* __restrict__ dout, int dout_ld, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, T* __restrict__ dk, T* __restrict__ dv, int dkv_ld,
                                                          float* __restrict__ slabs, int heads, int n_q, int n_kv, int n_kv_alloc,
                                                          int chunk_rows, float scale) {
    using V8 = V8t<T>;
    using V4 = V4t<T>;
    constexpr int TILE = SLICE * RS;                       // one 32-row image
    constexpr int BUF = 2 * TILE + 2 * SLICE * 4;          // Q image, dO image, -lse / scale, -delta
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int bh = blockIdx.z, b = bh / heads, head = bh - b * heads;
    const int chunk = blockIdx.y;
    const int key = blockIdx.x * KEY_BLOCK + wave * 32 + r;
    const bool valid = key < n_kv;
    const float sl2 = scale * LOG2E, inv_scale = 1.0f / scale;
    const int q_begin = chunk * chunk_rows, q_end = min(q_begin + chunk_rows, n_q);
    const int nslices = (q_end - q_begin + SLICE - 1) / SLICE;

    // the wave's K and V rows as B operands: lane (r, h) holds K[key][16 s + 8 h .. + 7]
    V8 kf[4], vf[4];
    {
        const long long o = ((long long)b * n_kv_alloc + min(key, n_kv - 1)) * kv_ld + head * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            kf[s] = *(const V8*)(k + o + 16 * s);
            vf[s] = *(const V8*)(v + o + 16 * s);
        }
    }
    const T* qbase = q + (long long)b * n_q * q_ld + head * 64;
    const T* dobase = dout + (long long)b * n_q * dout_ld + head * 64;
    const float* lbase = lse + ((long long)b * heads + head) * n_q;
    const float* dbase = delta + ((long long)b * heads + head) * n_q;

    // staging: thread = 16-byte chunk (tid & 7) of row (tid >> 3) of the Q and dO slices; rows past the chunk's end are zero and their
    // -lse is MASKED, so they add exactly 0 to both gradients
    V8 qreg, doreg;
    float lreg = 0.f, dreg = 0.f;
    auto gload = [&](int t) {
        const int row = q_begin + t * SLICE + (tid >> 3);
        V8 z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = from_f32<T>(0.f);
        qreg = z;
        doreg = z;
        if (row < q_end) {
            qreg = *(const V8*)(qbase + (long long)row * q_ld + (tid & 7) * 8);
            doreg = *(const V8*)(dobase + (long long)row * dout_ld + (tid & 7) * 8);
        }
        if (tid < SLICE) {
            const int rl = q_begin + t * SLICE + tid;
            lreg = rl < q_end ? -lbase[rl] * inv_scale : MASKED;
            dreg = rl < q_end ? -dbase[rl] : 0.f;
        }
    };
    auto lstore = [&](int buf) {
        char* p = smem + buf * BUF;
        const int o = (tid >> 3) * RS + (tid & 7) * 16;
        *(V8*)(p + o) = qreg;
        *(V8*)(p + TILE + o) = doreg;
        if (tid < SLICE) {
            ((float*)(p + 2 * TILE))[tid] = lreg;
            ((float*)(p + 2 * TILE))[SLICE + tid] = dreg;
        }
    };

    f32x16 dkacc[2] = {splat16(0.f), splat16(0.f)}, dvacc[2] = {splat16(0.f), splat16(0.f)};
    gload(0);
    lstore(0);
    __syncthreads();
    for (int t = 0; t < nslices; ++t) {
        const int cur = t & 1;
        if (t + 1 < nslices) gload(t + 1);
        const char* qt = smem + cur * BUF;
        const char* dot = qt + TILE;
        const float* nl = (const float*)(qt + 2 * TILE);
        const float* nd = nl + SLICE;
        // S'[q][key] = Q K^T - lse / scale and dP'[q][key] = dO V^T - delta: key = the lane's column, q = 8 g + 4 h + e in register 4 g + e
        f32x16 sacc, pacc;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 l4 = *(const f32x4*)(nl + 8 * g4 + 4 * h);
            const f32x4 d4 = *(const f32x4*)(nd + 8 * g4 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sacc[4 * g4 + e] = l4[e];
                pacc[4 * g4 + e] = d4[e];
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sacc = Op<T>::mfma32(row_frag<T>(qt, 0, s, lane), kf[s], sacc);
            pacc = Op<T>::mfma32(row_frag<T>(dot, 0, s, lane), vf[s], pacc);
        }
        V8 pf[2], dsf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = valid ? __builtin_amdgcn_exp2f(sacc[8 * s2 + j] * sl2) : 0.f;
                pf[s2][j] = from_f32<T>(p);
                dsf[s2][j] = from_f32<T>(p * pacc[8 * s2 + j]);
            }
        // dV^T[d][key] += dO^T P and dK^T[d][key] += Q^T dS: the slice's query rows are the k of the product
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                dvacc[d] = Op<T>::mfma32(tr_frag<T>(dot, 16 * s2, d * 32, lane), pf[s2], dvacc[d]);
                dkacc[d] = Op<T>::mfma32(tr_frag<T>(qt, 16 * s2, d * 32, lane), dsf[s2], dkacc[d]);
            }
        if (t + 1 < nslices) lstore(cur ^ 1);
        __syncthreads();
    }
    // lane (key, half h) holds dX[key][32 d + 8 g + 4 h + e] in register 4 g + e of dXacc[d]
    if (!valid) return;
    if constexpr (SLAB) {
        const long long rows = (long long)gridDim.z * n_kv;                          // slab = [chunk][b][h][n_kv][64] fp32, dK then dV
        float* sk = slabs + (((long long)chunk * gridDim.z + bh) * n_kv + key) * 64 + 4 * h;
        float* sv = sk + (long long)gridDim.y * rows * 64;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 a, c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = dkacc[d][4 * g4 + e];
                    c[e] = dvacc[d][4 * g4 + e];
                }
                *(f32x4*)(sk + d * 32 + 8 * g4) = a;
                *(f32x4*)(sv + d * 32 + 8 * g4) = c;
            }
    } else {
        const long long o = ((long long)b * n_kv_alloc + key) * dkv_ld + head * 64 + 4 * h;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                V4 a, c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = from_f32<T>(dkacc[d][4 * g4 + e] * scale);
                    c[e] = from_f32<T>(dvacc[d][4 * g4 + e]);
                }
                *(V4*)(dk + o + d * 32 + 8 * g4) = a;
                *(V4*)(dv + o + d * 32 + 8 * g4) = c;
            }
    }
}

// ---- form 1: dK = scale * (slab 0 + slab 1 + ...), dV likewise without the scale, ascending chunk order, one rounding to T
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_merge_kernel(const float* __restrict__ slabs, int chunks, T* __restrict__ dk, T* __restrict__ dv,
                                                            int dkv_ld, int heads, int n_kv, int n_kv_alloc, long long items, float scale) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;      // item = 4 columns of one (b, h, key) row
    if (it >= items) return;
    const int c4 = (int)(it & 15);
    const long long row = it >> 4;                                       // (b * heads + h) * n_kv + key
    const int key = (int)(row % n_kv);
    const long long bh = row / n_kv;
    const int head = (int)(bh % heads);
    const long long b = bh / heads;
    const long long slab = (items >> 4) * 64;                            // floats per chunk
    const float* pk = slabs + row * 64 + c4 * 4;
    const float* pv = pk + (long long)chunks * slab;
    f32x4 sk = *(const f32x4*)pk, sv = *(const f32x4*)pv;
    for (int c = 1; c < chunks; ++c) {
        sk += *(const f32x4*)(pk + c * slab);
        sv += *(const f32x4*)(pv + c * slab);
    }
    V4t<T> a, c;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] = from_f32<T>(sk[e] * scale);
        c[e] = from_f32<T>(sv[e]);
    }
    const long long o = (b * n_kv_alloc + key) * dkv_ld + head * 64 + c4 * 4;
    *(V4t<T>*)(dk + o) = a;
    *(V4t<T>*)(dv + o) = c;
}

// ---- dQ: one workgroup = 4 waves = 128 query rows of one (batch, head); the query on the lane, as in the forward
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const T* __restrict__ q, int q_ld, const T* __restrict__ k, const T* __restrict__ v,
                                                         int kv_ld, const T* __restrict__ dout, int dout_ld, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, T* __restrict__ dq, int dq_ld, int n_q, int n_kv,
                                                         int n_kv_alloc, float scale) {
    using V8 = V8t<T>;
    using V4 = V4t<T>;
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * KV_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
    const int q0 = blockIdx.x * Q_BLOCK + wave * 32;
    const int qr = min(q0 + r, n_q - 1);
    const float sl2 = scale * LOG2E;

    V8 qf[4], dof[4];
    {
        const T* qp = q + ((long long)b * n_q + qr) * q_ld + head * 64 + 8 * h;
        const T* dp = dout + ((long long)b * n_q + qr) * dout_ld + head * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qf[s] = *(const V8*)(qp + 16 * s);
            dof[s] = *(const V8*)(dp + 16 * s);
        }
    }
    const float nl = -lse[((long long)b * heads + head) * n_q + qr] / scale;
    const float nd = -delta[((long long)b * heads + head) * n_q + qr];
    const T* kbase = k + (long long)b * n_kv_alloc * kv_ld + head * 64;
    const T* vbase = v + (long long)b * n_kv_alloc * kv_ld + head * 64;
    const int ntiles = (n_kv + KV_TILE - 1) / KV_TILE;

    f32x16 qacc[2] = {splat16(0.f), splat16(0.f)};
    KvStage<T> st;
    st.load(kbase, vbase, kv_ld, 0, n_kv, tid);
    st.store(smem, tid);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) st.load(kbase, vbase, kv_ld, t + 1, n_kv, tid);
        const char* kt = smem + cur * 2 * KV_BYTES;
        const char* vt = kt + KV_BYTES;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            // S'^T[key][q] = K Q^T - lse / scale, dP'^T[key][q] = V dO^T - delta: q = the lane's column, key = 8 g + 4 h + e in register 4 g + e
            f32x16 sacc = splat16(nl), pacc = splat16(nd);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                sacc = Op<T>::mfma32(row_frag<T>(kt, kb * 32, s, lane), qf[s], sacc);
                pacc = Op<T>::mfma32(row_frag<T>(vt, kb * 32, s, lane), dof[s], pacc);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                V8 dsf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = 8 * s2 + j;
                    const int key = t * KV_TILE + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    const float p = key < n_kv ? __builtin_amdgcn_exp2f(sacc[i] * sl2) : 0.f;
                    dsf[j] = from_f32<T>(p * pacc[i]);
                }
                // dQ^T[d][q] += K^T dS^T
#pragma unroll
                for (int d = 0; d < 2; ++d) qacc[d] = Op<T>::mfma32(tr_frag<T>(kt, kb * 32 + 16 * s2, d * 32, lane), dsf, qacc[d]);
            }
        }
        if (t + 1 < ntiles) st.store(smem + (cur ^ 1) * 2 * KV_BYTES, tid);
        __syncthreads();
    }
    if (q0 + r < n_q) {
        T* op = dq + ((long long)b * n_q + q0 + r) * dq_ld + head * 64 + 4 * h;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                V4 pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk[e] = from_f32<T>(qacc[d][4 * g4 + e] * scale);
                *(V4*)(op + d * 32 + 8 * g4) = pk;
            }
    }
}

// The decision both idb_attention_bwd and idb_attention_bwd_plan read.
struct BwdPlan {
    int form, key_blocks, chunks, chunk_rows, launches;
    size_t delta_bytes, slab_bytes;
};

BwdPlan bwd_plan(int batch, int heads, int n_q, int n_kv) {
    BwdPlan p;
    p.key_blocks = (n_kv + KEY_BLOCK - 1) / KEY_BLOCK;
    const long long wgs = (long long)p.key_blocks * heads * batch;
    // the key-owning grid alone fills at least half of the 256 CUs, or one chunk would hold the whole query range anyway: no chunks
    int chunks = 1;
    if (wgs < IDB_ATTN_BWD_FULL_GRID && n_q > 2 * SLICE) {
        const long long want = (256 + wgs - 1) / wgs, most = (n_q + 2 * SLICE - 1) / (2 * SLICE);      // at least two slices per chunk
        chunks = (int)(want < most ? want : most);
    }
    p.chunk_rows = ((n_q + chunks - 1) / chunks + SLICE - 1) / SLICE * SLICE;
    p.chunks = (n_q + p.chunk_rows - 1) / p.chunk_rows;
    p.form = p.chunks > 1 ? 1 : 0;
    p.launches = p.form ? 4 : 3;
    p.delta_bytes = ((size_t)batch * heads * n_q * 4 + 255) / 256 * 256;
    p.slab_bytes = p.form ? (size_t)2 * p.chunks * batch * heads * n_kv * 64 * 4 : 0;
    return p;
}

struct Span {
    const char* name;
    const char* p;
    long long bytes;
};
bool overlaps(const Span& a, const Span& b) { return a.p < b.p + b.bytes && b.p < a.p + a.bytes; }

int check_dims(const char* api, int batch, int heads, int n_q, int n_kv) {
    IDB_REQUIRE(batch > 0 && heads > 0 && n_q > 0 && n_kv > 0, "%s: bad dims (batch, heads, n_q, n_kv must be positive)", api);
    IDB_REQUIRE(heads <= 65535 && (long long)batch * heads <= 65535, "%s: batch * heads too large for the grid", api);
    IDB_REQUIRE((long long)batch * heads * n_q < (1ll << 31) && (long long)batch * heads * n_kv < (1ll << 31), "%s: batch * heads * n too large", api);
    return IDB_OK;
}

#define IDB_REQUIRE_LD(api, name, ld, heads)                                                                                       \
    IDB_REQUIRE((ld) >= (heads) * 64 && (ld) % 8 == 0, "%s: %s must be at least heads*64 and a multiple of 8 elements (16 bytes)", \
                api, name)

}  // namespace

extern "C" size_t idb_attention_bwd_workspace_bytes(int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv) {
    if (check_dims("idb_attention_bwd_workspace_bytes", batch, heads, n_q, n_kv) != IDB_OK) return 0;
    const BwdPlan p = bwd_plan(batch, heads, n_q, n_kv);
    return p.delta_bytes + p.slab_bytes;
}

extern "C" int idb_attention_bwd_plan(int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t* form, int32_t* key_block,
                                      int32_t* query_rows, int32_t* launches) {
    IDB_REQUIRE(form && key_block && query_rows && launches, "idb_attention_bwd_plan: null pointer");
    if (int rc = check_dims("idb_attention_bwd_plan", batch, heads, n_q, n_kv)) return rc;
    const BwdPlan p = bwd_plan(batch, heads, n_q, n_kv);
    *form = p.form;
    *key_block = KEY_BLOCK;
    *query_rows = p.chunk_rows;
    *launches = p.launches;
    return IDB_OK;
}

extern "C" int idb_attention_fwd_train(const void* q, int32_t q_ld, const void* k, const void* v, int32_t kv_ld, void* out, int32_t out_ld,
                                       float* lse, int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t n_kv_alloc, float scale,
                                       int32_t dtype, void* stream) {
    const char* api = "idb_attention_fwd_train";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be bf16/f16", api);
        return IDB_EUNSUPPORTED;
    }
    IDB_REQUIRE(q, "%s: q is null", api);
    IDB_REQUIRE(k, "%s: k is null", api);
    IDB_REQUIRE(v, "%s: v is null", api);
    IDB_REQUIRE(out, "%s: out is null", api);
    IDB_REQUIRE(lse, "%s: lse is null", api);
    IDB_REQUIRE(idb_aligned16(q) && idb_aligned16(k) && idb_aligned16(v) && idb_aligned16(out), "%s: unaligned pointer (q, k, v, out: 16 bytes)", api);
    if (int rc = check_dims(api, batch, heads, n_q, n_kv)) return rc;
    IDB_REQUIRE(n_kv_alloc >= n_kv, "%s: n_kv_alloc < n_kv", api);
    IDB_REQUIRE_LD(api, "q_ld", q_ld, heads);
    IDB_REQUIRE_LD(api, "kv_ld", kv_ld, heads);
    IDB_REQUIRE_LD(api, "out_ld", out_ld, heads);
    IDB_REQUIRE(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite", api);
    const dim3 grid((n_q + Q_BLOCK - 1) / Q_BLOCK, heads, batch);
    IDB_REQUIRE(batch <= 65535, "%s: batch too large for the grid", api);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        hipLaunchKernelGGL(attn_fwd_train_kernel<__bf16>, grid, dim3(256), 0, st, (const __bf16*)q, q_ld, (const __bf16*)k, (const __bf16*)v, kv_ld,
                           (__bf16*)out, out_ld, lse, n_q, n_kv, n_kv_alloc, scale);
    else
        hipLaunchKernelGGL(attn_fwd_train_kernel<_Float16>, grid, dim3(256), 0, st, (const _Float16*)q, q_ld, (const _Float16*)k, (const _Float16*)v,
                           kv_ld, (_Float16*)out, out_ld, lse, n_q, n_kv, n_kv_alloc, scale);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

template <typename T>
static int bwd_launch(const BwdPlan& p, const void* q, int q_ld, const void* k, const void* v, int kv_ld, const void* out, int out_ld,
                      const void* dout, int dout_ld, const float* lse, void* dq, int dq_ld, void* dk, void* dv, int dkv_ld, void* workspace,
                      int batch, int heads, int n_q, int n_kv, int n_kv_alloc, float scale, hipStream_t st) {
    const char* api = "idb_attention_bwd";
    float* delta = (float*)workspace;
    float* slabs = (float*)((char*)workspace + p.delta_bytes);
    const long long ditems = (long long)batch * n_q * heads * 8;
    hipLaunchKernelGGL(attn_bwd_delta_kernel<T>, dim3((unsigned)((ditems + 255) / 256)), dim3(256), 0, st, (const T*)out, out_ld, (const T*)dout,
                       dout_ld, delta, heads, n_q, ditems);
    IDB_CHECK_LAUNCH(api);
    const dim3 kgrid(p.key_blocks, p.chunks, batch * heads);
    if (p.form) {
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, true>), kgrid, dim3(256), 0, st, (const T*)q, q_ld, (const T*)k, (const T*)v, kv_ld, (const T*)dout,
                           dout_ld, lse, delta, (T*)dk, (T*)dv, dkv_ld, slabs, heads, n_q, n_kv, n_kv_alloc, p.chunk_rows, scale);
        IDB_CHECK_LAUNCH(api);
        const long long items = (long long)batch * heads * n_kv * 16;
        hipLaunchKernelGGL(attn_bwd_merge_kernel<T>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, slabs, p.chunks, (T*)dk, (T*)dv, dkv_ld,
                           heads, n_kv, n_kv_alloc, items, scale);
        IDB_CHECK_LAUNCH(api);
    } else {
        hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, false>), kgrid, dim3(256), 0, st, (const T*)q, q_ld, (const T*)k, (const T*)v, kv_ld, (const T*)dout,
                           dout_ld, lse, delta, (T*)dk, (T*)dv, dkv_ld, slabs, heads, n_q, n_kv, n_kv_alloc, p.chunk_rows, scale);
        IDB_CHECK_LAUNCH(api);
    }
    hipLaunchKernelGGL(attn_bwd_dq_kernel<T>, dim3((n_q + Q_BLOCK - 1) / Q_BLOCK, heads, batch), dim3(256), 0, st, (const T*)q, q_ld, (const T*)k,
                       (const T*)v, kv_ld, (const T*)dout, dout_ld, lse, delta, (T*)dq, dq_ld, n_q, n_kv, n_kv_alloc, scale);
    IDB_CHECK_LAUNCH(api);
    return IDB_OK;
}

extern "C" int idb_attention_bwd(const void* q, int32_t q_ld, const void* k, const void* v, int32_t kv_ld, const void* out, int32_t out_ld,
                                 const void* dout, int32_t dout_ld, const float* lse, void* dq, int32_t dq_ld, void* dk, void* dv, int32_t dkv_ld,
                                 void* workspace, size_t workspace_bytes, int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv,
                                 int32_t n_kv_alloc, float scale, int32_t dtype, void* stream) {
    const char* api = "idb_attention_bwd";
    if (!idb_is_operand_dtype(dtype)) {
        idb_set_error("%s: dtype must be bf16/f16", api);
        return IDB_EUNSUPPORTED;
    }
    const void* ptrs[] = {q, k, v, out, dout, lse, dq, dk, dv, workspace};
    const char* names[] = {"q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "workspace"};
    for (int i = 0; i < 10; ++i) {
        IDB_REQUIRE(ptrs[i], "%s: %s is null", api, names[i]);
        IDB_REQUIRE(i == 5 ? ((uintptr_t)ptrs[i] & 3) == 0 : idb_aligned16(ptrs[i]), "%s: %s is not aligned (16 bytes; lse 4)", api, names[i]);
    }
    if (int rc = check_dims(api, batch, heads, n_q, n_kv)) return rc;
    IDB_REQUIRE(batch <= 65535, "%s: batch too large for the grid", api);
    IDB_REQUIRE(n_kv_alloc >= n_kv, "%s: n_kv_alloc < n_kv", api);
    IDB_REQUIRE_LD(api, "q_ld", q_ld, heads);
    IDB_REQUIRE_LD(api, "kv_ld", kv_ld, heads);
    IDB_REQUIRE_LD(api, "out_ld", out_ld, heads);
    IDB_REQUIRE_LD(api, "dout_ld", dout_ld, heads);
    IDB_REQUIRE_LD(api, "dq_ld", dq_ld, heads);
    IDB_REQUIRE_LD(api, "dkv_ld", dkv_ld, heads);
    IDB_REQUIRE(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite", api);
    const BwdPlan p = bwd_plan(batch, heads, n_q, n_kv);
    IDB_REQUIRE(workspace_bytes >= p.delta_bytes + p.slab_bytes, "%s: workspace_bytes %zu < %zu (idb_attention_bwd_workspace_bytes)", api,
                workspace_bytes, p.delta_bytes + p.slab_bytes);
    // a gradient may share a packed buffer with the other gradients (interleaved columns), never a byte range with an input
    auto rows_bytes = [&](long long rows, int ld) { return ((rows - 1) * ld + heads * 64) * 2; };
    const long long nq_rows = (long long)batch * n_q, nkv_rows = (long long)batch * n_kv_alloc;
    const Span in[] = {{"q", (const char*)q, rows_bytes(nq_rows, q_ld)},          {"k", (const char*)k, rows_bytes(nkv_rows, kv_ld)},
                       {"v", (const char*)v, rows_bytes(nkv_rows, kv_ld)},        {"out", (const char*)out, rows_bytes(nq_rows, out_ld)},
                       {"dout", (const char*)dout, rows_bytes(nq_rows, dout_ld)}, {"lse", (const char*)lse, (long long)batch * heads * n_q * 4},
                       {"workspace", (const char*)workspace, (long long)(p.delta_bytes + p.slab_bytes)}};
    const Span outs[] = {{"dq", (const char*)dq, rows_bytes(nq_rows, dq_ld)},
                         {"dk", (const char*)dk, rows_bytes(nkv_rows, dkv_ld)},
                         {"dv", (const char*)dv, rows_bytes(nkv_rows, dkv_ld)}};
    for (const Span& o : outs)
        for (const Span& i : in) IDB_REQUIRE(!overlaps(o, i), "%s: %s aliases %s", api, o.name, i.name);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == IDB_BF16)
        return bwd_launch<__bf16>(p, q, q_ld, k, v, kv_ld, out, out_ld, dout, dout_ld, lse, dq, dq_ld, dk, dv, dkv_ld, workspace, batch, heads, n_q,
                                  n_kv, n_kv_alloc, scale, st);
    return bwd_launch<_Float16>(p, q, q_ld, k, v, kv_ld, out, out_ld, dout, dout_ld, lse, dq, dq_ld, dk, dv, dkv_ld, workspace, batch, heads, n_q, n_kv,
                                n_kv_alloc, scale, st);
}
