// The tile helpers the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) kernels share: the accumulator's row map, the fixed-order double
// sums, and the 128-row LDS stage of idb_tail.hip and idb_block.hip.  idb_head.hip takes the row map and the sums, idb_pair.hip the
// row map alone.
#pragma once
#include "idb_common.h"

namespace {

constexpr int TM = 128;            // tile rows (4 x 32 per wave) and, at WN = 4, columns (4 waves x 32)
constexpr int TK = 32;             // reduction steps per LDS stage
constexpr int LDR = TK + 1;        // stride of an operand staged [row][k]: 33 r mod 64 is injective over a half-wave
constexpr int LDK = TM + 32;       // stride of an operand staged [k][row]: the two half-waves of a read hit disjoint banks

// the row of a 32x32 accumulator subtile t that register `reg` of half-wave h holds
__device__ __forceinline__ int tile_row(int t, int reg, int h) { return t * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order block sum of 256 threads: xor butterfly in the wave, then the four wave totals left to right; every thread gets it
__device__ __forceinline__ double block_sum_d(double v, double* lds4) {
    v = wave_sum_d(v);
    __syncthreads();                                   // lds4 may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// One LDS stage of 32 reduction steps on a 128-row tile of 32 WN columns.  WN = 4: wave w owns columns 32 w and all four 32-row
// subtiles; WN = 2: wave w owns columns 32 (w & 1) and the subtiles 2 (w >> 1), 2 (w >> 1) + 1.
// AR / BR: the operand is staged [row][k] (stride LDR), else [k][row] (stride LDK).
template <bool AR, bool BR, int WN>
__device__ __forceinline__ void mma_stage(const float* sA, const float* sB, f32x16 (&acc)[WN]) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5, wc = w % WN, wr = (w / WN) * WN;
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) {               // A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
        const float bv = BR ? sB[(wc * 32 + r) * LDR + kk + h] : sB[(kk + h) * LDK + wc * 32 + r];
#pragma unroll
        for (int t = 0; t < WN; ++t) {
            const float av = AR ? sA[((wr + t) * 32 + r) * LDR + kk + h] : sA[(kk + h) * LDK + (wr + t) * 32 + r];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
    }
}

// [row][k] staging: thread t holds columns 4 (t & 7) .. + 3 of rows (t >> 3) + 32 i, i < NI
template <int NI>
__device__ __forceinline__ void stash_rows(float* lds, const f32x4 (&v)[4]) {
    const int c = (threadIdx.x & 7) * 4, r = threadIdx.x >> 3;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[(r + 32 * i) * LDR + c + e] = v[i][e];
}
// [k][row] staging: thread t holds columns 4 (t & 31) .. + 3 of reduction rows (t >> 5) + 8 i
__device__ __forceinline__ void stash_cols(float* lds, const f32x4 (&v)[4]) {
    const int c = (threadIdx.x & 31) * 4, r = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4*)(lds + (r + 8 * i) * LDK + c) = v[i];
}

template <int WN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[WN]) {
#pragma unroll
    for (int t = 0; t < WN; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
}

// workspace sections start on 256 bytes
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
