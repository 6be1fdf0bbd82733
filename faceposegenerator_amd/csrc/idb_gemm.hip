// K1/K2/K3 — implicit GEMM on MFMA for gfx950: conv3x3 (stride 1/2, nearest-2x upsample), 1x1 conv,
// Linear, with skip-concat / fused-shortcut K segments and bias / temb / residual / GEGLU epilogues.
//
// Upstream ops replaced (see include/idb_kernels.h): diffusers ResnetBlock2D.conv1/conv2/conv_shortcut,
// Downsample2D.conv, Upsample2D (interpolate + conv), Attention.to_q/k/v/to_out, FeedForward (GEGLU),
// Transformer2DModel.proj_in/proj_out — reached from /root/reference/inference_ID-Booth.py:138.
//
// Design (MI355X):
//   * NHWC activations: one K-step (64 channels of one tap) of an im2col row is ONE contiguous
//     128-byte line, so both operands stream HBM/L2 -> LDS with buffer_load_dwordx4 ... lds (LDS-DMA,
//     16 B/lane, no VGPR staging); zero padding = out-of-range buffer offsets (hardware zero fill).
//   * LDS tile rows are 128 B; chunk c of row r is stored at chunk position c ^ (r & 7) (swizzle
//     applied on the SOURCE address, LDS-DMA destinations are lane-linear) so every ds_read_b128
//     fragment read is bank-conflict free.
//   * v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulate.  The weight fragment is the MFMA A operand
//     and the activation fragment the B operand, so each lane ends up with 4 CONSECUTIVE output
//     channels of one pixel -> 8-byte (bf16) / 16-byte (fp32) epilogue accesses.
//   * LDS ring of 2 stages (two workgroups per CU hide each other's latency) or 3 stages (a lone
//     workgroup per CU: two K-steps in flight), 8 waves per workgroup by default, next stage's DMA
//     issued before the current stage's MFMAs, counted vmcnt, one barrier per K-step; XCD-aware
//     bijective block remaps (runs of tiles per XCD, or one K-slice per XCD for split-K grids).
//   * grids smaller than the chip (the whole batch-1 UNet) use split-K sized to one workgroup per
//     CU, fp32 slabs + a reduce/epilogue launch (deterministic, no atomics) that can also emit the
//     first GroupNorm pass of its output.
//   * the launch geometry is resolved on the host (idb_gemm_epi.h: GemmParams, idb_fill_geometry; idb_fastdiv.h): no kernel of the
//     ring / loader-wave / fused-GroupNorm / patch families divides by a run-time value in front of its first load — tile index,
//     K range of a split, K seek and row decode are multiply-highs by exact reciprocals or shifts, the patch conv's H / nimg / RI
//     and the GroupNorm's group width arrive as values (a batch-1 launch is ~14 us, and 7-12 division expansions stood on every
//     loader wave's path to its first LDS-DMA).  Quotients, and with them every address and K range, are what they were.
//   * kernel arguments are laid out by when they are needed (idb_gemm_epi.h: GemmTile, GemmHead): the launch scalars of the tile index,
//     the K range and the K seek's source are leading plain parameters, preloaded into SGPRs at wave launch (Makefile: KERNARG_PRELOAD);
//     the loader waves and the ring kernel fetch the head and the source record of their first K-step as three 16-dword scalar loads
//     behind ONE wait (a lone workgroup per CU stood through 6-7 dependent kernel-argument round trips before its first LDS-DMA).
#include "idb_common.h"
#include <stdlib.h>

#include "idb_gemm_epi.h"

// __launch_bounds__(256, 2): at most 256 VGPRs so that TWO workgroups share a CU — the second workgroup's MFMAs are what
// hides this one's LDS-DMA issue, waits and epilogue (one workgroup per CU measured 0.70 vs 1.12 PFLOP/s on the conv shape).
// idb_gemm_kernel and its ReLU twin (idb_gemm_desc.act = 3) share one body (idb_gemm_ring_body.inc); the epilogue activation is a
// compile-time parameter, so the kernels without it keep their code and register budgets.
template <typename T, int MF, int NF, int NS, int WM = 2>   // WM wave rows x 2 wave columns; tile = (16*MF*WM) x (32*NF)
__global__ __launch_bounds__(128 * WM, 2) void idb_gemm_kernel(IDB_TILE_PARAMS, const GemmParams p) {
    [[maybe_unused]] constexpr bool RELU = false;
    [[maybe_unused]] const GemmTile h = IDB_TILE_PACK;
#include "idb_gemm_ring_body.inc"
}

template <typename T, int MF, int NF, int NS, int WM = 2>
__global__ __launch_bounds__(128 * WM, 2) void idb_gemm_kernel_relu(IDB_TILE_PARAMS, const GemmParams p) {
    [[maybe_unused]] constexpr bool RELU = true;
    [[maybe_unused]] const GemmTile h = IDB_TILE_PACK;
#include "idb_gemm_ring_body.inc"
}


// ------------------------------------------------------------------------------------------------------------
// Loader-wave variant (round 3) for grids of at most ONE workgroup per CU (the whole batch-1 UNet).  In idb_gemm_kernel every
// wave issues its share of the next stage's LDS-DMA instructions and THEN reads fragments and issues MFMAs; with a lone
// workgroup per CU nothing hides the ~100 issue cycles of each DMA instruction (4-5 per wave and K-step) nor the counted wait in
// front of the barrier, and all eight waves go through those phases in lock step: a K-step takes 0.6-1.0 us against 0.13-0.27 us
// of MFMA time.  Here the workgroup has LW extra waves (one or two per SIMD) that do nothing but the address arithmetic, the
// DMA issue and the counted vmcnt wait; the 2*WM compute waves keep exactly the fragment mapping, accumulation order and epilogue
// of idb_gemm_kernel (results are bit-identical) but execute only barrier -> ds_read -> MFMA.  Both roles pass ONE s_barrier per
// K-step (no flags, no polling: every wave reaches the same nk barriers), the loaders leave after the loop — s_barrier counts only
// the surviving waves of a workgroup — and the compute waves run the shared epilogue among themselves.
//   prologue: the A half of stage 0 is requested first — K seek, row decode, first tap's offsets — and the weight descriptor, the weight
//   offsets and the grouped-weight arithmetic, which only the W half needs, behind it; the loads of a stage keep their order and count.
//   ring: NS stages; at the top of K-step `it` the loaders wait until stage `it` has landed (counted vmcnt: stages it+1 ..
//   it+NS-2 stay in flight), the barrier publishes it and proves stage it-1 is read, then they issue stage it+NS-1 into that buffer.
// ------------------------------------------------------------------------------------------------------------
template <typename T, int MF, int NF, int NS, int WM, int LW, bool RELU>
__device__ __forceinline__ void idb_gemm_kernel_lw_body(const GemmTile& h, const GemmParams& p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using V8 = typename Op<T>::v8;
    constexpr int BM = 16 * MF * WM, BN = 32 * NF;
    constexpr int CT = 128 * WM;                               // compute threads
    constexpr int LR = 8 * LW;                                 // tile rows per sweep of the loader waves
    constexpr int NA = BM / LR, NJ = (BN + LR - 1) / LR;       // sweeps per stage: A rows, weight rows (the last may be partial)
    static_assert(BM % LR == 0, "loader sweep must divide the row tile");
    constexpr int STAGE = (BM + NJ * LR) * 128;
    constexpr int LOADS = NA + NJ;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 2 * WM;                        // wave-uniform (readfirstlane): a scalar branch, not an EXEC mask

    int wg, kz, tm, tn;
    idb_wg_tile(h, wg, kz);
    idb_tile_mn(h, wg, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    int kt0, kt1;
    idb_k_range(h, kz, kt0, kt1);
    const int nk = kt1 - kt0;

    if (loader) {
        // ---------------- loader waves: addresses, LDS-DMA issue, counted waits ----------------
        const int lw = wave - 2 * WM;
        const int lt = tid - CT;                               // 0 .. 64*LW-1
        const int lrow = lt >> 3;                              // 0 .. LR-1
        const unsigned cg16 = ((lt & 7) ^ (lrow & 7)) * 16;    // swizzle on the source side (LR is a multiple of 8)
        // First DMA first: the A half of stage 0 is requested as soon as the K seek and the row decode allow; the weight offsets, the
        // weight descriptor and the grouped-weight arithmetic — which only the W half needs — come behind it.
        // The source of the first K-step comes out of GemmTile alone, so the head and that source's record are requested together and
        // waited for once (idb_loader_head); from here to the first DMA the loaders read `q` and `S`, not the kernel-argument segment.
        int s, rem, tap, c0, cur_c = 64, tap_end = 9;
        idb_k_seek_src(h, kt0, s, rem);
        GemmHead q;
        GemmSrcK S;
        idb_loader_head(p, s, q, S);
        idb_k_seek_tap(S, rem, tap, c0);
        int a_b[NA], a_oy[NA], a_ox[NA];
        bool a_ok[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + i * LR + lrow;
            a_ok[i] = m < q.M;
            idb_row_decode(q, a_ok[i] ? m : 0, a_b[i], a_oy[i], a_ox[i]);
        }
        __amdgpu_buffer_rsrc_t rs_a, rs_w;
        unsigned a_voff[NA], w_voff[NJ];
        unsigned w_soff = (unsigned)kt0 * q.w_kstep;
        bool need_retap = true;
        auto stage_a = [&](int buf) {
            char* sA = smem + buf * STAGE;
            if (need_retap) {
                rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
                cur_c = S.C;
                tap_end = S.taps == 9 ? 9 : 5;
                const int t3 = tap / 3;
                const int dy = t3 - q.pad, dx = tap - t3 * 3 - q.pad;
                const int LH = S.H << S.up, LWd = S.W << S.up;
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const int iy = a_oy[i] * q.stride + dy, ix = a_ox[i] * q.stride + dx;
                    const bool ok = a_ok[i] && (unsigned)iy < (unsigned)LH && (unsigned)ix < (unsigned)LWd;
                    const int pix = (a_b[i] * S.H + (iy >> S.up)) * S.W + (ix >> S.up);
                    a_voff[i] = ok ? (unsigned)pix * (unsigned)(S.C * 2) + cg16 : IDB_OOB;
                }
                need_retap = false;
            }
            const unsigned a_soff = (unsigned)c0 * 2u;
#pragma unroll
            for (int i = 0; i < NA; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, LDS_PTR(sA + (i * 64 * LW + lw * 64) * 16), 16, a_voff[i], a_soff, 0, 0);
        };
        auto stage_w = [&](int buf) {                          // the W half, and on to the next K-step
            char* sB = smem + buf * STAGE + BM * 128;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(sB + (j * 64 * LW + lw * 64) * 16), 16, w_voff[j], w_soff, 0, 0);
            w_soff += q.w_kstep;
            c0 += 64;
            if (c0 == cur_c) {
                c0 = 0;
                need_retap = true;
                if (++tap == tap_end) {
                    if (s < IDB_MAX_SRC - 1) S = p.src[++s];
                    tap = S.taps == 9 ? 0 : 4;
                }
            }
        };
        if (nk > 0) stage_a(0);
        rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)(q.w + idb_weight_group(q, m0) * q.w_group_stride), 0, q.w_bytes, IDB_RSRC_FLAGS);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = n0 + j * LR + lrow;
            w_voff[j] = (n < q.N && j * LR + lrow < BN) ? (unsigned)(n >> 4) * q.w_blk_bytes + (unsigned)(n & 15) * q.w_row_bytes + cg16 : IDB_OOB;
        }
        if (nk > 0) stage_w(0);
        auto stage = [&](int buf) {
            stage_a(buf);
            stage_w(buf);
        };
#pragma unroll
        for (int st = 1; st < NS - 1; ++st)
            if (st < nk) stage(st);
        int cur = 0;
        for (int it = 0; it < nk; ++it) {
            if (it + NS - 2 < nk)
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * LOADS) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            if (it + NS - 1 < nk) stage(cur == 0 ? NS - 1 : cur - 1);
            cur = cur + 1 == NS ? 0 : cur + 1;
        }
        return;                                                // s_barrier counts the surviving waves only
    }

    // ---------------- compute waves: the fragment mapping and the epilogue of idb_gemm_kernel ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float2 ln_part = make_float2(0.f, 0.f);
    if (p.ln_stats) ln_part = idb_ln_row_partials<BM, CT>(p, m0, tid);
    if constexpr (MF >= 2) {
        // The K-step is rotated by half a step around the barrier: the fragments of the stage's SECOND 32-deep half are read before the
        // barrier that publishes the next stage and multiplied after it, while the next stage's first half is being read — every wave
        // leaves a barrier with 4*MF*NF/4 MFMAs of operands already in registers instead of with an LDS round trip in front of its
        // first MFMA (all waves of the workgroup pass the barrier together, so that round trip was exposed once per K-step).  The
        // protocol with the loaders is unchanged (barrier `it` publishes stage `it` and proves stage `it - 1` read: its reads are
        // drained by lgkmcnt(0) in front of the barrier) and so is the accumulation order: results stay bit-identical.
        const int pos0 = (fg ^ (fr & 7)) * 16, pos1 = pos0 ^ 64;
        const char* sA0 = smem + (wm * 16 * MF + fr) * 128;
        const char* sB0 = smem + BM * 128 + (wn * 16 * NF + fr) * 128;
        V8 af0[MF], wf0[NF], af1[MF], wf1[NF];
        asm volatile("s_barrier" ::: "memory");
    #pragma unroll
        for (int i = 0; i < MF; ++i) af0[i] = *(const V8*)(sA0 + i * 16 * 128 + pos0);
    #pragma unroll
        for (int j = 0; j < NF; ++j) wf0[j] = *(const V8*)(sB0 + j * 16 * 128 + pos0);
        int cur = 0;
        for (int it = 0; it + 1 < nk; ++it) {
            const char* sA = sA0 + cur * STAGE;
            const char* sB = sB0 + cur * STAGE;
    #pragma unroll
            for (int i = 0; i < MF; ++i) af1[i] = *(const V8*)(sA + i * 16 * 128 + pos1);
    #pragma unroll
            for (int j = 0; j < NF; ++j) wf1[j] = *(const V8*)(sB + j * 16 * 128 + pos1);
    #pragma unroll
            for (int i = 0; i < MF; ++i)
    #pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf0[j], af0[i], acc[i][j]);
            cur = cur + 1 == NS ? 0 : cur + 1;
            // lgkmcnt(0): this wave's fragment reads of stage `it` have returned before the loaders may overwrite its buffer.  As a
            // BUILTIN (0xC07F = lgkmcnt 0, vmcnt / expcnt untouched): the compiler's wait-count pass cannot see inside inline asm and
            // would otherwise make the first MFMAs behind the barrier wait for the reads issued behind it as well
            __builtin_amdgcn_s_waitcnt(0xC07F);
            asm volatile("s_barrier" ::: "memory");
            const char* nA = sA0 + cur * STAGE;
            const char* nB = sB0 + cur * STAGE;
    #pragma unroll
            for (int i = 0; i < MF; ++i) af0[i] = *(const V8*)(nA + i * 16 * 128 + pos0);
    #pragma unroll
            for (int j = 0; j < NF; ++j) wf0[j] = *(const V8*)(nB + j * 16 * 128 + pos0);
    #pragma unroll
            for (int i = 0; i < MF; ++i)
    #pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf1[j], af1[i], acc[i][j]);
        }
        {                                                          // the last K-step: no barrier behind its first half
            const char* sA = sA0 + cur * STAGE;
            const char* sB = sB0 + cur * STAGE;
    #pragma unroll
            for (int i = 0; i < MF; ++i) af1[i] = *(const V8*)(sA + i * 16 * 128 + pos1);
    #pragma unroll
            for (int j = 0; j < NF; ++j) wf1[j] = *(const V8*)(sB + j * 16 * 128 + pos1);
    #pragma unroll
            for (int i = 0; i < MF; ++i)
    #pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf0[j], af0[i], acc[i][j]);
    #pragma unroll
            for (int i = 0; i < MF; ++i)
    #pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf1[j], af1[i], acc[i][j]);
        }
    } else {
        // 64-row tiles (the short-K linears of the batch-1 UNet): plain order — barrier, both halves' reads, MFMAs (the rotated loop was
        // measured -0.3 % end to end at batch 1 with these tiles in it: nothing to hide behind 5-10 MFMAs per half)
        int cur = 0;
        for (int it = 0; it < nk; ++it) {
            // lgkmcnt(0): this wave's fragment reads of the previous stage have returned before the loaders may overwrite its buffer
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            const char* sA = smem + cur * STAGE + (wm * 16 * MF + fr) * 128;
            const char* sB = smem + cur * STAGE + BM * 128 + (wn * 16 * NF + fr) * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int pos = ((ks * 4 + fg) ^ (fr & 7)) * 16;
                V8 af[MF], wf[NF];
#pragma unroll
                for (int i = 0; i < MF; ++i) af[i] = *(const V8*)(sA + i * 16 * 128 + pos);
#pragma unroll
                for (int j = 0; j < NF; ++j) wf[j] = *(const V8*)(sB + j * 16 * 128 + pos);
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf[j], af[i], acc[i][j]);
            }
            cur = cur + 1 == NS ? 0 : cur + 1;
        }
    }
    idb_gemm_epilogue<T, MF, NF, WM, RELU>(p, smem, acc, m0, n0, tid, wm, wn, fr, fg, kz, p.ln_stats != nullptr, ln_part);
#endif
}

template <typename T, int MF, int NF, int NS, int WM, int LW>
__global__ __launch_bounds__(128 * WM + 64 * LW) void idb_gemm_kernel_lw(IDB_TILE_PARAMS, const GemmParams p) {
    idb_gemm_kernel_lw_body<T, MF, NF, NS, WM, LW, false>(IDB_TILE_PACK, p);
}

template <typename T, int MF, int NF, int NS, int WM, int LW>
__global__ __launch_bounds__(128 * WM + 64 * LW) void idb_gemm_kernel_lw_relu(IDB_TILE_PARAMS, const GemmParams p) {
    idb_gemm_kernel_lw_body<T, MF, NF, NS, WM, LW, true>(IDB_TILE_PACK, p);
}


// ------------------------------------------------------------------------------------------------------------
// Patch-resident 3x3 conv (round 3) for large grids: the 256-row loader-wave tile with the ACTIVATION operand fetched once per
// 64-channel chunk instead of once per tap.  A tile of 256 output pixels is whole image rows (W | 256), so for one channel chunk
// the nine taps read shifted windows of ONE halo patch — (rows + 2) x (W + 2) pixels x 128 B, <= 400 pixels = 50 KB — that sits in
// LDS while the K loop walks tap after tap over it: K order is chunk-major ([chunk][tap], the weight K-step index is
// tap * C/64 + chunk, an SGPR offset either way).  Per K-step the workgroup now moves patch/9 + BN*128 B into LDS instead of
// (256 + BN) * 128 B: 26 KB instead of 52 KB at BN = 160 — 195 instead of 97 FLOP per byte moved L2 -> LDS, and
// the same drop in LDS write traffic, which shares the LDS port with the fragment reads.
//   roles (wave index): [0, 8) MFMA — fragment mapping, epilogue and wave tile of idb_gemm_kernel_lw<T,4,NF,3,4,4>; [8, 10) weight
//   loaders (3-stage ring, counted vmcnt); [10, 12) patch loaders (double-buffered patch: chunk c+1 lands while the nine taps of
//   chunk c run; one vmcnt(0) per chunk).  ONE s_barrier per K-step for every role, no flags, no polling.
//   1x1 K segments (a ResnetBlock2D's conv_shortcut fused behind conv2) go through the same structure with a halo-less "patch" of the
//   256 tile pixels and one tap per chunk.  Zero padding = out-of-range buffer offsets, as everywhere.
// The accumulation order over K differs from the tap-major kernels, so results are equal to rounding, not bit-identical.
// ------------------------------------------------------------------------------------------------------------
// K-step g of the chunk-major K walk ([segment][chunk][tap]) -> segment s, chunk c, tap t, K-step base of that segment's weights
__device__ __forceinline__ void idb_patch_seek(const GemmTile& h, const GemmParams& p, int g, int& s, int& c, int& t, int& base) {
    const int st[IDB_MAX_SRC - 1] = {h.st01 & 0xffff, (int)((unsigned)h.st01 >> 16), h.mode_st2 & 0xffff};   // no load in front of s
    s = 0;
    base = 0;
#pragma unroll
    for (int q = 0; q < IDB_MAX_SRC - 1; ++q) {
        if (s == q && g >= st[q]) {
            g -= st[q];
            base += st[q];
            ++s;
        }
    }
    const int taps = p.src[s].taps;                            // 9 or 1: a division by a literal is a multiply-high
    c = taps == 9 ? g / 9 : g;
    t = g - c * taps;
}

// GN = true pieces shared by the transforming patch loaders and the MFMA waves that help with the first patch (below).
// {sum, sumsq} partials of eight groups (pw * 8 ..), 8 lanes per group: loads only
__device__ __forceinline__ void idb_gn_part_load(const GemmParams& p, int b0, int pw, int lane, f32x2 (&pv)[8]) {
    const int G = p.gn_in_groups;
    const int g = min(pw * 8 + (lane >> 3), G - 1), sub = lane & 7;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int ch = min(sub + 8 * u, p.gn_in_chunks - 1);
        pv[u] = *(const f32x2*)(p.gn_in_part + (((long long)b0 * p.gn_in_chunks + ch) * G + g) * 2);
    }
}

// {mean, rstd} of those groups into gst: the pixel-chunk partials are added in gn_apply_kernel's order
__device__ __forceinline__ void idb_gn_part_finish(const GemmParams& p, float2* gst, int pw, int lane, const f32x2 (&pv)[8]) {
    const int G = p.gn_in_groups, cpg = p.gn_in_cpg;
    const int g = min(pw * 8 + (lane >> 3), G - 1), sub = lane & 7;
    float a = 0.f, q = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (sub + 8 * u < p.gn_in_chunks) {
            a += pv[u][0];
            q += pv[u][1];
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        a += __shfl_xor(a, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if (pw * 8 + (lane >> 3) < G && sub == 0) {
        const double cnt = (double)p.HW * cpg;
        const double mean = (double)a / cnt;
        double var = (double)q / cnt - mean * mean;
        if (var < 0.0) var = 0.0;
        gst[g] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)p.gn_in_eps)));
    }
}

// k = rstd * gamma, h = beta - mean * k of the 8 channels from ch0.  The group of a channel is ch / cpg as ONE v_mul_hi_u32 with
// rcpg = ceil(2^32 / cpg) (exact for ch * cpg < 2^32; cpg = 1 has no such reciprocal in 32 bits): eight integer divisions by a run-time
// value were some 250 VALU instructions, in front of the first patch and in one K-step interval of every chunk
__device__ __forceinline__ void idb_gn_coeffs(const float2* gst, int ch0, int cpg, unsigned rcpg, f32x4 g0v, f32x4 g1v, f32x4 b0v, f32x4 b1v, float (&kk)[8],
                                              float (&hh)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float2 st = gst[cpg == 1 ? ch0 + e : (int)__umulhi((unsigned)(ch0 + e), rcpg)];
        kk[e] = st.y * (e < 4 ? g0v[e] : g1v[e - 4]);
        hh[e] = (e < 4 ? b0v[e] : b1v[e - 4]) - st.x * kk[e];
    }
}

// y = silu(x * k + h) in fp32, one rounding; a padding pixel (ok = false: its load was zero-filled) stays zero
template <typename T>
__device__ __forceinline__ typename Op<T>::v8 idb_gn_norm8(typename Op<T>::v8 r, bool ok, int silu, const float (&kk)[8], const float (&hh)[8]) {
    typename Op<T>::v8 o = r;
    if (ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float y = to_f32<T>(r[e]) * kk[e] + hh[e];
            if (silu) y = silu_f(y);
            o[e] = from_f32<T>(y);
        }
    }
    return o;
}

// MF = 4: 256-row tiles, 3-stage weight ring (large grids).  MF = 1 / 2: 64- / 128-row tiles, 4-stage ring, split-K by whole chunks
// (the one-workgroup-per-CU plans of the batch-1 UNet): the patch is 3-4 image rows there, the saving is the 9x smaller activation
// stream of a K-step whose weight stream is unchanged.
// GN = true (north_star "conv3x3 + GroupNorm+SiLU fused"; ResnetBlock2D norm1+conv1 / norm2+conv2 via inference_ID-Booth.py:138): the
// patch loaders become FOUR waves that fetch the raw patch into registers, apply y = silu(x * k[c] + h[c]) — gn_apply_kernel's arithmetic
// on the same partial sums (k = rstd * gamma, h = beta - mean * k), so the MFMA waves read the operands idb_groupnorm would have written —
// and store it to the patch buffer, one slice between each pair of the chunk's nine barriers.  The patch is normalised ONCE per chunk (the
// tap-major idb_gemm_kernel_gn re-normalises every pixel for each of its nine taps and lost on every 3x3 conv); padding pixels stay zero.
// Every K segment is a normalised 3x3 source and a tile lies inside one sample (host: gemm_fuses_gn).
template <typename T, int MF, int NF, int NS, bool GN = false>
__global__ __launch_bounds__(GN ? 896 : 768) void idb_conv_patch_kernel(IDB_TILE_PARAMS, const GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using V8 = typename Op<T>::v8;
    constexpr int WM = 4;
    constexpr int BM = 64 * MF, BN = 32 * NF;
    constexpr int PL = GN ? 4 : 2;                             // patch-loader waves
    constexpr int PP_PAD = MF == 1 ? (GN ? 224 : 208) : MF == 2 ? (GN ? 288 : 272) : 400;   // patch pixels, padded to the patch loaders' sweep of 8 * PL pixels (host: conv_patch_ok)
    constexpr int PATCH = PP_PAD * 128;                        // bytes of one patch buffer
    constexpr int NPI = PP_PAD / (8 * PL);                     // 16-byte-per-lane loads per patch-loader wave and chunk
    constexpr int NJ = BN / 16;                                // weight-row sweeps of the two weight loaders (8 rows per instruction)
    constexpr int BSTAGE = BN * 128;
    static_assert(2 * PATCH + NS * BSTAGE + (GN ? 256 : 0) <= 160 * 1024 && (MF < 4 || !GN), "LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem + 2 * PATCH;
    float2* gst = (float2*)(ring + NS * BSTAGE);               // GN: {mean, rstd} of the tile's sample, per group

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const GemmTile gt = IDB_TILE_PACK;                         // tile index, K range and the seek's source: no kernel-argument load
    int wg, kz, tm, tn;
    idb_wg_tile(gt, wg, kz);
    idb_tile_mn(gt, wg, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    // this workgroup's K range in K-steps of the chunk-major walk (balanced; a split may start and end inside a chunk)
    int g0, g1;
    idb_k_range(gt, kz, g0, g1);
    const int nk = g1 - g0;
    int s0, c0, t0, base0;
    idb_patch_seek(gt, p, g0, s0, c0, t0, base0);
    // tile geometry: R image rows of width W; nimg whole images when the image is smaller than the tile
    // (resolved on the host for this variant's BM: idb_fill_geometry)
    const int W = p.OW, H = p.pc_H;
    [[maybe_unused]] const int nimg = p.pc_nimg;
    const int RI = p.pc_RI;                                    // tile rows per image

    // GN, the prologue (everything in front of the first MFMA) runs on all twelve non-weight waves:
    //   * MFMA waves 0-3 load the producer's partial sums at once and turn them into {mean, rstd} per group (gst) in front of barrier S,
    //     while the patch loaders work out their patch addresses; nothing that does not need the statistics waits for them — the raw
    //     first patch and gamma / beta of the first chunk are requested before any wait, so ONE memory round trip is exposed;
    //   * behind barrier S the first patch is normalised by all twelve: of its NU eight-pixel units the patch loaders keep the first LI of
    //     their sweep (unit i * PL + pw, i < LI), MFMA wave w takes units PL * LI + w * NH + [0, NH), fetched raw by that wave in front of
    //     barrier S: 2-3 units per wave instead of 7-9 on four.
    // Barriers per role (a barrier that one wave misses hangs the workgroup): MFMA waves S + 1 (in front of the K loop) + (nk - 1) (in it),
    // weight loaders S + nk, patch loaders S + the sum over their chunks of 1 + (n - 1) = S + nk: S + nk each, as before.  The first K
    // barrier publishes patch buffer 0, so every wave that stored to it has lgkmcnt(0) in front of that barrier; the stores of the loaders
    // (units < PL * LI) and of the MFMA waves are disjoint, and buffer 0 is next written behind the first barrier of the second chunk.
    constexpr int NU = PP_PAD / 8;
    constexpr int LI = (NU + 11) / 12;
    constexpr int NH = GN ? (NU - PL * LI) / 8 : 1;
    static_assert(!GN || (PL * LI + 8 * NH == NU && LI <= NPI), "first-patch split over 4 + 8 waves");
    [[maybe_unused]] V8 hraw[NH];                              // MFMA waves: their raw units of the first patch,
    [[maybe_unused]] bool hok[NH];                             // inside the image?
    [[maybe_unused]] f32x4 hg0, hg1, hb0, hb1;                 // gamma / beta of their 8 channels of the first chunk
    [[maybe_unused]] f32x2 hpv[8];                             // waves 0-3: the partial sums of eight groups
    [[maybe_unused]] int hch0 = 0, hcpg = 1;
    [[maybe_unused]] unsigned hrcpg = 0;

    if constexpr (GN) {
        const int q8 = lane >> 3;
        int b0, y0, x0;
        idb_row_decode(p, m0, b0, y0, x0);
        const int cpg = p.gn_in_cpg;
        const unsigned rcpg = p.gn_in_rcpg;                    // ceil(2^32 / cpg) for cpg > 1 (idb_gn_coeffs)
        const int co = (lane & 7) ^ q8;                        // this lane's channel octet inside every chunk (pixel q has q & 7 == q8)
        const int PW = W + 2, PP = (RI + 2) * PW;
        const unsigned rpw = p.pc_rpw;                         // ceil(2^16 / PW): q / PW == (q * rpw) >> 16: q < 288, PW <= 66, so q * (rpw * PW - 65536) < 65536
        // patch pixel q -> offset of this lane's 16 bytes in a source of C channels (IDB_OOB: outside the image or behind the patch's last pixel)
        auto pix_voff = [&](int q, int C, bool& ok) -> unsigned {
            const int pr = (int)(((unsigned)q * rpw) >> 16), px = q - pr * PW;
            const int y = y0 + pr - 1, x = px - 1;
            ok = q < PP && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const int pix = (b0 * H + y) * W + x;
            return ok ? (unsigned)pix * (unsigned)(C * 2) + (unsigned)(co * 16) : IDB_OOB;
        };
        if (wave < 8) {
            // ---------------- MFMA waves, first half of their prologue: requests only ----------------
            if (wave < 4) idb_gn_part_load(p, b0, wave, lane, hpv);
            const GemmSrcK S = p.src[s0];
            int cb = 0;
            for (int q = 0; q < s0; ++q) cb += p.src[q].C;
            hch0 = cb + c0 * 64 + co * 8;
            hcpg = cpg;
            hrcpg = rcpg;
            hg0 = *(const f32x4*)(p.gn_in_gamma + hch0), hg1 = *(const f32x4*)(p.gn_in_gamma + hch0 + 4);
            hb0 = *(const f32x4*)(p.gn_in_beta + hch0), hb1 = *(const f32x4*)(p.gn_in_beta + hch0 + 4);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                const unsigned vo = pix_voff((PL * LI + wave * NH + j) * 8 + q8, S.C, hok[j]);
                hraw[j] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)c0 * 128u, 0));
            }
        } else if (wave >= 10) {
            // ---------------- transforming patch loaders (registers -> normalise -> LDS) ----------------
            const int pw = wave - 10;
            unsigned voff[NPI];
            bool okp[NPI];
            int seg = -1, cb = 0;
            __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.src[0].ptr, 0, p.src[0].bytes, IDB_RSRC_FLAGS);
            auto setup = [&](int s) {
                const GemmSrcK S = p.src[s];
                rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
#pragma unroll
                for (int i = 0; i < NPI; ++i) voff[i] = pix_voff((i * PL + pw) * 8 + q8, S.C, okp[i]);
                cb = 0;
                for (int q = 0; q < s; ++q) cb += p.src[q].C;   // first channel of source s inside the normalised concatenation
                seg = s;
            };
            V8 raw[NPI];
            f32x4 g0v, g1v, b0v, b1v;
            float kk[8], hh[8];
            int ch0 = 0;
            auto fetch_gb = [&]() {                            // gamma / beta of this lane's 8 channels
                g0v = *(const f32x4*)(p.gn_in_gamma + ch0), g1v = *(const f32x4*)(p.gn_in_gamma + ch0 + 4);
                b0v = *(const f32x4*)(p.gn_in_beta + ch0), b1v = *(const f32x4*)(p.gn_in_beta + ch0 + 4);
            };
            auto fetch = [&](int s, int c) {                   // the raw patch: loads only
                if (s != seg) setup(s);
                ch0 = cb + c * 64 + co * 8;
                const unsigned soff = (unsigned)c * 128u;
#pragma unroll
                for (int i = 0; i < NPI; ++i) raw[i] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], soff, 0));
            };
            auto coeffs = [&]() { idb_gn_coeffs(gst, ch0, cpg, rcpg, g0v, g1v, b0v, b1v, kk, hh); };   // the first use of the loads above
            auto put = [&](int i, int buf) {
                *(V8*)(smem + buf * PATCH + ((i * PL + pw) * 8 + q8) * 128 + (lane & 7) * 16) = idb_gn_norm8<T>(raw[i], okp[i], p.gn_in_silu, kk, hh);
            };
            int s = s0, c = c0, t = t0, buf = 0, done = 0;
            setup(s);                                          // the first patch: this wave's first LI units, the MFMA waves fetch the others
            ch0 = cb + c * 64 + co * 8;
            fetch_gb();
#pragma unroll
            for (int i = 0; i < LI; ++i) raw[i] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], (unsigned)c * 128u, 0));
            asm volatile("s_barrier" ::: "memory");            // barrier S: MFMA waves 0-3 have put the statistics into LDS
            coeffs();
#pragma unroll
            for (int i = 0; i < LI; ++i) put(i, 0);
            while (done < nk) {
                const int n = 9 - t < nk - done ? 9 - t : nk - done;
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // first K-step of the chunk: its normalised patch is in LDS
                done += n;
                int s2 = s, c2 = c + 1;
                if (c2 == (p.src[s].C >> 6)) { c2 = 0; if (s2 < IDB_MAX_SRC - 1) ++s2; }
                if (done < nk) {
                    fetch(s2, c2);
                    fetch_gb();
                    if (n == 9) {
                        // a whole chunk ahead: the loads fly during the chunk's first three K-steps, then one slice of the next patch is
                        // normalised and stored between each pair of the remaining barriers (the compiler's counted vmcnt: loads return in order)
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            if (k == 3) coeffs();
                            if (k >= 3) {
#pragma unroll
                                for (int i = (k - 3) * NPI / 5; i < (k - 2) * NPI / 5; ++i) put(i, buf ^ 1);
                            }
                            asm volatile("s_barrier" ::: "memory");
                        }
                    } else {                                   // a split boundary inside the chunk: everything at once
                        coeffs();
#pragma unroll
                        for (int i = 0; i < NPI; ++i) put(i, buf ^ 1);
                        for (int k = 1; k < n; ++k) asm volatile("s_barrier" ::: "memory");
                    }
                } else {
                    for (int k = 1; k < n; ++k) asm volatile("s_barrier" ::: "memory");
                }
                s = s2; c = c2; t = 0; buf ^= 1;
            }
            return;
        }
    }
    if (!GN && wave >= 10) {
        // ---------------- patch loaders ----------------
        const int pw = wave - 10;
        const int q8 = lane >> 3;
        int b0, y0, x0;
        idb_row_decode(p, m0, b0, y0, x0);
        unsigned voff[NPI];
        int seg = -1, npi = 0;
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.src[0].ptr, 0, p.src[0].bytes, IDB_RSRC_FLAGS);
        auto setup = [&](int s) {
            const GemmSrcK S = p.src[s];
            rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
            const int h = S.taps == 9 ? 1 : 0;
            const int PW = W + 2 * h, RIh = RI + 2 * h;
            const int PP = nimg * RIh * PW;
            npi = (PP + 15) >> 4;
#pragma unroll
            for (int i = 0; i < NPI; ++i) {
                const int q = (i * 2 + pw) * 8 + q8;
                const int pr = idb_fd_div(q, p.fd_pw[h]), px = q - pr * PW;
                const int img = idb_fd_div(pr, p.fd_rih[h]), lr = pr - img * RIh;
                const int y = y0 + lr - h, x = px - h;
                const bool ok = q < PP && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
                const int pix = ((b0 + img) * H + y) * W + x;
                voff[i] = ok ? (unsigned)pix * (unsigned)(S.C * 2) + (unsigned)(((lane & 7) ^ q8) * 16) : IDB_OOB;
            }
            seg = s;
        };
        auto issue = [&](int s, int c, int buf) {
            if (s != seg) setup(s);
            char* dst = smem + buf * PATCH + pw * 1024;
            const unsigned soff = (unsigned)c * 128u;
#pragma unroll
            for (int i = 0; i < NPI; ++i)
                if (i < npi) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, LDS_PTR(dst + i * 2048), 16, voff[i], soff, 0, 0);
        };
        int s = s0, c = c0, t = t0, buf = 0, done = 0;
        issue(s, c, 0);
        while (done < nk) {
            const int taps = p.src[s].taps, CS = p.src[s].C >> 6;
            const int n = taps - t < nk - done ? taps - t : nk - done;          // this split's K-steps inside the chunk
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");      // first of them: the chunk's patch has landed
            done += n;
            int s2 = s, c2 = c + 1;
            if (c2 == CS) { c2 = 0; if (s2 < IDB_MAX_SRC - 1) ++s2; }
            if (done < nk) issue(s2, c2, buf ^ 1);             // into the buffer of the PREVIOUS chunk: every read of it is behind the barrier
            for (int k = 1; k < n; ++k) asm volatile("s_barrier" ::: "memory");
            s = s2; c = c2; t = 0; buf ^= 1;
        }
        return;
    }
    if (wave >= 8) {
        // ---------------- weight loaders ----------------
        const int bw = wave - 8;
        const int lrow = lane >> 3;
        const unsigned cg16 = ((lane & 7) ^ lrow) * 16;
        const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + idb_weight_group(p, m0) * p.w_group_stride), 0, p.w_bytes, IDB_RSRC_FLAGS);
        unsigned w_voff[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = n0 + j * 16 + bw * 8 + lrow;
            w_voff[j] = n < p.N ? (unsigned)(n >> 4) * p.w_blk_bytes + (unsigned)(n & 15) * p.w_row_bytes + cg16 : IDB_OOB;
        }
        int s = s0, c = c0, tap = t0, base = base0;
        int taps = p.src[s].taps, CS = p.src[s].C >> 6;
        auto stage = [&](int buf) {
            char* sB = ring + buf * BSTAGE + bw * 1024;
            const unsigned soff = (unsigned)(base + tap * CS + c) * p.w_kstep;
#pragma unroll
            for (int j = 0; j < NJ; ++j) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(sB + j * 2048), 16, w_voff[j], soff, 0, 0);
            if (++tap == taps) {
                tap = 0;
                if (++c == CS) {
                    c = 0;
                    base += taps * CS;
                    if (s < IDB_MAX_SRC - 1) ++s;
                    taps = p.src[s].taps;
                    CS = p.src[s].C >> 6;
                }
            }
        };
#pragma unroll
        for (int st = 0; st < NS - 1; ++st)
            if (st < nk) stage(st);
        if constexpr (GN) asm volatile("s_barrier" ::: "memory");   // barrier S
        int cur = 0;
        for (int it = 0; it < nk; ++it) {
            if (it + NS - 2 < nk)
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * NJ) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            if (it + NS - 1 < nk) stage(cur == 0 ? NS - 1 : cur - 1);
            cur = cur + 1 == NS ? 0 : cur + 1;
        }
        return;
    }

    // ---------------- MFMA waves ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int rr[MF], xx[MF];                                        // tile row -> (patch row without halo, x)
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int ml = wm * 16 * MF + i * 16 + fr;
        const int r = idb_fd_div(ml, p.fd_ow);
        xx[i] = ml - r * W;
        rr[i] = r + 2 * idb_fd_div(r, p.fd_rih[0]);                              // + 2 halo rows per image in front (9-tap segments only)
    }
    // K-step state (segment s, chunk c, tap t) and the half-step rotation around the barrier of idb_gemm_kernel_lw: the second 32-deep
    // half of a K-step is read before the barrier that publishes the next one and multiplied behind it
    int cur = 0, pb = 0, s = s0, c = c0, t = t0, ky = t0 / 3, kx = t0 - 3 * (t0 / 3);
    int taps = p.src[s].taps, CS = p.src[s].C >> 6, h = taps == 9 ? 1 : 0, PW = W + 2 * h;
    int pp0[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) pp0[i] = h ? rr[i] * PW + xx[i] : wm * 16 * MF + i * 16 + fr;
    const int posw0 = (fg ^ (fr & 7)) * 16;
    const char* sBw = ring + (wn * 16 * NF + fr) * 128;
    unsigned a_addr[MF];
    auto addr = [&]() {
        const int toff = ky * PW + kx;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int pp = pp0[i] + toff;
            a_addr[i] = (unsigned)(pb * PATCH) + (unsigned)pp * 128u + (unsigned)((fg ^ (pp & 7)) << 4);
        }
    };
    auto advance = [&]() {
        cur = cur + 1 == NS ? 0 : cur + 1;
        if (++kx == 3) { kx = 0; ++ky; }
        if (++t == taps) {
            t = 0; ky = 0; kx = 0;
            pb ^= 1;
            if (++c == CS) {
                c = 0;
                if (s < IDB_MAX_SRC - 1) ++s;
                taps = p.src[s].taps;
                CS = p.src[s].C >> 6;
                h = taps == 9 ? 1 : 0;
                PW = W + 2 * h;
#pragma unroll
                for (int i = 0; i < MF; ++i) pp0[i] = h ? rr[i] * PW + xx[i] : wm * 16 * MF + i * 16 + fr;
            }
        }
    };
    V8 af0[MF], wf0[NF], af1[MF], wf1[NF];
    if constexpr (GN) {
        // second half of the MFMA waves' prologue: the statistics (waves 0-3), barrier S, this wave's units of the first patch
        if (wave < 4) idb_gn_part_finish(p, gst, wave, lane, hpv);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // barrier S: the statistics are in LDS
        float kk[8], hh[8];
        idb_gn_coeffs(gst, hch0, hcpg, hrcpg, hg0, hg1, hb0, hb1, kk, hh);
#pragma unroll
        for (int j = 0; j < NH; ++j)
            *(V8*)(smem + ((PL * LI + wave * NH + j) * 8 + (lane >> 3)) * 128 + (lane & 7) * 16) = idb_gn_norm8<T>(hraw[j], hok[j], p.gn_in_silu, kk, hh);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // ... are in patch buffer 0 before the barrier that publishes it
    }
    asm volatile("s_barrier" ::: "memory");
    addr();
#pragma unroll
    for (int i = 0; i < MF; ++i) af0[i] = *(const V8*)(smem + a_addr[i]);
#pragma unroll
    for (int j = 0; j < NF; ++j) wf0[j] = *(const V8*)(sBw + j * 16 * 128 + posw0);
    for (int it = 0; it + 1 < nk; ++it) {
        const char* sB = sBw + cur * BSTAGE;
#pragma unroll
        for (int i = 0; i < MF; ++i) af1[i] = *(const V8*)(smem + (a_addr[i] ^ 64u));
#pragma unroll
        for (int j = 0; j < NF; ++j) wf1[j] = *(const V8*)(sB + j * 16 * 128 + (posw0 ^ 64));
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf0[j], af0[i], acc[i][j]);
        advance();
        addr();
        __builtin_amdgcn_s_waitcnt(0xC07F);                    // lgkmcnt(0), as a builtin (see idb_gemm_kernel_lw)
        asm volatile("s_barrier" ::: "memory");
        const char* nB = sBw + cur * BSTAGE;
#pragma unroll
        for (int i = 0; i < MF; ++i) af0[i] = *(const V8*)(smem + a_addr[i]);
#pragma unroll
        for (int j = 0; j < NF; ++j) wf0[j] = *(const V8*)(nB + j * 16 * 128 + posw0);
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf1[j], af1[i], acc[i][j]);
    }
    {
        const char* sB = sBw + cur * BSTAGE;
#pragma unroll
        for (int i = 0; i < MF; ++i) af1[i] = *(const V8*)(smem + (a_addr[i] ^ 64u));
#pragma unroll
        for (int j = 0; j < NF; ++j) wf1[j] = *(const V8*)(sB + j * 16 * 128 + (posw0 ^ 64));
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf0[j], af0[i], acc[i][j]);
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf1[j], af1[i], acc[i][j]);
    }
    idb_gemm_epilogue<T, MF, NF, WM>(p, smem, acc, m0, n0, tid, wm, wn, fr, fg, kz, false, make_float2(0.f, 0.f));
#endif
}


// ------------------------------------------------------------------------------------------------------------
// GroupNorm(+SiLU) -> conv / linear in ONE kernel (round 3; north_star "conv3x3 + GroupNorm+SiLU fused"; diffusers ResnetBlock2D
// norm1+conv1, norm2+conv2(+shortcut), Transformer2DModel norm+proj_in via inference_ID-Booth.py:138) on the loader-wave structure:
// a THIRD role, NV normalizer waves, transforms each landed A stage in place in LDS — y = silu(x * k[b][c] + h[b][c]), the exact
// arithmetic of gn_apply_kernel (k = rstd * gamma, h = beta - mean * k from the same partial sums, added in the same order, so the
// MFMA waves read bit-identical operands) — one K-step ahead of the MFMA waves.  The normalised tensor never exists in HBM and the
// gn_apply launch (60 per CFG forward, 6.4 us each at batch 1) disappears.  Round 2's idb_hconv did this transform on the MFMA
// waves themselves and lost; here it runs on waves that do nothing else, so the MFMA waves' stream is unchanged.
//   roles (wave index): [0, 2*WM) MFMA, [2*WM, 2*WM + 4) loaders, then NV normalizers.  Every wave passes the same barriers:
//   two while the normalizers build the {k, h} table in LDS (group statistics, then per channel), one that publishes the
//   normalised stage 0, then one per K-step.  Ring of NS stages: at K-step `it` the MFMA waves read stage it, the normalizers
//   transform stage it+1 (landed: the loaders waited for it before the barrier), stages it+2 .. are in flight.
//   Zero padding stays zero: rows whose tap falls outside the image are skipped (silu(h) != 0).  Sources beyond gn_in_nsrc (the
//   raw inputs of a fused 1x1 shortcut) pass untouched.  A tile lies inside one sample, or covers whole samples (host check).
// ------------------------------------------------------------------------------------------------------------
template <typename T, int MF, int NF, int NS, int WM, int NV>
__global__ __launch_bounds__(128 * WM + 256 + 64 * NV) void idb_gemm_kernel_gn(IDB_TILE_PARAMS, const GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using V8 = typename Op<T>::v8;
    constexpr int LW = 4;
    constexpr int BM = 16 * MF * WM, BN = 32 * NF;
    constexpr int CT = 128 * WM, LT = 64 * LW, VT = 64 * NV;
    constexpr int LR = 8 * LW;
    constexpr int NA = BM / LR, NJ = (BN + LR - 1) / LR;
    constexpr int STAGE = (BM + NJ * LR) * 128;
    constexpr int LOADS = NA + NJ;
    constexpr int NI = BM * 8 / VT;                            // 16-byte items of an A stage per normalizer lane
    static_assert(BM % LR == 0 && (BM * 8) % VT == 0, "tile / role geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* tab = (float2*)(smem + NS * STAGE);                // [nsamp][gn_in_c] {k, h}
    const int hw_s = p.HW;
    const int nsamp = p.gn_in_nsamp;                           // BM > HW ? BM / HW : 1 (host: HW % BM == 0 or BM % HW == 0)
    float2* gstat = tab + nsamp * p.gn_in_c;                   // [nsamp][groups] {mean, rstd}

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const GemmTile h = IDB_TILE_PACK;                          // tile index, K range and the seek's source: no kernel-argument load
    int wg, kz, tm, tn;
    idb_wg_tile(h, wg, kz);
    idb_tile_mn(h, wg, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    int kt0, kt1;
    idb_k_range(h, kz, kt0, kt1);
    const int nk = kt1 - kt0;

    // K-step cursor shared by loaders and normalizers: source s, tap, channel offset c0
    int s, rem, tap, c0;
    idb_k_seek_src(h, kt0, s, rem);
    idb_k_seek_tap(p.src[s], rem, tap, c0);
    auto advance = [&]() {                                     // to the next K-step
        c0 += 64;
        if (c0 == p.src[s].C) {
            c0 = 0;
            if (++tap == (p.src[s].taps == 9 ? 9 : 5)) {
                if (s < IDB_MAX_SRC - 1) ++s;
                tap = p.src[s].taps == 9 ? 0 : 4;
            }
        }
    };

    if (wave >= 2 * WM + LW) {
        // ---------------- normalizer waves ----------------
        const int nt = tid - CT - LT;
        const int b_first = idb_fd_div(m0, p.fd_hw);
        const int G = p.gn_in_groups, cpg = p.gn_in_cpg;
        // phase 1: {mean, rstd} per (sample, group): 8 lanes per pair add the pixel-chunk partials in gn_apply_kernel's order
        for (int pr0 = 0; pr0 < nsamp * G; pr0 += VT / 8) {
            const int pr = pr0 + (nt >> 3), sub = nt & 7;
            const int prc = min(pr, nsamp * G - 1);
            const int sm = idb_fd_div(prc, p.fd_gn_g), g = prc - sm * G;
            const int b = min(b_first + sm, p.gn_in_last_b);
            f32x2 pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int ch = min(sub + 8 * u, p.gn_in_chunks - 1);
                pv[u] = *(const f32x2*)(p.gn_in_part + (((long long)b * p.gn_in_chunks + ch) * G + g) * 2);
            }
            float a = 0.f, q = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (sub + 8 * u < p.gn_in_chunks) {
                    a += pv[u][0];
                    q += pv[u][1];
                }
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                a += __shfl_xor(a, o, 64);
                q += __shfl_xor(q, o, 64);
            }
            if (pr < nsamp * G && sub == 0) {
                const double cnt = (double)hw_s * cpg;
                const double mean = (double)a / cnt;
                double var = (double)q / cnt - mean * mean;
                if (var < 0.0) var = 0.0;
                gstat[pr] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)p.gn_in_eps)));
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                     // barrier A
        // phase 2: k = rstd * gamma, h = beta - mean * k per (sample, channel)
        for (int i = nt; i < nsamp * p.gn_in_c; i += VT) {
            const int sm = idb_fd_div(i, p.fd_gn_c), c = i - sm * p.gn_in_c;
            const float2 st = gstat[sm * G + idb_fd_div(c, p.fd_gn_cpg)];
            const float k = st.y * p.gn_in_gamma[c];
            tab[i] = make_float2(k, p.gn_in_beta[c] - st.x * k);
        }
        // rows of this lane's items: item j = row j * (VT / 8) + (nt >> 3), LDS chunk position nt & 7
        int r_b[NI], r_oy[NI], r_ox[NI];
        bool r_ok[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int row = j * (VT / 8) + (nt >> 3);
            const int m = m0 + row;
            r_ok[j] = m < p.M;
            idb_row_decode(p, r_ok[j] ? m : 0, r_b[j], r_oy[j], r_ox[j]);
            r_b[j] -= b_first;
        }
        int cb = 0;                                            // first channel of source s inside the normalised concatenation
        for (int q = 0; q < s; ++q) cb += p.src[q].C;
        int s_seen = s;
        const int pos = nt & 7;
        auto transform = [&](int buf) {
            if (s != s_seen) {                                 // entered the next source
                cb += p.src[s_seen].C;
                s_seen = s;
            }
            if (s < p.gn_in_nsrc) {
                const GemmSrcK S = p.src[s];
                const int t3 = tap / 3;
                const int dy = t3 - p.pad, dx = tap - t3 * 3 - p.pad;
                const int LH = S.H << S.up, LWd = S.W << S.up;
                char* sA = smem + buf * STAGE;
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int row = j * (VT / 8) + (nt >> 3);
                    const int iy = r_oy[j] * p.stride + dy, ix = r_ox[j] * p.stride + dx;
                    const bool ok = r_ok[j] && (S.taps == 1 || ((unsigned)iy < (unsigned)LH && (unsigned)ix < (unsigned)LWd));
                    if (ok) {
                        const int c = cb + c0 + 8 * (pos ^ (row & 7));
                        const f32x4* tp = (const f32x4*)(tab + r_b[j] * p.gn_in_c + c);
                        const f32x4 t0 = tp[0], t1 = tp[1], t2 = tp[2], t3v = tp[3];      // {k,h} x 8 channels
                        V8* px = (V8*)(sA + row * 128 + pos * 16);
                        const V8 raw = *px;
                        const float ks[8] = {t0[0], t0[2], t1[0], t1[2], t2[0], t2[2], t3v[0], t3v[2]};
                        const float kh[8] = {t0[1], t0[3], t1[1], t1[3], t2[1], t2[3], t3v[1], t3v[3]};
                        V8 o;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float y = to_f32<T>(raw[e]) * ks[e] + kh[e];
                            if (p.gn_in_silu) y = silu_f(y);
                            o[e] = from_f32<T>(y);
                        }
                        *px = o;
                    }
                }
            }
            advance();
        };
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                     // barrier B: table complete, stage 0 landed
        if (nk > 0) transform(0);
        int cur = 0;
        for (int it = 0; it < nk; ++it) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                 // barrier C_it
            const int nxt = cur + 1 == NS ? 0 : cur + 1;
            if (it + 1 < nk) transform(nxt);
            cur = nxt;
        }
        return;
    }

    if (wave >= 2 * WM) {
        // ---------------- loader waves ----------------
        const int lw = wave - 2 * WM;
        const int lt = tid - CT;
        const int lrow = lt >> 3;
        const unsigned cg16 = ((lt & 7) ^ (lrow & 7)) * 16;
        int a_b[NA], a_oy[NA], a_ox[NA];
        bool a_ok[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + i * LR + lrow;
            a_ok[i] = m < p.M;
            idb_row_decode(p, a_ok[i] ? m : 0, a_b[i], a_oy[i], a_ox[i]);
        }
        const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + idb_weight_group(p, m0) * p.w_group_stride), 0, p.w_bytes, IDB_RSRC_FLAGS);
        unsigned w_voff[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = n0 + j * LR + lrow;
            w_voff[j] = (n < p.N && j * LR + lrow < BN) ? (unsigned)(n >> 4) * p.w_blk_bytes + (unsigned)(n & 15) * p.w_row_bytes + cg16 : IDB_OOB;
        }
        unsigned w_soff = (unsigned)kt0 * p.w_kstep;
        __amdgpu_buffer_rsrc_t rs_a = rs_w;
        unsigned a_voff[NA];
        int last_s = -1, last_tap = -1;
        auto stage = [&](int buf) {
            char* sA = smem + buf * STAGE;
            char* sB = sA + BM * 128;
            if (s != last_s || tap != last_tap) {
                const GemmSrcK S = p.src[s];
                rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
                const int t3 = tap / 3;
                const int dy = t3 - p.pad, dx = tap - t3 * 3 - p.pad;
                const int LH = S.H << S.up, LWd = S.W << S.up;
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const int iy = a_oy[i] * p.stride + dy, ix = a_ox[i] * p.stride + dx;
                    const bool ok = a_ok[i] && (unsigned)iy < (unsigned)LH && (unsigned)ix < (unsigned)LWd;
                    const int pix = (a_b[i] * S.H + (iy >> S.up)) * S.W + (ix >> S.up);
                    a_voff[i] = ok ? (unsigned)pix * (unsigned)(S.C * 2) + cg16 : IDB_OOB;
                }
                last_s = s;
                last_tap = tap;
            }
            const unsigned a_soff = (unsigned)c0 * 2u;
#pragma unroll
            for (int i = 0; i < NA; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, LDS_PTR(sA + (i * 64 * LW + lw * 64) * 16), 16, a_voff[i], a_soff, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(sB + (j * 64 * LW + lw * 64) * 16), 16, w_voff[j], w_soff, 0, 0);
            w_soff += p.w_kstep;
            advance();
        };
#pragma unroll
        for (int st = 0; st < NS - 1; ++st)
            if (st < nk) stage(st);
        asm volatile("s_barrier" ::: "memory");                                             // barrier A
        if (NS - 1 <= nk)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * LOADS) : "memory");   // barrier B: stage 0 landed
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        int cur = 0;
        for (int it = 0; it < nk; ++it) {
            // stage it+1 landed (the normalizers transform it next); stages it+2 .. it+NS-2 stay in flight
            if (it + NS - 2 < nk)
                asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 3) * LOADS) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            if (it + NS - 1 < nk) stage(cur == 0 ? NS - 1 : cur - 1);
            cur = cur + 1 == NS ? 0 : cur + 1;
        }
        return;
    }

    // ---------------- MFMA waves ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    asm volatile("s_barrier" ::: "memory");                                                 // barrier A
    asm volatile("s_barrier" ::: "memory");                                                 // barrier B
    int cur = 0;
    for (int it = 0; it < nk; ++it) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                     // barrier C_it
        const char* sA = smem + cur * STAGE + (wm * 16 * MF + fr) * 128;
        const char* sB = smem + cur * STAGE + BM * 128 + (wn * 16 * NF + fr) * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pos = ((ks * 4 + fg) ^ (fr & 7)) * 16;
            // one weight fragment live at a time: with 4 MFMA waves the wave tile is 2x that of the 8-wave kernels and the workgroup's
            // 16 waves cap a wave at 128 VGPRs (80 of them accumulators at 128x160)
            V8 af[MF];
#pragma unroll
            for (int i = 0; i < MF; ++i) af[i] = *(const V8*)(sA + i * 16 * 128 + pos);
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const V8 wf = *(const V8*)(sB + j * 16 * 128 + pos);
#pragma unroll
                for (int i = 0; i < MF; ++i) acc[i][j] = Op<T>::mfma16(wf, af[i], acc[i][j]);
            }
        }
        cur = cur + 1 == NS ? 0 : cur + 1;
    }
    idb_gemm_epilogue<T, MF, NF, WM>(p, smem, acc, m0, n0, tid, wm, wn, fr, fg, kz, false, make_float2(0.f, 0.f));
#endif
}

// ------------------------------------------------------------------------------------------------------------
// Register-staged variant: identical tiling, addressing and epilogue, but the operands go HBM/L2 -> VGPR
// (buffer_load_dwordx4, asynchronous until its first use) -> LDS (ds_write_b128 after the MFMAs of the current
// tile).  Measured on MI355X: one `buffer_load ... lds` costs ~85 issue cycles, nine of them per K-step are as long
// as the 40 MFMAs they feed and serialise with them inside a wave; a register load + ds_write_b128 pair costs ~20.
// ------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned idb_u32x4;

template <typename T, int MF, int NF>
__global__ __launch_bounds__(256, 2) void idb_gemm_kernel_rs(const GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using V8 = typename Op<T>::v8;
    constexpr int BM = 32 * MF, BN = 32 * NF, STAGE = (BM + BN) * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    const int nwg = gridDim.x, orig = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
    const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    int tm, tn;
    idb_tile_mn(p, wg, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    const int kz = blockIdx.z;
    int kt0, kt1;
    idb_k_range(p, kz, kt0, kt1);
    const int nk = kt1 - kt0;

    // thread stages chunk (tid&7) of rows (tid>>3)+32i: global chunk c lands at LDS chunk position c ^ (row&7)
    const int lrow = tid >> 3;
    const unsigned c16 = (tid & 7) * 16;
    const int lds_off = lrow * 128 + (((tid & 7) ^ (lrow & 7)) * 16);
    int a_b[MF], a_oy[MF], a_ox[MF];
    bool a_ok[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + i * 32 + lrow;
        a_ok[i] = m < p.M;
        idb_row_decode(p, a_ok[i] ? m : 0, a_b[i], a_oy[i], a_ox[i]);
    }
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + idb_weight_group(p, m0) * p.w_group_stride), 0, p.w_bytes, IDB_RSRC_FLAGS);
    unsigned w_voff[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + j * 32 + lrow;
        w_voff[j] = n < p.N ? (unsigned)(n >> 4) * p.w_blk_bytes + (unsigned)(n & 15) * p.w_row_bytes + c16 : IDB_OOB;
    }
    unsigned w_soff = (unsigned)kt0 * p.w_kstep;

    int s, tap, c0, cur_c = 64, tap_end = 9;
    idb_k_seek(p, kt0, s, tap, c0);
    __amdgpu_buffer_rsrc_t rs_a = rs_w;
    unsigned a_voff[MF];
    bool need_retap = true;
    idb_u32x4 areg[MF], wreg[NF];
    auto gload = [&]() {
        if (need_retap) {
            const GemmSrcK S = p.src[s];
            rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
            cur_c = S.C;
            tap_end = S.taps == 9 ? 9 : 5;
            const int t3 = tap / 3;
            const int dy = t3 - p.pad, dx = tap - t3 * 3 - p.pad;
            const int LH = S.H << S.up, LW = S.W << S.up;
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                const int iy = a_oy[i] * p.stride + dy, ix = a_ox[i] * p.stride + dx;
                const bool ok = a_ok[i] && (unsigned)iy < (unsigned)LH && (unsigned)ix < (unsigned)LW;
                const int pix = (a_b[i] * S.H + (iy >> S.up)) * S.W + (ix >> S.up);
                a_voff[i] = ok ? (unsigned)pix * (unsigned)(S.C * 2) + c16 : IDB_OOB;
            }
            need_retap = false;
        }
        const unsigned a_soff = (unsigned)c0 * 2u;
#pragma unroll
        for (int i = 0; i < MF; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_a, a_voff[i], a_soff, 0);
#pragma unroll
        for (int j = 0; j < NF; ++j) wreg[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_voff[j], w_soff, 0);
        w_soff += p.w_kstep;
        c0 += 64;
        if (c0 == cur_c) {
            c0 = 0;
            need_retap = true;
            if (++tap == tap_end) {
                if (s < IDB_MAX_SRC - 1) ++s;
                tap = p.src[s].taps == 9 ? 0 : 4;
            }
        }
    };
    auto lstore = [&](int buf) {
        char* sA = smem + buf * STAGE + lds_off;
        char* sB = sA + BM * 128;
#pragma unroll
        for (int i = 0; i < MF; ++i) *(idb_u32x4*)(sA + i * 32 * 128) = areg[i];
#pragma unroll
        for (int j = 0; j < NF; ++j) *(idb_u32x4*)(sB + j * 32 * 128) = wreg[j];
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (nk > 0) {
        gload();
        lstore(0);
        __syncthreads();
    }
    for (int it = 0; it < nk; ++it) {
        const int cur = it & 1;
        if (it + 1 < nk) gload();                      // next tile -> registers, in flight under the MFMAs below
        const char* sA = smem + cur * STAGE + (wm * 16 * MF + fr) * 128;
        const char* sB = smem + cur * STAGE + BM * 128 + (wn * 16 * NF + fr) * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pos = ((ks * 4 + fg) ^ (fr & 7)) * 16;
            V8 af[MF], wf[NF];
#pragma unroll
            for (int i = 0; i < MF; ++i) af[i] = *(const V8*)(sA + i * 16 * 128 + pos);
#pragma unroll
            for (int j = 0; j < NF; ++j) wf[j] = *(const V8*)(sB + j * 16 * 128 + pos);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf[j], af[i], acc[i][j]);
        }
        if (it + 1 < nk) lstore(cur ^ 1);               // the other buffer was last read one barrier ago
        __syncthreads();
    }
    idb_gemm_epilogue<T, MF, NF>(p, smem, acc, m0, n0, tid, wm, wn, fr, fg, kz);
#endif
}

// Epilogue of the persistent variant: same arithmetic as the direct epilogue, but EVERY lane issues exactly one
// buffer_store_dwordx2 per (value) fragment — rows/columns outside the matrix get an out-of-range offset and are
// dropped by the buffer range check — so the store count per wave is a compile-time constant and the K loop can wait
// for the next tile's loads with a counted vmcnt while these stores are still in flight.
template <typename T, int MF, int NF, bool GEGLU>
__device__ __forceinline__ void idb_pl_epilogue(const GemmParams& p, f32x4 (&acc)[MF][NF], const f32x4 (&cb)[NF], const f32x4 (&cu)[NF],
                                                const float2 (&mr)[MF], int m0, int n0, int wm, int wn, int fr, int fg) {
    using V4 = typename Op<T>::v4;
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, IDB_RSRC_FLAGS);
    const bool ln = p.ln_stats != nullptr;              // folded LayerNorm: out = rstd (scale acc - mean u) + v, cb = ln_v, cu = ln_u
    const bool hb = p.bias != nullptr || ln;            // cb holds dummy reads otherwise
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + (wm * MF + i) * 16 + fr;
        const bool mok = m < p.M;
        const int mc = mok ? m : 0;
        const float* sb = p.sbias ? p.sbias + (long long)(mc / p.HW) * p.sbias_ld : nullptr;
        const float rs = ln ? mr[i].y * p.scale : p.scale, kb = ln ? -mr[i].x * mr[i].y : 0.f;
#pragma unroll
        for (int j = 0; j < NF; j += (GEGLU ? 2 : 1)) {
            const int n = n0 + (wn * NF + j) * 16 + fg * 4;               // packed row (value part for GEGLU)
            const int oc = GEGLU ? (n0 + (wn * NF + j) * 16) / 2 + fg * 4 : n;
            const bool nok = GEGLU ? (n + 16 < p.N) : (n < p.N);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = acc[i][j][e] * rs + (ln ? kb * cu[j][e] : 0.f);
            if constexpr (GEGLU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float gt = acc[i][j + 1][e] * rs + (ln ? kb * cu[j + 1][e] : 0.f);
                    o[e] += hb ? cb[j][e] : 0.f;                        // columns past N are never stored
                    gt += hb ? cb[j + 1][e] : 0.f;
                    o[e] *= gelu_erf_f(gt);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += hb ? cb[j][e] : 0.f;
                if (nok && sb) {
                    const f32x4 b4 = *(const f32x4*)(sb + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += b4[e];
                }
                if (p.act == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = gelu_erf_f(o[e]);
                }
                if (p.res && mok && nok) {
                    const V4 r4 = *(const V4*)((const T*)p.res + (long long)m * p.out_ld + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += to_f32<T>(r4[e]);
                }
            }
            const V4 pk = {from_f32<T>(o[0]), from_f32<T>(o[1]), from_f32<T>(o[2]), from_f32<T>(o[3])};
            const unsigned voff = (mok && nok) ? (unsigned)(((long long)m * p.out_ld + oc) * 2) : IDB_OOB;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, pk), rs_o, voff, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// Persistent variant for plain [M][K] x [N][K]^T GEMMs with a SHORT K loop (the K = C projection layers of the
// transformer blocks at large batch: 5-20 K-steps).  A grid of 2 workgroups per CU walks the output tiles; the
// 2-deep LDS ring runs straight across tile boundaries, so the first K tile of output tile t+1 is already in
// flight while tile t's accumulators go through the epilogue, and no workgroup launch / address prologue /
// pipeline fill is paid per tile.  Same fragment layout and epilogue arithmetic as idb_gemm_kernel.
// ------------------------------------------------------------------------------------------------------------
template <typename T, int MF, int NF>
__global__ __launch_bounds__(256, 2) void idb_gemm_kernel_pl(const GemmParams p) {   // 2 waves/SIMD: two workgroups per CU
#if defined(__HIP_DEVICE_COMPILE__)
    using V8 = typename Op<T>::v8;
    constexpr int BM = 32 * MF, BN = 32 * NF, STAGE = (BM + BN) * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    const int tiles_m = (p.M + BM - 1) / BM;
    const int ntiles = tiles_m * p.tiles_n;
    const int G = gridDim.x, KT = p.ktiles;
    // Tiles b, b + G, ...: the 20-80 column tiles of one row tile run on all eight XCDs at once and every L2 fetches that A tile for
    // itself (FETCH_SIZE x 2 = 2.86 GB per launch against 337 MB of operands, GEGLU K = 320 at B_eff 128).  Measured alternative: each XCD
    // owning whole row tiles (its 64 workgroups walking [tm][tn] in order) cut that to 517 MB and was SLOWER — 575 vs 593 TFLOP/s at
    // K = 320, 719 vs 795 at K = 640, 832 vs 922 at K = 1280, batch 64 15.30 vs 15.37 images/s: the re-reads are served by the
    // Infinity Cache, and 64 workgroups pulling the same three A tiles through one L2 at the same moment queue on its channels.
    // Also measured: a 64x128 form with three workgroups per CU (more loads in flight against the one-round-trip K-step): 480 vs 574,
    // 624 vs 756, 676 vs 896 TFLOP/s — half the rows per weight tile costs more than the third workgroup hides.
    if ((int)blockIdx.x >= ntiles) return;
    const int my_tiles = (ntiles - (int)blockIdx.x + G - 1) / G;
    const int total = my_tiles * KT;

    const int lrow = tid >> 3;
    const unsigned cg16 = ((tid & 7) ^ (lrow & 7)) * 16;
    const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)p.src[0].ptr, 0, p.src[0].bytes, IDB_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, IDB_RSRC_FLAGS);
    const unsigned a_row_bytes = (unsigned)p.src[0].C * 2u;        // A is [M][K], K = C of the single 1x1 source

    // load-side cursor: output tile lt, K-step lk
    int lt = blockIdx.x, lk = 0;
    unsigned a_voff[MF], w_voff[NF];
    auto set_tile = [&](int tile) {
        const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int m = tm * BM + i * 32 + lrow;
            a_voff[i] = m < p.M ? (unsigned)m * a_row_bytes + cg16 : IDB_OOB;
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int n = tn * BN + j * 32 + lrow;
            w_voff[j] = n < p.N ? (unsigned)(n >> 4) * p.w_blk_bytes + (unsigned)(n & 15) * p.w_row_bytes + cg16 : IDB_OOB;
        }
    };
    set_tile(lt);
    auto stage = [&](int buf) {
        char* sA = smem + buf * STAGE;
        char* sB = sA + BM * 128;
        const unsigned soff = (unsigned)lk * 128u;
#pragma unroll
        for (int i = 0; i < MF; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, LDS_PTR(sA + (i * 256 + wave * 64) * 16), 16, a_voff[i], soff, 0, 0);
        const unsigned wsoff = (unsigned)lk * p.w_kstep;
#pragma unroll
        for (int j = 0; j < NF; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(sB + (j * 256 + wave * 64) * 16), 16, w_voff[j], wsoff, 0, 0);
        if (++lk == KT) {
            lk = 0;
            lt += G;
            if (lt < ntiles) set_tile(lt);
        }
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int ct = blockIdx.x, ck = 0;        // compute-side cursor
    // bias vectors of this lane's NF fragments, loaded at the FIRST K-step of every output tile (one round trip under the tile's
    // MFMAs): inside the epilogue they sat behind a runtime branch and were awaited one fragment at a time
    f32x4 cb[NF], cu[NF];
    const bool ln = p.ln_stats != nullptr;
    const float* bias_or_dummy = ln ? p.ln_v : (p.bias ? p.bias : (const float*)p.w);
    const bool has_cb = ln || p.bias;
    // folded LayerNorm: the ln_nt partial {sum, sum of squares} of a tile row are split over its four fg lane groups (two loads
    // per lane and row, ln_nt <= 8; more: an accumulating loop), loaded RAW at the tile's first K-step and reduced at the second
    // (behind that step's vmcnt(0) + barrier: no exposed round trip); {mean, rstd} then wait in mr for the epilogue
    float2 sp[MF][2], mr[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) mr[i] = make_float2(0.f, 1.f);
    int stores_in_flight = 0;           // 1 / 2: the previous step ended with an epilogue that issued exactly MF*NF / MF*NF/2 stores
    stage(0);
    for (int st = 0; st < total; ++st) {
        const int cur = st & 1;
        // the next tile's loads are OLDER than the epilogue's stores: a counted wait retires the loads only
        if (stores_in_flight == 1)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(MF * NF) : "memory");
        else if (stores_in_flight == 2)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(MF * NF / 2) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        stores_in_flight = 0;
        if (ln && ck == 1) {                            // the statistics loads of step 0 have landed (vmcnt(0) above)
            const float inv_c = 1.0f / (float)p.ln_c;
#pragma unroll
            for (int i = 0; i < MF; ++i) {
                float a = sp[i][0].x + sp[i][1].x, q = sp[i][0].y + sp[i][1].y;
                a += __shfl_xor(a, 16, 64);
                q += __shfl_xor(q, 16, 64);
                a += __shfl_xor(a, 32, 64);
                q += __shfl_xor(q, 32, 64);
                const float mean = a * inv_c;
                double var = (double)q * (double)inv_c - (double)mean * (double)mean;     // see idb_ln_row_table
                if (var < 0.0) var = 0.0;
                mr[i] = make_float2(mean, __builtin_amdgcn_rsqf((float)var + p.ln_eps));
            }
        }
        if (st + 1 < total) stage(cur ^ 1);
        if (ck == 0) {
            const int tm = ct / p.tiles_n, tn = ct - tm * p.tiles_n;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const int nc = min(tn * BN + (wn * NF + j) * 16 + fg * 4, p.N - 4);
                cb[j] = *(const f32x4*)(bias_or_dummy + (has_cb ? nc : 0));   // raw: first use (and the wait) is in the epilogue
                cu[j] = *(const f32x4*)(ln ? p.ln_u + nc : bias_or_dummy);
            }
            if (ln) {
#pragma unroll
                for (int i = 0; i < MF; ++i) {
                    const int m = min(tm * BM + (wm * MF + i) * 16 + fr, p.M - 1);
                    const float* ps = p.ln_stats + (long long)m * p.ln_nt * 2;
                    if (p.ln_nt <= 8) {
                        const float2 v0 = *(const float2*)(ps + 2 * min(fg, p.ln_nt - 1)), v1 = *(const float2*)(ps + 2 * min(fg + 4, p.ln_nt - 1));
                        sp[i][0] = fg < p.ln_nt ? v0 : make_float2(0.f, 0.f);
                        sp[i][1] = fg + 4 < p.ln_nt ? v1 : make_float2(0.f, 0.f);
                    } else {
                        float a = 0.f, q = 0.f;
                        for (int t = fg; t < p.ln_nt; t += 4) {
                            const float2 v = *(const float2*)(ps + 2 * t);
                            a += v.x;
                            q += v.y;
                        }
                        sp[i][0] = make_float2(a, q);
                        sp[i][1] = make_float2(0.f, 0.f);
                    }
                }
            }
        }
        const char* sA = smem + cur * STAGE + (wm * 16 * MF + fr) * 128;
        const char* sB = smem + cur * STAGE + BM * 128 + (wn * 16 * NF + fr) * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pos = ((ks * 4 + fg) ^ (fr & 7)) * 16;
            V8 af[MF], wf[NF];
#pragma unroll
            for (int i = 0; i < MF; ++i) af[i] = *(const V8*)(sA + i * 16 * 128 + pos);
#pragma unroll
            for (int j = 0; j < NF; ++j) wf[j] = *(const V8*)(sB + j * 16 * 128 + pos);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = Op<T>::mfma16(wf[j], af[i], acc[i][j]);
        }
        if (++ck == KT) {
            const int tm = ct / p.tiles_n, tn = ct - tm * p.tiles_n;
            if (p.geglu) {
                if constexpr ((NF & 1) == 0) {
                    idb_pl_epilogue<T, MF, NF, true>(p, acc, cb, cu, mr, tm * BM, tn * BN, wm, wn, fr, fg);
                    stores_in_flight = 2;
                }
            } else {
                idb_pl_epilogue<T, MF, NF, false>(p, acc, cb, cu, mr, tm * BM, tn * BN, wm, wn, fr, fg);
                stores_in_flight = 1;
            }
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            ck = 0;
            ct += G;
        }
    }
#endif
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {

struct Plan;

// ---- kernel variants ---------------------------------------------------------------------------------
// A tile id (idb_gemm_desc.tile, idb_gemm_plan's `tile`; include/idb_kernels.h) is shape + 10 * family.
struct Shape { int mf, nf, wm; };   // tile = (16*mf*wm) x (32*nf), 128*wm MFMA threads
constexpr Shape kShapes[] = {{0, 0, 2}, {4, 5, 2}, {4, 4, 2}, {2, 5, 2}, {1, 2, 4}, {4, 1, 2},
                             {1, 5, 4}, {1, 4, 4}, {2, 5, 4}, {2, 4, 4}};   // index = shape
// shapes 4 and 6-9 have 8 waves per workgroup (2- or 3-stage ring): 4 = 64x64, 6 = 64x160, 7 = 64x128, 8 = 128x160, 9 = 128x128 — 6-9
// are the tiles 3/-/1/2 with half the LDS-DMA instructions per wave and K-step; 4 exists to put more workgroups on the chip for the
// smallest batch-1 projections (M = 512, N = 1280: 160 instead of 80)
// (a 256x160 tile with 8 waves was measured 3-8 % slower than 128x160 with two workgroups per CU and is not kept).

enum Family {        // = tile id / 10
    kRing2,          // 0: LDS-DMA ring (idb_gemm_kernel), 2 stages
    kRing3,          // 1: 3 stages
    kRing4,          // 2: 4 stages
    kRegStaged,      // 3: register-staged double buffer (idb_gemm_kernel_rs)
    kPersistent,     // 4: persistent, plain [M][K] matrices (idb_gemm_kernel_pl)
    kLw3x4,          // 5: loader-wave variant (idb_gemm_kernel_lw): 4 loader waves + 3-stage ring
    kLw3x8,          // 6: 8 loader waves + 3 stages
    kLw4x4,          // 7: 4 loader waves + 4 stages
    kLw256,          // 8: loader waves with TWICE the rows (shapes 8 / 9 only: 256x160 / 256x128, 8 MFMA waves + 4 loader waves, 3-stage
                     //    ring, one workgroup per CU with all 160 KB of LDS): 97 / 85 FLOP per byte moved L2 -> LDS instead of 73 for large grids
    kPatch256,       // 9: patch-resident 3x3 conv (idb_conv_patch_kernel) on those 256-row tiles
    kPatchSmall,     // 10: patch-resident 3x3 conv on the shape's own 64- / 128-row tile (fused GroupNorm: transforming patch loaders)
};

struct Variant;
using LaunchFn = int (*)(const Variant&, const GemmParams&, const Plan&, hipStream_t);

struct Variant {
    int id;
    Family fam;
    int mf, nf, ns, wm, lw;             // the kernel's template shape (lw: loader waves; the patch kernel's 2 patch + 2 weight loaders)
    int bm, bn, threads, epi_threads;   // tile, workgroup size, threads of the LDS-staged epilogue (the MFMA waves)
    int lds;                            // dynamic LDS bytes
    int gn_lds;                         // fused-GroupNorm twin: its LDS ring (normalizer-wave kernel) / all its LDS (patch kernel); 0: none
    bool xcd_round;                     // the planner rounds a heuristic split-K to one K-slice per XCD (S % 8 == 0 or S == 4)
    bool xcd_slices;                    // the kernel runs the K-slice-per-XCD remap (GemmParams.xcd_mode 1 / 2) when the split allows
    LaunchFn launch[2], launch_gn[2];   // [bf16, f16]; launch_gn: the fused-GroupNorm twin (nullptr: none)
    LaunchFn launch_relu[2];            // the ReLU-epilogue twin (idb_gemm_desc.act = 3): ring and loader-wave families; nullptr: none
};

struct Plan {
    const Variant* v;
    int splitk, tiles_m, tiles_n, ktiles, kt_per_split, M;
    long long K;
};

constexpr int patch_lds(int mf, int nf, int ns, bool gn) {   // two patch buffers + the weight ring (+ group statistics)
    return 2 * (mf == 1 ? (gn ? 224 : 208) : mf == 2 ? (gn ? 288 : 272) : 400) * 128 + ns * 32 * nf * 128 + (gn ? 256 : 0);
}

// fused GroupNorm through normalizer waves: LDS = ring + {k, h} table per normalised channel + group statistics, per sample in the tile
size_t gn_fused_lds(const Variant& v, long long hw, long long cn, int groups) {
    const long long nsamp = v.bm > hw ? v.bm / hw : 1;
    return (size_t)v.gn_lds + (size_t)(nsamp * cn * 8) + (size_t)(nsamp * groups * 8);
}

// Launch of a kernel whose launch scalars stand in front of GemmParams as plain parameters (GemmTile, idb_gemm_epi.h)
template <auto K>
static int idb_launch_tile(const char* api, const char* name, dim3 grid, dim3 block, size_t lds, int lds_max, hipStream_t st, const GemmParams& p, int tiles) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (e != hipSuccess) {
            idb_set_error("%s: hipFuncSetAttribute(%d) failed: %s", api, lds_max, hipGetErrorString(e));
            return IDB_EHIP;
        }
        attr_done = true;
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, IDB_TILE_ARGS(p, tiles), p);
    IDB_CHECK_LAUNCH(name);
    return IDB_OK;
}

template <typename T, Family F, int MF, int NF, int NS, int WM, int LW, bool GN, bool RELU = false>
int launch_variant(const Variant& v, const GemmParams& p, const Plan& pl, hipStream_t st) {
    const int tiles = pl.tiles_m * pl.tiles_n;
    const dim3 grid(tiles, 1, pl.splitk);
    if constexpr (GN && F == kPatchSmall) {
        return idb_launch_tile<idb_conv_patch_kernel<T, MF, NF, NS, true>>("idb_gemm", "idb_gemm(patch)", grid, dim3(896), v.gn_lds, v.gn_lds, st, p, tiles);
    } else if constexpr (GN) {
        // 4 MFMA waves (2 x 2, one per SIMD: the wave tile is twice that of the 8-wave kernels of the same workgroup tile) + 4 loader waves +
        // 8 normalizer waves = 16 waves: with 4 normalizer waves the transform (9x redundant for a 3x3 conv: every tap re-reads its pixels)
        // was the K-step's critical path — 50 vs 34 us on conv 320->320 @64x64 at B_eff 2.  64-row tiles only, 4-stage ring: a 4-wave MFMA
        // role needs > 128 VGPRs on 128-row tiles (16 waves per workgroup)
        const size_t lds = gn_fused_lds(v, p.HW, p.gn_in_c, p.gn_in_groups);
        if (lds > 160 * 1024) {
            idb_set_error("idb_gemm: fused GroupNorm needs %zu bytes of LDS for this tile", lds);
            return IDB_EUNSUPPORTED;
        }
        return idb_launch_tile<idb_gemm_kernel_gn<T, 2, NF, 4, 2, 8>>("idb_gemm", "idb_gemm(gn)", grid, dim3(128 * 2 + 256 + 64 * 8), lds, 160 * 1024, st, p, tiles);
    } else if constexpr (F <= kRing4 && RELU) {
        return idb_launch_tile<idb_gemm_kernel_relu<T, MF, NF, NS, WM>>("idb_gemm", "idb_gemm(relu)", grid, dim3(v.threads), v.lds, v.lds, st, p, tiles);
    } else if constexpr (F <= kRing4) {
        return idb_launch_tile<idb_gemm_kernel<T, MF, NF, NS, WM>>("idb_gemm", "idb_gemm", grid, dim3(v.threads), v.lds, v.lds, st, p, tiles);
    } else if constexpr (F == kRegStaged) {
        return idb_launch<idb_gemm_kernel_rs<T, MF, NF>>("idb_gemm", "idb_gemm(rs)", grid, dim3(v.threads), v.lds, v.lds, st, p);
    } else if constexpr (F == kPersistent) {
        return idb_launch<idb_gemm_kernel_pl<T, MF, NF>>("idb_gemm", "idb_gemm(pl)", dim3(tiles < 512 ? tiles : 512), dim3(v.threads), v.lds, v.lds, st, p);
    } else if constexpr (F <= kLw256 && RELU) {
        return idb_launch_tile<idb_gemm_kernel_lw_relu<T, MF, NF, NS, WM, LW>>("idb_gemm", "idb_gemm(lw, relu)", grid, dim3(v.threads), v.lds, v.lds, st, p, tiles);
    } else if constexpr (F <= kLw256) {
        return idb_launch_tile<idb_gemm_kernel_lw<T, MF, NF, NS, WM, LW>>("idb_gemm", "idb_gemm(lw)", grid, dim3(v.threads), v.lds, v.lds, st, p, tiles);
    } else {
        return idb_launch_tile<idb_conv_patch_kernel<T, MF, NF, NS>>("idb_gemm", "idb_gemm(patch)", grid, dim3(v.threads), v.lds, v.lds, st, p, tiles);
    }
}

template <Family F, int S>
constexpr Variant variant() {
    constexpr Shape s = kShapes[S];
    constexpr int MF = F == kLw256 || F == kPatch256 ? 2 * s.mf : s.mf, NF = s.nf, WM = s.wm;
    constexpr int NS = F <= kRing4 ? 2 + F : F == kRegStaged || F == kPersistent ? 2 : F == kLw4x4 || F == kPatchSmall ? 4 : 3;
    constexpr int LW = F == kLw3x8 ? 8 : F >= kLw3x4 ? 4 : 0;
    constexpr int BM = 16 * MF * WM, BN = 32 * NF;
    constexpr int RS = F >= kLw3x4 ? 8 * LW : 16 * WM;                      // tile rows per staging sweep (weight rows rounded up to it)
    constexpr int LDS = F >= kPatch256 ? patch_lds(MF, NF, NS, false) : (BM + (BN + RS - 1) / RS * RS) * 128 * NS;
    constexpr bool gn = F == kPatchSmall || (F >= kLw3x4 && F <= kLw4x4 && BM == 64);
    constexpr int GN_LDS = !gn ? 0 : F == kPatchSmall ? patch_lds(MF, NF, NS, true) : (BM + (BN + 31) / 32 * 32) * 128 * 4;
    static_assert(LDS <= 160 * 1024 && GN_LDS <= 160 * 1024, "LDS does not fit");
    constexpr bool ring_or_lw = F <= kRing3 || F >= kLw3x4;
    LaunchFn gn_bf16 = nullptr, gn_f16 = nullptr, relu_bf16 = nullptr, relu_f16 = nullptr;
    if constexpr (gn) {
        gn_bf16 = launch_variant<__bf16, F, MF, NF, NS, WM, LW, true>;
        gn_f16 = launch_variant<_Float16, F, MF, NF, NS, WM, LW, true>;
    }
    if constexpr (F <= kRing4 || (F >= kLw3x4 && F <= kLw256)) {
        relu_bf16 = launch_variant<__bf16, F, MF, NF, NS, WM, LW, false, true>;
        relu_f16 = launch_variant<_Float16, F, MF, NF, NS, WM, LW, false, true>;
    }
    return {S + 10 * F, F, MF, NF, NS, WM, LW, BM, BN, 128 * WM + 64 * LW, 128 * WM, LDS, GN_LDS, ring_or_lw && WM == 4, ring_or_lw && S != 5,
            {launch_variant<__bf16, F, MF, NF, NS, WM, LW, false>, launch_variant<_Float16, F, MF, NF, NS, WM, LW, false>}, {gn_bf16, gn_f16},
            {relu_bf16, relu_f16}};
}

constexpr Variant kVariants[] = {
    variant<kRing2, 1>(), variant<kRing2, 2>(), variant<kRing2, 3>(), variant<kRing2, 4>(), variant<kRing2, 5>(),
    variant<kRing2, 6>(), variant<kRing2, 7>(), variant<kRing2, 8>(), variant<kRing2, 9>(),
    variant<kRing3, 1>(), variant<kRing3, 2>(), variant<kRing3, 3>(), variant<kRing3, 4>(),
    variant<kRing3, 6>(), variant<kRing3, 7>(), variant<kRing3, 8>(), variant<kRing3, 9>(),
    variant<kRing4, 1>(), variant<kRing4, 2>(), variant<kRing4, 3>(),
    variant<kRegStaged, 1>(), variant<kRegStaged, 2>(), variant<kRegStaged, 3>(), variant<kRegStaged, 5>(),
    variant<kPersistent, 1>(), variant<kPersistent, 2>(),
    variant<kLw3x4, 4>(), variant<kLw3x4, 6>(), variant<kLw3x4, 7>(), variant<kLw3x4, 8>(), variant<kLw3x4, 9>(),
    variant<kLw3x8, 4>(), variant<kLw3x8, 6>(), variant<kLw3x8, 7>(), variant<kLw3x8, 8>(), variant<kLw3x8, 9>(),
    variant<kLw4x4, 4>(), variant<kLw4x4, 6>(), variant<kLw4x4, 7>(), variant<kLw4x4, 8>(), variant<kLw4x4, 9>(),
    variant<kLw256, 8>(), variant<kLw256, 9>(),
    variant<kPatch256, 8>(), variant<kPatch256, 9>(),
    variant<kPatchSmall, 4>(), variant<kPatchSmall, 6>(), variant<kPatchSmall, 7>(), variant<kPatchSmall, 8>(), variant<kPatchSmall, 9>(),
};

const Variant* find_variant(int id) {   // nullptr: no such variant
    for (const Variant& v : kVariants)
        if (v.id == id) return &v;
    return nullptr;
}

// ---- A/B switches for measurements: read once per process ---------------------------------------------
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

struct PlanEnv {
    int plan_ab = env_int("IDB_GEMM_PLAN_AB", 0);                  // bits: 1 keeps 64x128 over 64x64, 2 / 4 move two 128-row thresholds
    int patch_shortcut = env_int("IDB_CONV_PATCH_SHORTCUT", 0);
    int ring_small_m = env_int("IDB_GEMM_RING_SMALL_M", 2);
    int ring_m = env_int("IDB_GEMM_RING_M", 2048);
    int regstage = env_int("IDB_GEMM_REGSTAGE", 0);
    int persist = env_int("IDB_GEMM_PERSIST", 1);
    int pl_geglu_tiles = env_int("IDB_GEMM_PL_GEGLU_TILES", 512);
    int lw = env_int("IDB_GEMM_LW", 7);
    int big_tiles = env_int("IDB_GEMM_BIG_TILES", 512);
    int patch = env_int("IDB_CONV_PATCH", 1);
    int patch_small = env_int("IDB_CONV_PATCH_SMALL", 0);
    int xcd_slices = env_int("IDB_GEMM_XCD_SLICES", 1);
    int pl_ln = env_int("IDB_GEMM_PL_LN", 0);
    int gn_tapmajor = env_int("IDB_GN_TAPMAJOR", 0);
    int fused_reduce = env_int("IDB_GEMM_FUSED_REDUCE", 0);
};

const PlanEnv& plan_env() {
    static const PlanEnv env;
    return env;
}

// idb_conv_patch_kernel's shapes: whole tiles of bm (64 / 128 / 256) output pixels that are whole image rows (or whole images), every
// K segment on the output grid; the halo patch of one tile fits the kernel's patch buffer (208 / 272 / 400 pixels)
static bool conv_patch_ok(const idb_gemm_desc* d, long long M, int bm) {
    if (d->stride != 1 || d->pad_mode == 1 || d->geglu || d->ln_stats || d->nsrc < 1 || d->src[0].taps != 9 || d->act) return false;
    const int W = d->out_w, H = d->out_h;
    if (!(W == 8 || W == 16 || W == 32 || W == 64) || W > bm || M % bm) return false;
    const long long HW = (long long)H * W;
    if (!(HW % bm == 0 || bm % HW == 0)) return false;
    const int nimg = HW >= bm ? 1 : (int)(bm / HW);
    if (nimg * (bm / W / nimg + 2) * (W + 2) > (bm == 64 ? 208 : bm == 128 ? 272 : 400)) return false;
    if (d->gn_in_partials) {
        // fused GroupNorm (transforming patch loaders): small tiles inside ONE sample, every K segment a normalised 3x3 source
        if (bm > 128 || HW < bm || d->gn_in_nsrc != d->nsrc || d->gn_in_groups <= 0 || d->gn_in_groups > 32 || d->gn_in_chunks < 1 || d->gn_in_chunks > 64) return false;
        long long cn = 0;
        for (int s = 0; s < d->nsrc; ++s) {
            if (d->src[s].taps != 9) return false;
            cn += d->src[s].channels;
        }
        if (cn % d->gn_in_groups) return false;
    }
    // 1x1 K segments (a fused conv_shortcut) run through the patch buffers with ONE K-step per chunk, i.e. on a two-deep pipeline:
    // auto plans take the patch kernel for pure 3x3 convs only unless IDB_CONV_PATCH_SHORTCUT=1 (forced tile ids run every mix)
    for (int s = 0; s < d->nsrc; ++s) {
        if (d->src[s].upsample || d->src[s].in_h != H || d->src[s].in_w != W || d->src[s].channels % 64) return false;
        if (d->src[s].taps != 9 && d->tile == 0 && !plan_env().patch_shortcut) return false;
    }
    return true;
}

int plan_gemm(const idb_gemm_desc* d, Plan* pl) {
    IDB_REQUIRE(d != nullptr, "idb_gemm: null descriptor");
    IDB_REQUIRE(idb_is_operand_dtype(d->dtype), "idb_gemm: dtype must be bf16 or f16 (got %d)", d->dtype);
    IDB_REQUIRE(d->batch > 0 && d->out_h > 0 && d->out_w > 0 && d->n > 0, "idb_gemm: non-positive dims");
    IDB_REQUIRE(d->stride == 1 || d->stride == 2, "idb_gemm: stride must be 1 or 2");
    IDB_REQUIRE(d->pad_mode == 0 || (d->pad_mode == 1 && d->stride == 2), "idb_gemm: pad_mode must be 0, or 1 with stride 2");
    if (d->gn_partials) {
        const long long hw = (long long)d->out_h * d->out_w;
        IDB_REQUIRE(d->gn_groups > 0 && d->n % d->gn_groups == 0 && d->n / d->gn_groups >= 2 && !d->geglu && d->out_dtype == d->dtype &&
                        hw % 64 == 0 && hw <= 4096 && d->out_ld == d->n && idb_aligned16(d->gn_partials),
                    "idb_gemm: gn_partials needs n %% gn_groups == 0, dense operand-dtype output, no GEGLU, out_h*out_w %% 64 == 0 and <= 4096");
    }
    IDB_REQUIRE(d->nsrc >= 1 && d->nsrc <= IDB_MAX_SRC, "idb_gemm: nsrc out of range");
    IDB_REQUIRE(d->out_dtype == d->dtype || d->out_dtype == IDB_F32, "idb_gemm: out_dtype must be dtype or f32");
    const long long M = (long long)d->batch * d->out_h * d->out_w;
    IDB_REQUIRE(M < (1LL << 31), "idb_gemm: M too large");
    long long K = 0;
    for (int s = 0; s < d->nsrc; ++s) {
        const idb_gemm_src& S = d->src[s];
        IDB_REQUIRE(S.ptr != nullptr && idb_aligned16(S.ptr), "idb_gemm: src[%d] pointer null or not 16-byte aligned", s);
        IDB_REQUIRE(S.channels > 0 && S.channels % 64 == 0, "idb_gemm: src[%d].channels=%d must be a multiple of 64", s, S.channels);
        IDB_REQUIRE(S.taps == 9 || S.taps == 1, "idb_gemm: src[%d].taps must be 9 or 1", s);
        IDB_REQUIRE(S.upsample == 0 || S.upsample == 1, "idb_gemm: src[%d].upsample must be 0/1", s);
        IDB_REQUIRE(S.in_h > 0 && S.in_w > 0, "idb_gemm: src[%d] spatial dims", s);
        const int lh = S.in_h << S.upsample, lw = S.in_w << S.upsample;
        if (S.taps == 9) {
            IDB_REQUIRE(d->out_h == (lh + d->stride - 1) / d->stride && d->out_w == (lw + d->stride - 1) / d->stride,
                        "idb_gemm: src[%d] %dx%d (up=%d, stride=%d) does not produce %dx%d", s, S.in_h, S.in_w,
                        S.upsample, d->stride, d->out_h, d->out_w);
        } else if (d->stride == 2 && d->pad_mode == 0 && S.upsample == 0 && (lh != d->out_h || lw != d->out_w)) {
            // 1x1 source at stride 2 (a strided shortcut beside a stride-2 3x3 source): output pixel (oy, ox) reads (2 oy, 2 ox)
            IDB_REQUIRE(d->out_h == (lh + 1) / 2 && d->out_w == (lw + 1) / 2,
                        "idb_gemm: stride-2 1x1 src[%d] %dx%d does not produce %dx%d", s, S.in_h, S.in_w, d->out_h, d->out_w);
        } else {
            IDB_REQUIRE(d->stride == 1 && lh == d->out_h && lw == d->out_w,
                        "idb_gemm: 1x1 src[%d] must match the output grid", s);
        }
        K += (long long)S.taps * S.channels;
        IDB_REQUIRE((long long)d->batch * S.in_h * S.in_w * S.channels * 2 < (1LL << 31),
                    "idb_gemm: src[%d] tensor is >= 2 GiB; split the batch", s);
    }
    IDB_REQUIRE(d->w && idb_aligned16(d->w) && d->out && idb_aligned16(d->out), "idb_gemm: w/out null or unaligned");
    IDB_REQUIRE(d->out_ld >= (d->geglu ? d->n / 2 : d->n), "idb_gemm: out_ld too small");
    if (d->geglu) {
        IDB_REQUIRE(d->n % 32 == 0 && d->out_dtype == d->dtype && !d->residual && !d->sample_bias,
                    "idb_gemm: GEGLU needs n %% 32 == 0, operand-dtype output, no residual/sample_bias");
        IDB_REQUIRE(d->out_ld % 4 == 0, "idb_gemm: GEGLU out_ld must be a multiple of 4");
    }
    if (d->n % 4 == 0) IDB_REQUIRE(d->out_ld % 4 == 0, "idb_gemm: out_ld must be a multiple of 4 when n is");
    IDB_REQUIRE(d->act == 0 || d->act == 2 || ((d->act == 1 || d->act == 3) && !d->geglu && !d->residual),
                "idb_gemm: act must be 0, 2, or 1 (GELU) / 3 (ReLU) without GEGLU/residual");
    if (d->act == 3) IDB_REQUIRE(!d->gn_partials && !d->gn_in_partials, "idb_gemm: act 3 (ReLU) is not combined with gn_partials / gn_in_partials");
    if (d->act == 2)
        IDB_REQUIRE(d->act_slope && idb_aligned16(d->act_slope) && !d->geglu && !d->residual && !d->ln_stats && !d->gn_in_partials &&
                        !d->gn_partials && d->n % 4 == 0,
                    "idb_gemm: act 2 (PReLU) needs a 16-byte aligned act_slope, n %% 4 == 0, and no residual / GEGLU / LayerNorm / GroupNorm fold / gn_partials");
    if (d->out2 || d->out2_scale || d->out2_shift)
        IDB_REQUIRE(d->out2 && d->out2_scale && d->out2_shift && idb_aligned16(d->out2) && idb_aligned16(d->out2_scale) &&
                        idb_aligned16(d->out2_shift) && d->out_dtype == d->dtype && !d->geglu && !d->gn_partials && !d->row_stats_out &&
                        !d->ln_stats && !d->gn_in_partials && d->n % 4 == 0,
                    "idb_gemm: out2 needs 16-byte aligned out2, out2_scale and out2_shift, operand-dtype output, n %% 4 == 0, and no GEGLU / "
                    "gn_partials / row_stats_out / LayerNorm / GroupNorm fold");
    if (d->act == 2 || d->out2)
        IDB_REQUIRE(d->out_dtype == d->dtype && (!d->bias || idb_aligned16(d->bias)) && (!d->residual || ((uintptr_t)d->residual & 7) == 0) &&
                        (!d->sample_bias || (idb_aligned16(d->sample_bias) && d->sample_bias_ld % 4 == 0)),
                    "idb_gemm: act 2 / out2 need operand-dtype output, a 16-byte aligned bias / sample_bias (ld %% 4 == 0), an 8-byte aligned residual");
    if (d->sample_bias) IDB_REQUIRE(d->sample_bias_ld == 0 || d->sample_bias_ld >= d->n, "idb_gemm: sample_bias_ld must be 0 (broadcast) or >= n");

    IDB_REQUIRE(((long long)d->n + 15) / 16 * 16 * K * 2 < (1LL << 31), "idb_gemm: weight matrix is >= 2 GiB");
    IDB_REQUIRE(d->w_layout == 0 || d->w_layout == 1, "idb_gemm: w_layout must be 0 (rows) or 1 (idb_tile_weight)");
    pl->M = (int)M;
    pl->K = K;
    pl->ktiles = (int)(K / 64);
    // PReLU / second output: applied by the reduce launch of a split-K plan (idb_splitk_reduce_ex_kernel), so the GEMM kernels keep
    // their epilogues (and register budgets) as they are
    const bool ex = d->act == 2 || d->out2;
    IDB_REQUIRE(!ex || pl->ktiles >= 2, "idb_gemm: act 2 / out2 need K >= 128 (they run on a split-K plan)");
    const Variant* v = find_variant(d->tile);                // forced tile id; 0: chosen by the rules below
    IDB_REQUIRE(d->tile == 0 || v, "idb_gemm: tile id out of range");
    const bool plain = d->nsrc == 1 && d->src[0].taps == 1 && d->src[0].in_h == 1 && d->src[0].in_w == 1;
    const bool pl_ok = plain && d->split_k <= 1 && d->out_dtype == d->dtype && (d->geglu ? d->n / 2 : d->n) % 4 == 0 && d->act != 2 && d->act != 3 && !d->out2 &&
                       d->out_ld % 4 == 0 && M * d->out_ld * 2 < (1LL << 31);
    IDB_REQUIRE(!v || v->fam != kPersistent || pl_ok, "idb_gemm: the persistent variant needs one plain [M][K] source, operand-dtype output < 2 GiB, no split-K");
    const PlanEnv& env = plan_env();
    int auto_sk = 0;                                    // split-K chosen together with the tile (0: by the rules below)
    if (!v) {
        int tile = 0, fam = kRing2;                     // shape and family of the plan
        const bool n160 = (d->n % 160 == 0) && !d->geglu;
        const int bn = d->n <= 32 ? 32 : (n160 ? 160 : 128);
        const long long blocks_big = ((M + 127) / 128) * ((d->n + bn - 1) / bn);
        const long long blocks64 = ((M + 63) / 64) * ((d->n + 127) / 128);
        // measured on MI355X with HBM-cold operands inside a HIP graph (tools/bench_conv.py, tools/bench_small.py; warm
        // back-to-back timings rank the variants differently and mislead):
        //  * >= 2 workgroups per CU: 128-row 8-wave tiles, 2-deep ring (two co-resident workgroups hide each other's latency);
        //  * at most ONE workgroup per CU (the whole batch-1 UNet): the K-step of a lone workgroup is the issue time of its
        //    LDS-DMA instructions plus one memory round trip (tools/bench_latency.py: unchanged with the MFMAs removed), so
        //    8 waves (half the DMA instructions per wave) and a 3-deep ring (two K-steps in flight): -25...-45 % per launch;
        //  * long K (convs, the big FF projections): 128x160 ring-3 tile, split-K to one workgroup per CU (256 / blocks; 384
        //    blocks = 1.5 rounds is worse than 256 or 512), at least 8 K-steps per split; if that cannot fill half the chip
        //    (M = 128) the 64x128 ring-3 tile with the same rule;
        //  * short K: 64-row ring-3 tiles, split only for tiny grids (the reduce launch costs more than a short K loop).
        const bool short_k = pl->ktiles <= 10;
        const bool lin = d->nsrc == 1 && d->src[0].taps == 1;          // a plain linear / 1x1 conv
        bool keep7 = false;                                            // a measured 64x128 plan: not narrowed to 64x64 below
        if (d->n <= 32) tile = 5;
        else if (d->geglu && blocks_big >= 256) tile = pl->ktiles >= 16 ? 2 : 9;   // N = 8C, no split-K: 128-row (persistent form for K >= 1024)
        else if (blocks_big >= (env.plan_ab & 2 ? 512 : 384)) tile = n160 ? 8 : 9;   // measured at batch 3 (384 workgroups): +6 % over the 64-row tiles; at 256 (batch 2): -1.4 %
        // (the 4-wave 128x160 tile reads 9 instead of 14 ds_read_b128 per 20 MFMAs and is 2-5 % faster on every long-K conv with
        //  M >= 32,768 in tools/bench_conv.py at B_eff 128 — end to end it changed nothing: batch 64 15.39 vs 15.32-15.35, batch 8 / 16
        //  -0.3 %; not adopted)
        else if (!d->geglu && pl->ktiles >= 32 && blocks_big <= (env.plan_ab & 4 ? 255 : 256)) {   // = 256 (batch 2, 64x64 level): 37.7 vs 49.8 us
            int sk = (int)(256 / blocks_big);
            const int cap = pl->ktiles / 8;
            if (sk > cap) sk = cap;
            if (sk > 32) sk = 32;
            if (sk < 1) sk = 1;
            if (M <= 128 && M > 64) {
                // ONE 128-row tile of rows (the 8x8 level at batch 1): two 64-row tiles with half the split reach 256 workgroups where the
                // 128-row plan stops at 192, and their slabs are half as many — conv 1280->1280 @8x8 21.7 -> 19.0 us, 2560->1280 26.2 -> 26.0
                // (tools/bench_conv.py 2); a 64-row tile also lies inside one 8x8 sample, so the GroupNorm in front of it can fuse
                tile = n160 ? 6 : 7;
                const long long b64 = 2 * ((d->n + 32 * kShapes[tile].nf - 1) / (32 * kShapes[tile].nf));
                sk = (int)(256 / b64);
                if (sk > cap) sk = cap;
                if (sk > 32) sk = 32;
                auto_sk = sk < 1 ? 1 : sk;
            } else if (blocks_big * sk >= 128) {
                tile = n160 ? 8 : 9;
                auto_sk = sk;
                if (n160 && sk == 2 && pl->ktiles < 64) { tile = 6; auto_sk = 1; }   // 64x160: the same 256 workgroups without a reduce launch
                else if (lin && sk <= 4 && pl->ktiles <= 48 && blocks64 >= 128 && blocks64 <= 256) {
                    // a short split of a plain linear: 64x128 tiles fill more than half the chip without one — FF-out at 32x32 (M = 2048, N = 640,
                    // K = 2560): 22.3 -> 16.7 us incl. the reduce launch it no longer needs (tools/bench_small.py)
                    tile = 7;
                    auto_sk = 1;
                    keep7 = true;
                }
            } else {
                tile = 7;
                sk = (int)(256 / blocks64);
                if (sk > cap) sk = cap;
                if (sk > 32) sk = 32;
                auto_sk = sk < 1 ? 1 : sk;
            }
            fam = kRing3;
        }
        else if (short_k && M >= 4096) { tile = (n160 && blocks_big < 256) ? 6 : 9; fam = tile == 6 ? kRing3 : kRing2; }
        else if (lin && short_k && M < 4096 && ((M + 127) / 128) * ((d->n + 127) / 128) >= 128 && ((M + 127) / 128) * ((d->n + 127) / 128) <= 256) {
            // QKV at 32x32 (M = 2048, N = 1920, K = 640): 240 workgroups of 128x128 with loader waves instead of 480 of 64x128 two per CU:
            // 13.9 -> 12.5 us (tools/bench_small.py)
            tile = 9;
            fam = kRing3;
        }
        else if (lin && n160 && pl->ktiles >= 16 && M >= 4096 && ((M + 63) / 64) * (d->n / 160) <= 256) {
            // FF-out at 64x64 (M = 8192, N = 320, K = 1280): 256 workgroups of 64x160 with loader waves instead of 384 of 64x128 two per CU:
            // 17.9 -> 14.1 us (tools/bench_small.py)
            tile = 6;
            fam = kRing3;
        }
        else tile = (n160 && pl->ktiles >= 32) ? (M >= 4096 ? 6 : 3) : 7;
        if (tile == 7 && blocks64 <= 256) fam = kRing3;
        if (tile == 7 && blocks64 <= 160 && !d->geglu && !(env.plan_ab & 1) && !keep7) tile = 4;   // 64x64: twice the workgroups (m=512 n=1280 k=1280: 12.6 -> 9.9 us)
        const bool lw_shape = tile == 4 || tile >= 6;                  // the 8-wave shapes: loader-wave and 256-row forms exist
        // weight-bound layers stream cold weights from HBM once per launch: a deeper ring keeps more loads in flight
        if (tile != 5 && M <= env.ring_m && env.ring_small_m >= 3 && env.ring_small_m <= 4) fam = env.ring_small_m - 2;
        if (env.regstage) fam = kRegStaged;
        const long long tiles = ((M + 127) / 128) * ((d->n + (32 * kShapes[tile].nf) - 1) / (32 * kShapes[tile].nf));
        // measured: +12-15 % on the GEGLU projections (N = 8C, K = C), neutral or slightly negative on the other K = C layers
        if (env.persist && pl_ok && d->geglu && tile == 2 && pl->ktiles <= 24 && tiles >= 256 && d->split_k <= 1) fam = kPersistent;
        // with the bias vectors loaded at the tile's first K-step (round 2) the persistent form also wins the SHORT-K GEGLU
        // projections once the grid is many rounds deep: K = 320: 593 vs 529 TFLOP/s, K = 640: 795 vs 637 (B_eff = 128,
        // tools/bench_proj.py).  It cannot fold the LayerNorm (ln_stats -> IDB_EUNSUPPORTED, the caller keeps idb_layernorm); end
        // to end with that launch back: batch 64 14.76 -> 15.12, batch 8 13.63 -> 13.87, batch 1 6.44 -> 6.52 images/s
        if (env.persist && pl_ok && d->geglu && tile == 9 && env.pl_geglu_tiles > 0 && tiles >= env.pl_geglu_tiles && d->split_k <= 1) { tile = 2; fam = kPersistent; }
        if (fam == kRing3 && lw_shape) {
            // one workgroup per CU (ring-3 plans): loader waves take the DMA issue and the waits off the MFMA waves (idb_gemm_kernel_lw)
            // measured (tools/bench_lw.py, B_eff 2, cold weights in a HIP graph): conv 320->320 @64x64 31.3 -> 23.7 us, the other convs of the
            // 64x64 / 32x32 levels -5...-10 %, weight-streaming 16x16 / 8x8 layers and short-K linears 0...-3 %; 4 loader waves with a
            // 4-stage ring (7) >= 4 with 3 stages (5) >= 8 with 3 stages (6); end to end batch 1 +1.1 %.  IDB_GEMM_LW=0: ring-3 kernels
            if (env.lw >= kLw3x4 && env.lw <= kLw4x4) fam = env.lw;
        }
        if (fam == kRing2 && (tile == 8 || tile == 9) && !d->geglu && pl->ktiles >= 20) {
            // large grids, K >= 1280: 256-row loader-wave tiles once the 256-row grid is still >= IDB_GEMM_BIG_TILES workgroups (two rounds of
            // the chip; 0 = off).  Measured at B_eff 128 (tools/bench_conv.py / bench_proj.py): every 3x3 conv +8...+19 % (1.01-1.17 ->
            // 1.08-1.32 PFLOP/s), K >= 1280 projections +3...+15 %, K = 640 equal, K = 320 -19 % (excluded); batch 64 end to end +4.1 %
            const long long blocks256 = ((M + 255) / 256) * ((d->n + 32 * kShapes[tile].nf - 1) / (32 * kShapes[tile].nf));
            if (env.big_tiles > 0 && blocks256 >= env.big_tiles) fam = kLw256;
            // 3x3 stride-1 convs on that plan: the patch-resident form (idb_conv_patch_kernel).  IDB_CONV_PATCH=0: tap-major 256-row tiles
            if (fam == kLw256 && env.patch && d->split_k <= 1 && !ex && conv_patch_ok(d, M, 256)) fam = kPatch256;
        }
        // the same for the one-workgroup-per-CU plans (64- / 128-row tiles, split-K by whole chunks): IDB_CONV_PATCH_SMALL=1
        if (fam >= kLw3x4 && fam <= kLw4x4 && !d->geglu && (env.patch_small || d->gn_in_partials) &&
            conv_patch_ok(d, M, 16 * kShapes[tile].mf * kShapes[tile].wm))
            fam = kPatchSmall;
        v = find_variant(tile + 10 * fam);
        IDB_REQUIRE(v, "idb_gemm: the A/B switches chose tile %d, which is not built", tile + 10 * fam);
    }
    if (d->geglu) IDB_REQUIRE(v->nf % 2 == 0, "idb_gemm: GEGLU needs an even-NF tile");
    IDB_REQUIRE(d->act != 3 || v->launch_relu[0], "idb_gemm: act 3 (ReLU) runs on the LDS-ring and loader-wave tiles only (tile %d)", v->id);
    IDB_REQUIRE(!ex || (v->fam != kPersistent && v->fam != kPatch256), "idb_gemm: act 2 / out2 need a split-K capable tile (not the persistent or 256-row patch-resident variant)");
    if ((v->fam == kPatch256 && !(d->split_k <= 1 && conv_patch_ok(d, M, 256))) || (v->fam == kPatchSmall && !conv_patch_ok(d, M, v->bm))) {
        idb_set_error("idb_gemm: tile %d (patch-resident conv) needs a 3x3 stride-1 pad-1 first source, 1x1 / 3x3 sources on the output grid without "
                      "upsampling, out_w in {8,16,32,64}, whole tiles of 256 pixels, no folded LayerNorm / fused GroupNorm / GEGLU / split-K", d->tile);
        return IDB_EUNSUPPORTED;
    }
    pl->v = v;
    pl->tiles_m = (int)((M + v->bm - 1) / v->bm);
    pl->tiles_n = (d->n + v->bn - 1) / v->bn;
    const long long blocks = (long long)pl->tiles_m * pl->tiles_n;
    IDB_REQUIRE(blocks < (1LL << 31), "idb_gemm: grid too large");
    int sk = d->split_k;
    if (sk <= 0) {
        sk = 1;
        if (auto_sk) {
            sk = auto_sk;
        } else if (!d->geglu && v->bm <= 64 && blocks < 96 && pl->ktiles >= 10) {
            // measured (tools/bench_small.py): with the 3-deep ring a short K loop is cheaper than a split + reduce launch
            // unless the grid is tiny (M = 128)
            sk = (int)((160 + blocks - 1) / blocks);
            const int max_by_k = pl->ktiles / (blocks >= 64 ? 16 : 5);
            if (sk > max_by_k) sk = max_by_k;
            if (sk > 32) sk = 32;
            if (sk < 1) sk = 1;
        } else if (!d->geglu && v->bm > 64 && blocks < 192 && pl->ktiles >= 10) {
            sk = (int)((384 + blocks - 1) / blocks);
            const int max_by_k = pl->ktiles / 8;
            if (sk > max_by_k) sk = max_by_k;
            if (sk > 32) sk = 32;
            if (sk < 1) sk = 1;
        }
    }
    if (v->fam == kPersistent || v->fam == kPatch256) sk = 1;
    IDB_REQUIRE(!(d->geglu && sk > 1), "idb_gemm: GEGLU does not support split-K");
    if (d->act == 1 || d->act == 2) sk = 1;   // act 3 (ReLU) keeps its split: the reduce launch applies it after the sum
    if (ex && sk < 2) sk = 2;          // act 2 / out2: the reduce launch applies them
    if (sk > pl->ktiles) sk = pl->ktiles;
    if (sk < 1) sk = 1;
    if (d->split_k <= 0 && !(d->flags & 16) && v->xcd_round && env.xcd_slices) {
        // one K-slice per XCD (kernel remap modes 1/2) needs S % 8 == 0 or S == 4: round the heuristic's choice
        if (sk > 8) {
            const int up = ((sk + 7) / 8) * 8;
            sk = (up <= 32 && up * 6 <= pl->ktiles) ? up : (sk / 8) * 8;
        } else if (sk >= 5) {
            sk = (8 * 6 <= pl->ktiles) ? 8 : 4;
        }
    }
    pl->splitk = sk;
    pl->kt_per_split = (pl->ktiles + sk - 1) / sk;
    return IDB_OK;
}

// the LDS-staged coalesced epilogue runs (`reduced`: the launch writes final outputs, not split-K slabs)
static bool lds_epilogue_runs(const idb_gemm_desc* d, const Variant& v, bool reduced) {
    const int no = d->geglu ? d->n / 2 : d->n;
    return v.fam != kPersistent && d->out_dtype == d->dtype && reduced && no % 8 == 0 && d->out_ld % 8 == 0 && !(d->flags & 4) &&
           (!d->residual || idb_aligned16(d->residual));
}

// ... and can emit row statistics / fold a LayerNorm (not the register-staged kernel's)
static bool gemm_uses_lds_epilogue(const idb_gemm_desc* d, const Plan& pl) {
    return pl.v->fam != kRegStaged && lds_epilogue_runs(d, *pl.v, pl.splitk == 1);
}

// Split-K tail of the PReLU / second-output plans (idb_gemm_desc.act = 2, out2; ArcFace IResNet blocks): one thread per output row and
// 4 channels sums the slabs in ascending split order, then v = sum*scale + bias (+ per-sample bias); PReLU; + residual; ONE rounding;
// out2 = fma(rounded, out2_scale, out2_shift) rounded once.  n % 4 == 0 and out_ld % 4 == 0 (checked on the host); the slab and vector
// loads are issued together as in idb_splitk_reduce_kernel.
template <typename T>
__global__ __launch_bounds__(256) void idb_splitk_reduce_ex_kernel(const float* __restrict__ partial, int splitk, int M, int N, int HW,
                                                                   float scale, const float* bias, const float* sbias, int sbias_ld,
                                                                   const T* res, T* out, int out_ld, const float* slope, T* out2,
                                                                   const float* out2_scale, const float* out2_shift) {
    using V4 = typename Op<T>::v4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * (N / 4)) return;
    const int m = (int)(idx / (N / 4)), n = (int)(idx - (long long)m * (N / 4)) * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 bi = zero, sbv = zero, sl = zero;
    V4 r4;
    if (res) r4 = *(const V4*)(res + (long long)m * out_ld + n);
    if (bias) bi = *(const f32x4*)(bias + n);
    if (sbias) sbv = *(const f32x4*)(sbias + (long long)(m / HW) * sbias_ld + n);
    if (slope) sl = *(const f32x4*)(slope + n);
    const float* src = partial + (long long)m * N + n;
    const long long slab = (long long)M * N;
    f32x4 v = zero;
    for (int z0 = 0; z0 < splitk; z0 += 8) {
        f32x4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = *(const f32x4*)(src + (long long)min(z0 + u, splitk - 1) * slab);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = z0 + u < splitk;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += in ? t[u][e] : 0.f;
        }
    }
    V4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = v[e] * scale + bi[e] + sbv[e];
        if (slope && x < 0.f) x *= sl[e];
        if (res) x += to_f32<T>(r4[e]);
        o[e] = from_f32<T>(x);
    }
    *(V4*)(out + (long long)m * out_ld + n) = o;
    if (out2) {
        const f32x4 a = *(const f32x4*)(out2_scale + n), b = *(const f32x4*)(out2_shift + n);
        V4 o2;
#pragma unroll
        for (int e = 0; e < 4; ++e) o2[e] = affine_round<T>(to_f32<T>(o[e]), a[e], b[e]);
        *(V4*)(out2 + (long long)m * out_ld + n) = o2;
    }
}

template <typename T>
int launch_all(const idb_gemm_desc* d, const GemmParams& p, const Plan& pl, hipStream_t st) {
    constexpr int dt = std::is_same<T, __bf16>::value ? 0 : 1;
    const LaunchFn launch = p.gn_in_part ? pl.v->launch_gn[dt] : d->act == 3 ? pl.v->launch_relu[dt] : pl.v->launch[dt];
    if (!launch) {
        idb_set_error("idb_gemm: fused GroupNorm is built for 64-row tiles only");
        return IDB_EUNSUPPORTED;
    }
    const int rc = launch(*pl.v, p, pl, st);
    if (rc != IDB_OK || (d->flags & 1)) return rc;
    if (d->act == 2 || d->out2) {
        const long long total = (long long)pl.M * (d->n / 4);
        hipLaunchKernelGGL((idb_splitk_reduce_ex_kernel<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, p.partial, pl.splitk, pl.M,
                           d->n, p.HW, p.scale, p.bias, p.sbias, p.sbias_ld, (const T*)p.res, (T*)p.out, p.out_ld,
                           d->act == 2 ? d->act_slope : nullptr, (T*)d->out2, d->out2_scale, d->out2_shift);
        IDB_CHECK_LAUNCH("idb_splitk_reduce_ex");
        return IDB_OK;
    }
    return idb_finish_splitk<T>(p, pl.M, d->n, d->batch, pl.splitk, d->gn_partials, d->gn_groups, d->dtype, st, d->act == 3);
}

}  // namespace

extern "C" size_t idb_gemm_workspace_bytes(const idb_gemm_desc* d) {
    Plan pl;
    if (plan_gemm(d, &pl) != IDB_OK) return 0;
    return pl.splitk > 1 ? (size_t)pl.splitk * pl.M * d->n * sizeof(float) : 0;
}

// a folded LayerNorm needs the LDS-staged epilogue, or the persistent variant with >= 2 K-steps (statistics loaded at the first,
// reduced at the second)
static bool gemm_folds_ln(const idb_gemm_desc* d, const Plan& pl) {
    if (d->nsrc != 1 || d->src[0].taps != 1 || d->n % 4 || d->bias || d->sample_bias) return false;
    // persistent variant: built and tested, but off unless asked for (flags bit 8 / IDB_GEMM_PL_LN=1) — measured on one box, the
    // producer's statistics pass + the fold cost what the idb_layernorm launch costs: batch 64 14.77 -> 14.65 images/s (twice),
    // batch 1 6.645 vs 6.641 with 15 fewer launches
    if (pl.v->fam == kPersistent) return (plan_env().pl_ln || (d->flags & 256)) && pl.ktiles >= 2;
    return gemm_uses_lds_epilogue(d, pl);
}

// the GEMM's own LDS-staged epilogue can emit the first GroupNorm pass of the output (no split-K, whole groups per column tile)
static bool gemm_epilogue_emits_gn(const idb_gemm_desc* d, const Plan& pl, int groups) {
    if (d->geglu || !gemm_uses_lds_epilogue(d, pl)) return false;
    const int epi_threads = d->gn_in_partials ? 256 : pl.v->epi_threads;      // the fused-GroupNorm kernel has 4 MFMA waves
    return idb_epilogue_emits_gn(pl.v->bm, pl.v->bn, epi_threads, pl.M, d->n, groups) && (long long)d->out_h * d->out_w % 64 == 0 &&
           d->out_ld == d->n;
}

extern "C" int32_t idb_gemm_emits_gn_partials(const idb_gemm_desc* d, int32_t groups) {
    Plan pl;
    if (plan_gemm(d, &pl) != IDB_OK) return 0;
    if (pl.splitk > 1) return d->out_dtype == d->dtype && pl.M % 64 == 0 && gn_reduce_slice(d->n, groups) != 0 ? 1 : 0;
    return gemm_epilogue_emits_gn(d, pl, groups) ? 2 : 0;
}

// the fused GroupNorm runs on the patch-resident small tiles, or on the one-workgroup-per-CU loader-wave plans with a normalizer-wave
// twin (64-row tiles of families 5-7): stride 1, every normalised source on the output grid, tiles inside one sample or covering whole
// samples, no folded LayerNorm on the same launch
static bool gemm_fuses_gn(const idb_gemm_desc* d, const Plan& pl) {
    const Variant& v = *pl.v;
    if (!d->gn_in_partials) return false;
    if (v.fam == kPatchSmall) return conv_patch_ok(d, pl.M, v.bm);
    // the tap-major normalizer-wave kernel loses on every 3x3 conv (it re-normalises each pixel per tap): auto plans use it for 1x1 sources
    // only (Transformer2DModel norm + proj_in); forced tile ids and IDB_GN_TAPMAJOR=1 still reach it for 3x3 sources
    if (d->src[0].taps == 9 && d->tile == 0 && !plan_env().gn_tapmajor) return false;
    if (!v.launch_gn[0] || d->stride != 1 || d->ln_stats || d->geglu || d->gn_in_nsrc < 1 || d->gn_in_nsrc > d->nsrc) return false;
    const long long hw = (long long)d->out_h * d->out_w;
    if (!(hw % v.bm == 0 || (v.bm % hw == 0 && v.bm / hw <= 2))) return false;
    long long cn = 0;
    for (int s = 0; s < d->gn_in_nsrc; ++s) {
        if (d->src[s].upsample || d->src[s].in_h != d->out_h || d->src[s].in_w != d->out_w) return false;
        cn += d->src[s].channels;
    }
    if (d->gn_in_groups <= 0 || cn % d->gn_in_groups || cn / d->gn_in_groups < 1 || d->gn_in_chunks < 1 || d->gn_in_chunks > 64) return false;
    return gn_fused_lds(v, hw, cn, d->gn_in_groups) <= 160 * 1024;
}

extern "C" int32_t idb_gemm_fuses_groupnorm(const idb_gemm_desc* d) {
    Plan pl;
    return plan_gemm(d, &pl) == IDB_OK && gemm_fuses_gn(d, pl) ? 1 : 0;
}

// grouped weights (w_groups > 1) select the matrix per row tile: a tile must lie inside one group, and the persistent variant walks
// tiles across groups.  When this holds idb_gemm refuses the grouped descriptor and the caller runs one launch per group on row
// slices, which carry neither row statistics out nor a folded LayerNorm in
static bool grouped_runs_per_group(const idb_gemm_desc* d, const Plan& pl) {
    return d->w_groups > 1 && (pl.v->fam == kPersistent || d->w_group_rows % pl.v->bm != 0);
}

extern "C" int32_t idb_gemm_folds_layernorm(const idb_gemm_desc* d) {
    Plan pl;
    return plan_gemm(d, &pl) == IDB_OK && !grouped_runs_per_group(d, pl) && gemm_folds_ln(d, pl) ? 1 : 0;
}

extern "C" int32_t idb_gemm_row_stats_tiles(const idb_gemm_desc* d) {
    Plan pl;
    if (plan_gemm(d, &pl) != IDB_OK || grouped_runs_per_group(d, pl) || !gemm_uses_lds_epilogue(d, pl)) return 0;
    return pl.tiles_n;
}

extern "C" int idb_gemm_plan(const idb_gemm_desc* d, int32_t* tile, int32_t* split_k, int32_t* blocks) {
    Plan pl;
    int rc = plan_gemm(d, &pl);
    if (rc != IDB_OK) return rc;
    if (tile) *tile = pl.v->id;
    if (split_k) *split_k = pl.splitk;
    if (blocks) *blocks = pl.tiles_m * pl.tiles_n * pl.splitk;
    return IDB_OK;
}
extern "C" int idb_gemm(const idb_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    Plan pl;
    int rc = plan_gemm(d, &pl);
    if (rc != IDB_OK) return rc;
    const size_t need = pl.splitk > 1 ? (size_t)pl.splitk * pl.M * d->n * sizeof(float) : 0;
    IDB_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && idb_aligned16(workspace)),
                "idb_gemm: workspace too small (%zu < %zu) or unaligned", workspace_bytes, need);
    GemmParams p = {};
    for (int s = 0; s < IDB_MAX_SRC; ++s) {
        const idb_gemm_src& S = d->src[s < d->nsrc ? s : d->nsrc - 1];
        p.src[s] = GemmSrcK{(const char*)S.ptr, (unsigned)((long long)d->batch * S.in_h * S.in_w * S.channels * 2), S.channels,
                            S.taps, S.in_h, S.in_w, S.upsample};
    }
    p.M = pl.M;
    p.N = d->n;
    p.HW = d->out_h * d->out_w;
    p.OW = d->out_w;
    p.stride = d->stride;
    p.pad = d->pad_mode == 1 ? 0 : 1;
    if (d->w_layout == 1) {          // K-tiled 16-row blocks (idb_tile_weight): [ceil(n/16)][K/64][16 rows][64 k]
        p.w_row_bytes = 128u;
        p.w_kstep = 2048u;
        p.w_blk_bytes = (unsigned)pl.ktiles * 2048u;
        p.w_bytes = (unsigned)(((long long)d->n + 15) / 16 * pl.ktiles * 2048);
    } else {
        p.w_row_bytes = (unsigned)(pl.K * 2);
        p.w_kstep = 128u;
        p.w_blk_bytes = (unsigned)(pl.K * 32);
        p.w_bytes = (unsigned)((long long)d->n * pl.K * 2);
    }
    p.ktiles = pl.ktiles;
    p.kt_per_split = pl.kt_per_split;
    p.xcd_mode = 0;
    if (plan_env().xcd_slices && pl.v->xcd_slices) {
        if (pl.splitk >= 8 && pl.splitk % 8 == 0) p.xcd_mode = 1;
        else if (pl.splitk == 4 && ((long long)pl.tiles_m * pl.tiles_n) % 2 == 0) p.xcd_mode = 2;
    }
    p.splitk = pl.splitk;
    p.w = (const char*)d->w;
    p.bias = d->bias;
    p.sbias = d->sample_bias;
    p.sbias_ld = d->sample_bias_ld;
    p.res = (const char*)d->residual;
    p.out = d->out;
    p.out_ld = d->out_ld;
    p.out_f32 = d->out_dtype == IDB_F32;
    p.geglu = d->geglu;
    p.scale = d->out_scale == 0.f ? 1.f : d->out_scale;
    p.partial = (float*)workspace;
    p.tiles_n = pl.tiles_n;
#ifndef IDB_PROFILING
    IDB_REQUIRE(!(d->flags & (2 | 32 | 64 | 128)), "idb_gemm: flags bits 1/5/6/7 are profiling switches of libidb_kernels_prof.so (make prof)");
#endif
    p.dbg_skip_store = (d->flags & 2) ? 1 : ((d->flags & 32) ? 2 : 0);
    p.out_bytes = (unsigned)((long long)pl.M * d->out_ld * 2);
    p.act = d->act;
    p.dbg_loop = (d->flags & 64) ? 1 : ((d->flags & 128) ? 2 : 0);
    {
        // In-kernel split-K reduce (flags bit 4 only).  Measured on MI355X it LOSES to the separate reduce launch in the
        // sampling loop (batch 1: 4.49 vs 5.11 images/s): every split workgroup pays an agent-scope release (buffer_wbl2
        // of its XCD's L2) and one workgroup per tile re-reads all slabs — the "splitk-seam" price of the CDNA guide.
        // The path is kept, tested bit-identical to the two-launch form, for shapes where a launch boundary is dearer.
        const int env_fused = plan_env().fused_reduce;
        const bool want_fused = (d->flags & 16) || (env_fused > 0 && pl.splitk <= env_fused);
        const bool fused_reduce = pl.splitk > 1 && d->counters && want_fused && !(d->flags & 8) && !(d->flags & 1) && d->act != 2 && !d->out2 &&
                                  (long long)pl.tiles_m * pl.tiles_n <= d->counters_len;
        p.counters = fused_reduce ? d->counters : nullptr;
        p.lds_epi = lds_epilogue_runs(d, *pl.v, pl.splitk == 1 || fused_reduce) ? 1 : 0;
    }
    if (d->row_stats_out || d->ln_stats) {
        if ((d->row_stats_out && (!p.lds_epi || pl.v->fam == kRegStaged)) || (d->ln_stats && !gemm_folds_ln(d, pl))) {
            idb_set_error("idb_gemm: row_stats_out needs a plan with the LDS-staged epilogue (no split-K, no persistent / register-staged variant); "
                          "ln_stats that or the persistent variant");
            return IDB_EUNSUPPORTED;
        }
        IDB_REQUIRE(!d->ln_stats || (d->ln_tiles > 0 && d->ln_u && d->ln_v && idb_aligned16(d->ln_u) && idb_aligned16(d->ln_v) && ((uintptr_t)d->ln_stats & 7) == 0 &&
                                     d->nsrc == 1 && d->src[0].taps == 1 && d->n % 4 == 0 && !d->bias && !d->sample_bias),
                    "idb_gemm: ln_stats needs ln_tiles > 0, aligned ln_u / ln_v, one 1x1 source, n %% 4 == 0, and no bias / sample_bias "
                    "(add the layer's bias into ln_v)");
        IDB_REQUIRE(!d->row_stats_out || (((uintptr_t)d->row_stats_out & 7) == 0 && !d->geglu), "idb_gemm: row_stats_out must be 8-byte aligned, no GEGLU");
    }
    if (d->gn_partials && pl.splitk == 1 && !(d->flags & 1) && gemm_epilogue_emits_gn(d, pl, d->gn_groups)) {
        p.gn_part = d->gn_partials;          // launch_all's idb_finish_splitk then has nothing left to launch
        p.gn_groups = d->gn_groups;
    }
    if (d->gn_in_partials) {
        if (!gemm_fuses_gn(d, pl)) {
            idb_set_error("idb_gemm: this plan cannot fuse the GroupNorm (needs a one-workgroup-per-CU loader-wave plan, stride 1, sources on the "
                          "output grid, tile inside one sample): run idb_groupnorm + idb_gemm");
            return IDB_EUNSUPPORTED;
        }
        IDB_REQUIRE(d->gn_in_gamma && d->gn_in_beta && d->gn_in_eps > 0.f && idb_aligned16(d->gn_in_partials), "idb_gemm: gn_in_gamma / gn_in_beta / gn_in_eps invalid");
        p.gn_in_part = d->gn_in_partials;
        p.gn_in_gamma = d->gn_in_gamma;
        p.gn_in_beta = d->gn_in_beta;
        p.gn_in_chunks = d->gn_in_chunks;
        p.gn_in_groups = d->gn_in_groups;
        p.gn_in_nsrc = d->gn_in_nsrc;
        p.gn_in_silu = d->gn_in_silu;
        p.gn_in_eps = d->gn_in_eps;
        p.gn_in_c = 0;
        for (int s = 0; s < d->gn_in_nsrc; ++s) p.gn_in_c += d->src[s].channels;
    }
    p.w_groups = d->w_groups > 1 ? d->w_groups : 1;
    p.w_group_rows = d->w_group_rows;
    p.w_group_stride = d->w_group_stride;
    if (p.w_groups > 1) {
        IDB_REQUIRE(d->w_group_rows > 0 && d->w_group_stride >= (long long)p.w_bytes && d->w_group_stride % 16 == 0 &&
                        (long long)d->w_groups * d->w_group_stride < (1LL << 40), "idb_gemm: w_groups needs w_group_rows > 0 and a 16-byte-multiple w_group_stride >= one matrix");
        if (grouped_runs_per_group(d, pl)) {
            idb_set_error("idb_gemm: w_group_rows = %d is not a multiple of the plan's tile height %d (or the persistent variant was chosen): run one launch per group",
                          d->w_group_rows, pl.v->bm);
            return IDB_EUNSUPPORTED;
        }
    }
    p.rowstat_out = d->row_stats_out;
    p.ln_stats = d->ln_stats;
    p.ln_u = d->ln_u;
    p.ln_v = d->ln_v;
    p.ln_nt = d->ln_tiles;
    p.ln_c = (int)pl.K;
    p.ln_eps = d->ln_eps;
    p.slab_swc = 0;
    if (d->gn_partials && pl.splitk > 1 && !p.counters && !(d->flags & 1) && !p.out_f32 && pl.M % 64 == 0) {
        // the reduce launch will be idb_splitk_reduce_gn_kernel: same conditions and slice width as launch_all computes
        if (idb_reduce_vec_ok(p, d->n)) p.slab_swc = gn_reduce_slice(d->n, d->gn_groups);
    }
    // everything the kernels would otherwise divide for (idb_gemm_epi.h: GemmParams)
    IDB_REQUIRE(idb_fill_geometry(p, (long long)pl.tiles_m * pl.tiles_n, pl.v->bm), "idb_gemm: grid or K range beyond 2^31 (tiles, split_k * K-steps)");
    hipStream_t st = (hipStream_t)stream;
    return d->dtype == IDB_BF16 ? launch_all<__bf16>(d, p, pl, st) : launch_all<_Float16>(d, p, pl, st);
}

