// Body of idb_gemm_kernel and of its ReLU twin idb_gemm_kernel_relu (idb_gemm.hip), included inside each kernel with the
// compile-time RELU of its epilogue (idb_gemm_desc.act = 3) in scope.  Textual inclusion rather than a shared device function: that
// form moved the 3-stage kernels' SGPR counts, this one leaves the existing kernels' code as it was.
#if defined(__HIP_DEVICE_COMPILE__)   // the host pass only needs the launch stub (buffer-resource types are device-only)
    using V8 = typename Op<T>::v8;
    constexpr int BM = 16 * MF * WM, BN = 32 * NF;
    constexpr int THREADS = 128 * WM, RS = 16 * WM;          // staging: RS tile rows per wave-instruction sweep of the workgroup
    constexpr int NJ = (BN + RS - 1) / RS;                   // weight-row sweeps; the last may be partial (160 rows / 64): its surplus
    constexpr int STAGE = (BM + NJ * RS) * 128;              // rows are LDS padding filled with zeros (out-of-range voffset), so every
                                                             // wave issues the same number of loads and the counted vmcnt stays exact
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4;

    // XCD-aware bijective remaps (workgroups are dealt round-robin over the 8 XCDs in linear-id order, so ids b and b+8 share
    // an XCD and its L2; the 8 L2s are not coherent and do not share lines).
    //  mode 0: each XCD gets a contiguous run of tiles, so neighbours re-use the same activation rows from that L2; the K
    //          split, if any, is the grid's z.
    //  mode 1 (split-K, S % 8 == 0) / mode 2 (S == 4): each XCD owns ONE K-slice (mode 2: half the tiles of one) of EVERY
    //          tile, so every weight and activation byte crosses the fabric once instead of once per XCD — on the batch-1
    //          weight-streaming layers (M = 512: 4 row tiles on 4 XCD pairs) mode 0 fetched the weights 4-8 times
    //          (rocprofv3 FETCH_SIZE: 99-113 MB per launch against 28-40 MB of operands).
    // `h` (GemmTile) holds the launch scalars as plain kernel parameters: tile index, K range and the source of the first K-step need no
    // kernel-argument load.  The head and that source's record are then requested together and waited for once (idb_loader_head).
    int wg, kz, tm, tn;
    idb_wg_tile(h, wg, kz);
    idb_tile_mn(h, wg, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    int kt0, kt1;                                            // balanced partition: slice sizes differ by at most one
    idb_k_range(h, kz, kt0, kt1);
    const int nk = kt1 - kt0;

    // ---- K-step state: source s, tap (0..8; a 1x1 source sits on the centre tap 4), channel offset c0.
    // Per-row voffsets (pixel address, zero padding -> out-of-range) are recomputed only when the tap or the
    // source changes (every C/64 K-steps); inside a tap the channel offset rides in the SGPR soffset, so a
    // K-step costs no address VALU at all.
    int s, rem, tap, c0, cur_c = 64, tap_end = 9;
    idb_k_seek_src(h, kt0, s, rem);
    GemmHead q;
    GemmSrcK S;
    idb_loader_head(p, s, q, S);
    idb_k_seek_tap(S, rem, tap, c0);

    // ---- per-thread staging coordinates: thread loads chunk position (tid&7) of rows (tid>>3)+32i;
    // the 16-byte chunk it fetches is (tid&7) ^ (row&7): the swizzle lives on the source address.
    const int lrow = tid >> 3;
    const unsigned cg16 = ((tid & 7) ^ (lrow & 7)) * 16;
    int a_b[MF], a_oy[MF], a_ox[MF];
    bool a_ok[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + i * RS + lrow;
        a_ok[i] = m < q.M;
        idb_row_decode(q, a_ok[i] ? m : 0, a_b[i], a_oy[i], a_ox[i]);
    }
    __amdgpu_buffer_rsrc_t rs_a, rs_w;
    unsigned a_voff[MF], w_voff[NJ];
    unsigned w_soff = (unsigned)kt0 * q.w_kstep;
    bool need_retap = true;
    auto retap = [&]() {
        rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)S.ptr, 0, S.bytes, IDB_RSRC_FLAGS);
        cur_c = S.C;
        tap_end = S.taps == 9 ? 9 : 5;
        const int t3 = tap / 3;
        const int dy = t3 - q.pad, dx = tap - t3 * 3 - q.pad;
        const int LH = S.H << S.up, LW = S.W << S.up;
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int iy = a_oy[i] * q.stride + dy, ix = a_ox[i] * q.stride + dx;
            const bool ok = a_ok[i] && (unsigned)iy < (unsigned)LH && (unsigned)ix < (unsigned)LW;
            const int pix = (a_b[i] * S.H + (iy >> S.up)) * S.W + (ix >> S.up);
            a_voff[i] = ok ? (unsigned)pix * (unsigned)(S.C * 2) + cg16 : IDB_OOB;
        }
    };
    auto stage_a = [&](int buf) {                            // the A half of a stage
        char* sA = smem + buf * STAGE;
        if (need_retap) {
            retap();
            need_retap = false;
        }
        const unsigned a_soff = (unsigned)c0 * 2u;
#pragma unroll
        for (int i = 0; i < MF; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_a, LDS_PTR(sA + (i * THREADS + wave * 64) * 16), 16, a_voff[i], a_soff, 0, 0);
    };
    auto stage_w = [&](int buf) {                            // the W half, and on to the next K-step
        char* sB = smem + buf * STAGE + BM * 128;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, LDS_PTR(sB + (j * THREADS + wave * 64) * 16), 16, w_voff[j], w_soff, 0, 0);
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
    auto stage = [&](int buf) {
        stage_a(buf);
        stage_w(buf);
    };
    // First DMA first, as in idb_gemm_kernel_lw: the A half of stage 0 is requested as soon as the K seek and the row decode allow;
    // the weight descriptor, the weight offsets and the grouped-weight arithmetic — which only the W half needs — come behind it.
    // The loads of a stage keep their order and count.
    if (0 < nk) stage_a(0);
    // weights: one descriptor, per-row voffset fixed for the whole K loop, K position in the SGPR soffset
    rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)(q.w + idb_weight_group(q, m0) * q.w_group_stride), 0, q.w_bytes, IDB_RSRC_FLAGS);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + j * RS + lrow;
        w_voff[j] = (n < q.N && j * RS + lrow < BN) ? (unsigned)(n >> 4) * q.w_blk_bytes + (unsigned)(n & 15) * q.w_row_bytes + cg16 : IDB_OOB;
    }
    if (0 < nk) stage_w(0);

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- NS-deep LDS ring, one barrier per K-step.  At the top of iteration `it` tiles it .. it+NS-2 are in
    // flight; the counted vmcnt retires tile `it` (this wave's share), the barrier makes every wave's share
    // visible AND proves that all waves are done reading tile it-1, whose buffer the next DMA overwrites.
    constexpr int LOADS = MF + NJ;
#pragma unroll
    for (int st = 1; st < NS - 1; ++st)
        if (st < nk) stage(st);
    // folded LayerNorm: this thread's share of its tile row's statistics, the loads in flight with the first operand tiles
    float2 ln_part = make_float2(0.f, 0.f);
    if (p.ln_stats) ln_part = idb_ln_row_partials<BM, THREADS>(p, m0, tid);
    int cur = 0;
    for (int it = 0; it < nk; ++it) {
        if (NS > 2 && it + NS - 2 < nk)
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * LOADS) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (it + NS - 1 < nk && IDB_DBG(p.dbg_loop) != 2) stage(cur == 0 ? NS - 1 : cur - 1);
        if (IDB_DBG(p.dbg_loop) == 1) {
            cur = cur + 1 == NS ? 0 : cur + 1;
            continue;
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
        cur = cur + 1 == NS ? 0 : cur + 1;
    }

    idb_gemm_epilogue<T, MF, NF, WM, RELU>(p, smem, acc, m0, n0, tid, wm, wn, fr, fg, kz, p.ln_stats != nullptr, ln_part);
#endif
