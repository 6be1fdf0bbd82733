/*
 * idb_kernels.h — C ABI of libidb_kernels.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * ID-Booth sampling path (SD-2.1 UNet forward, CFG + DDPM step, VAE decode).
 *
 * The reference has no FFI for this path: it is a Python object protocol
 * (diffusers.StableDiffusionPipeline, /root/reference/inference_ID-Booth.py:103-108,138), and every
 * arithmetic step is dispatched by torch/cuDNN/cuBLAS inside un-vendored diffusers.  Each entry point
 * below therefore cites the upstream op it replaces and the reference call
 * site that reaches it.  INTEGRATION.md shows the ctypes binding a maintainer of the reference adds.
 *
 * Conventions:
 *   - plain C types only; device pointers are void*; `stream` is a hipStream_t passed as void*;
 *   - every function returns 0 (IDB_OK) or a negative idb_status; idb_last_error() gives the text
 *     (thread-local);
 *   - no ownership transfer: the caller allocates inputs, outputs and workspaces;
 *   - kernels are asynchronous on `stream` and never synchronise (graph-capturable);
 *   - activations are NHWC ("channels-last") in the operand dtype (bf16 or f16), so a [B,H,W,C]
 *     feature map and a [B, H*W, C] token matrix are the same bytes;
 *   - weights are [N][K] row-major in the operand dtype (torch Linear convention); conv weights are
 *     repacked to [Cout][tap][Cin] by idb_pack_conv_weight.
 */
#ifndef IDB_KERNELS_H
#define IDB_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { IDB_OK = 0, IDB_EINVAL = -1, IDB_EUNSUPPORTED = -2, IDB_EHIP = -3 } idb_status;
typedef enum { IDB_BF16 = 0, IDB_F16 = 1, IDB_F32 = 2 } idb_dtype;

#define IDB_MAX_SRC 4

int idb_version(void);
/* Number of kernels this library has launched in this process so far (every entry point counts each of its launches, e.g. a
 * split-K idb_gemm counts the GEMM and its reduce launch).  For launch-count accounting (bench.py, tests); monotonic. */
uint64_t idb_launch_count(void);
const char* idb_last_error(void);
/* 0 iff `device` is a gfx950 part (the only target this library is built for). */
int idb_device_check(int device);

/* ------------------------------------------------------------------------------------------
 * K1/K2/K3 — implicit GEMM:  out[m][n] = sum_k A[m][k] * W[n][k]  (+ fused epilogue)
 *
 * Replaces: nn.Conv2d 3x3 (stride 1/2, pad 1), nearest-2x upsample + conv, 1x1 conv_shortcut,
 * nn.Linear, GEGLU — i.e. diffusers ResnetBlock2D / Downsample2D / Upsample2D / Attention.to_* /
 * FeedForward as dispatched from UNet2DConditionModel.forward (inference_ID-Booth.py:138,
 * train_ID-Booth.py:1040-1046) and Decoder.forward (train_ID-Booth.py:410-412).
 *
 * A is never materialised: row m = output pixel (b, oy, ox); the K axis is the concatenation of up
 * to IDB_MAX_SRC sources, each contributing taps*channels columns ordered [tap][channel]:
 *   taps = 9 : 3x3 window with zero padding 1 read from an NHWC tensor [batch][in_h][in_w][channels]
 *              (upsample = 1: the tensor is logically nearest-2x upsampled first);
 *   taps = 1 : the pixel itself (1x1 conv, or a plain [M][K] matrix with in_h = in_w = 1); in a stride-2 GEMM (pad_mode 0) a 1x1
 *              source may instead sit on the input grid (out = ceil(in / 2)) and read pixel (2 oy, 2 ox): the strided shortcut.
 * Several sources give skip-concatenation and the fused 1x1 shortcut without a concat pass.
 * channels must be a multiple of 64 for every source.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* ptr;
    int32_t channels;
    int32_t taps;      /* 9 or 1 */
    int32_t in_h, in_w;
    int32_t upsample;  /* 0 or 1 */
} idb_gemm_src;

typedef struct {
    int32_t dtype;            /* IDB_BF16 or IDB_F16: operand dtype of A, W, residual */
    int32_t batch, out_h, out_w;   /* M = batch*out_h*out_w */
    int32_t stride;           /* 1 or 2, applies to taps=9 sources */
    int32_t n;                /* rows of W (before GEGLU halving) */
    int32_t nsrc;
    idb_gemm_src src[IDB_MAX_SRC];
    const void* w;            /* [n][K] */
    const float* bias;        /* [n] or NULL */
    const float* sample_bias; /* [batch][sample_bias_ld] added per sample (temb projection) or NULL */
    int32_t sample_bias_ld;   /* 0 = the same row for every sample */
    const void* residual;     /* [M][out_ld] operand dtype, or NULL */
    int32_t geglu;            /* 1: W rows interleaved by idb_pack_matrix(geglu=1); out has n/2 cols */
    void* out;
    int32_t out_dtype;        /* IDB_BF16/IDB_F16 (== dtype) or IDB_F32 */
    int32_t out_ld;           /* elements between output rows */
    int32_t split_k;          /* 0 = library heuristic, >=1 explicit */
    int32_t tile;             /* 0 = heuristic; else a tile config id as idb_gemm_plan reports it (tests and measurements) */
    float out_scale;          /* multiplies the accumulator before bias (0 => 1.0) */
    int32_t flags;            /* profiling/testing only — bit 0: skip the split-K reduce launch (`out` not written); bit 1: skip the epilogue stores; bit 2: force the direct (non-LDS-staged) epilogue; bit 3: force the two-launch split-K reduce; bit 4: in-kernel split-K reduce (default: separate reduce launch, which measured faster); bit 8: let the persistent variant fold a LayerNorm (ln_stats; default: IDB_EUNSUPPORTED there, the separate idb_layernorm measured no slower) */
    int32_t act;              /* 0 none, 1 exact GELU applied to (acc*scale + bias) (CLIP MLP fc1); not with residual/GEGLU;
                               * 3 ReLU, the same place (RepVGG blocks): not with residual / GEGLU / gn_partials / gn_in_partials, on the
                               * LDS-ring and loader-wave tiles; split-K plans apply it in their reduce; 2: see act_slope */
    uint32_t* counters;       /* optional: >= counters_len zeroed uint32 on the device, private to the stream; used only with
                                 flags bit 4: a split-K launch then reduces inside the GEMM (the last-arriving workgroup of a
                                 tile sums the slabs in fixed order and runs the epilogue; counters are left zero) */
    int32_t counters_len;
    float* gn_partials;       /* optional out: per-(sample, 64-row block, group) {sum, sum of squares} of the ROUNDED output, fp32
                                 [batch][out_h*out_w/64][gn_groups][2] — the first pass of the nn.GroupNorm that consumes `out`
                                 (idb_groupnorm's partials_in), produced by the split-K reduce launch when there is one, by the GEMM's own
                                 LDS-staged epilogue when its column tiles hold whole groups (idb_gemm_emits_gn_partials), by an extra
                                 statistics launch otherwise.  Needs out_h*out_w % 64 == 0, out_h*out_w <= 4096, n % gn_groups == 0,
                                 operand-dtype output, no GEGLU */
    int32_t gn_groups;
    /* LayerNorm folded into the GEMM (BasicTransformerBlock norm1/2/3 -> to_q/k/v, attn2.to_q, ff.net.0): `src` holds the RAW rows
     * x [M][K = ln_c]; `w` = W scaled by the LayerNorm gamma along K; out = rstd_m (x W'^T - mean_m u) + v, with
     * u[n] = sum_k W'[n][k] (of the ROUNDED operand values) and v[n] = sum_k beta[k] W[n][k] + the layer's bias[n] (fp32 [n],
     * 16-byte aligned; `bias` and `sample_bias` must be NULL: the epilogue keeps two column vectors per fragment in flight), and the
     * per-row statistics taken from ln_stats = the row_stats_out of the GEMM that produced x: fp32 [M][ln_tiles][2] partial
     * {sum, sum of squares} per column tile.  Exact in fp32 (x W'^T - mean u = (x - mean) W'^T term by term).  row_stats_out needs
     * a plan that runs the LDS-staged epilogue (no split-K, no persistent variant, operand-dtype output), ln_stats that or the
     * persistent variant: idb_gemm returns IDB_EUNSUPPORTED otherwise and the caller keeps idb_layernorm; idb_gemm_row_stats_tiles
     * (producer side, 0 = unsupported) and idb_gemm_folds_layernorm (consumer side) tell beforehand. */
    float* row_stats_out;     /* optional out: [M][idb_gemm_row_stats_tiles(d)][2] */
    const float* ln_stats;    /* optional in */
    int32_t ln_tiles;
    const float* ln_u;
    const float* ln_v;
    float ln_eps;
    int32_t pad_mode;         /* taps=9 sources — 0: zero padding 1 on every side (nn.Conv2d padding=1); 1: padding on the
                                 bottom/right only, i.e. F.pad(x, (0,1,0,1)) + padding=0, the stride-2 Downsample2D of the VAE
                                 encoder (diffusers downsampling.py; AutoencoderKL.encode at train_ID-Booth.py:1001) */
    int32_t w_layout;         /* 0: `w` is [n][K] rows (K contiguous); 1: K-tiled 16-row blocks written by idb_tile_weight,
                                 [ceil(n/16)][K/64][16 rows][64 k]: the rows of one K-step of a column tile are whole 2 KiB runs and
                                 a workgroup's K loop reads each of its row blocks as ONE contiguous stream (HBM pages, TLB reach)
                                 instead of 128-byte pieces at a K*2-byte stride */
    /* Grouped weights — a mixed-identity batch in ONE launch (BASELINE configs[2] = 8 identities x 8 prompts; per-row LoRA adapters of
     * peft's lora.Linear, train_ID-Booth.py:672-678, in their MERGED form): `w` holds w_groups weight matrices of identical shape,
     * w_group_stride bytes apart (each [n][K] rows or K-tiled as w_layout says); output row m uses matrix (m / w_group_rows) % w_groups.
     * w_group_rows must be a multiple of the plan's tile height (idb_gemm returns IDB_EUNSUPPORTED otherwise: the caller then runs one
     * launch per group).  With a folded LayerNorm, ln_u / ln_v hold w_groups vectors of n floats each.  0 or 1: one matrix. */
    int32_t w_groups;
    int32_t w_group_rows;
    int64_t w_group_stride;
    /* GroupNorm(+SiLU) fused into the GEMM (north_star "conv3x3 + GroupNorm+SiLU fused"; diffusers ResnetBlock2D norm1+conv1,
     * norm2+conv2(+conv_shortcut), Transformer2DModel norm+proj_in): the first gn_in_nsrc sources hold the RAW tensors; their channel
     * concatenation is normalised with nn.GroupNorm(gn_in_groups, eps) from gn_in_partials (the statistics idb_groupnorm takes as
     * partials_in: [batch][gn_in_chunks][gn_in_groups][2], gn_in_chunks <= 64), gamma / beta over those channels, then SiLU if
     * gn_in_silu — inside the kernel, with idb_groupnorm's arithmetic (the MFMA waves read the operand bits idb_groupnorm would have
     * written); zero padding stays zero.  Two forms, both for plans that run one workgroup per CU (small grids: the batch-1 UNet):
     * 3x3 sources (every source normalised, 64- / 128-row tiles inside one sample) go through the patch-resident conv, whose patch
     * loaders normalise each halo patch once per 64-channel chunk (tile ids 10x); 1x1 sources (proj_in) through dedicated normalizer
     * waves on the landed LDS stage (tile ids 5x-7x).  idb_gemm_fuses_groupnorm tells beforehand, idb_gemm returns IDB_EUNSUPPORTED
     * otherwise and the caller runs idb_groupnorm + idb_gemm.  Needs stride 1 and sources on the output's spatial grid.  NULL: off. */
    const float* gn_in_partials;
    int32_t gn_in_chunks, gn_in_groups, gn_in_nsrc, gn_in_silu;
    float gn_in_eps;
    const float* gn_in_gamma;
    const float* gn_in_beta;
    /* PReLU epilogue (act = 2; ArcFace IResNet): v = acc*out_scale + bias (+ per-sample bias), then v >= 0 ? v : v*act_slope[n], before
     * the one rounding.  fp32 [n], 16-byte aligned; not with residual / GEGLU / a folded LayerNorm or GroupNorm.  Every plan applies it,
     * split-K ones in their reduce launch. */
    const float* act_slope;
    /* Second, affine output: out2[m][n] = fma(float(out[m][n]), out2_scale[n], out2_shift[n]) computed on the ROUNDED primary output and
     * rounded once to the operand dtype (the eval-mode BatchNorm that feeds the next zero-padded conv; ArcFace IBasicBlock.bn1), row stride
     * out_ld, 16-byte aligned.  All three or none; operand-dtype output, n % 4 == 0, no GEGLU / gn_partials / row_stats_out.  NULL: off. */
    void* out2;
    const float* out2_scale;
    const float* out2_shift;
} idb_gemm_desc;

size_t idb_gemm_workspace_bytes(const idb_gemm_desc* d);
/* What idb_gemm would launch for `d`: tile config id (shape + 10 * variant; shapes 1: 128x160, 2: 128x128, 3: 64x160,
 * 4: 64x64 (8 waves), 5: 128x32, 6-9: 64x160 / 64x128 / 128x160 / 128x128 with 8 waves; variant 0/1/2: 2-/3-/4-stage LDS ring,
 * 3: register-staged, 4: persistent, 5-7: loader waves, 8: loader waves with 256-row tiles (shapes 8/9), 9: patch-resident 3x3 conv
 * on 256-row tiles, 10: patch-resident 3x3 conv on the shape's own 64-/128-row tile), split-K factor and workgroup count.
 * Host-only, no GPU call. */
int idb_gemm_plan(const idb_gemm_desc* d, int32_t* tile, int32_t* split_k, int32_t* blocks);
/* Column tiles of the plan idb_gemm would run for `d` if that plan can emit row statistics (LDS-staged epilogue), else 0.  Also 0 for
 * a grouped descriptor (w_groups > 1) that idb_gemm refuses (w_group_rows no multiple of the plan's tile height, or the persistent
 * variant): the caller's one-launch-per-group run emits no row statistics. */
int32_t idb_gemm_row_stats_tiles(const idb_gemm_desc* d);
/* Would idb_gemm produce gn_partials for `groups` groups WITHOUT an extra statistics launch?  0: no (it would launch one — the caller's
 * two-pass idb_groupnorm is as good); 1: from its split-K reduce launch; 2: from its own LDS-staged epilogue (no split-K, 160-wide
 * tiles holding whole groups). */
int32_t idb_gemm_emits_gn_partials(const idb_gemm_desc* d, int32_t groups);
/* 1 if the plan idb_gemm would run for `d` (bias / sample_bias NULL, one 1x1 source) can apply a folded LayerNorm (ln_*); 0 as well
 * for a grouped descriptor (w_groups > 1) that idb_gemm refuses, as idb_gemm_row_stats_tiles. */
int32_t idb_gemm_folds_layernorm(const idb_gemm_desc* d);
/* 1 if idb_gemm would run `d` with its fused GroupNorm (gn_in_* set) in ONE launch. */
int32_t idb_gemm_fuses_groupnorm(const idb_gemm_desc* d);
int idb_gemm(const idb_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Weight packing (run once at load; SURVEY.md §8b "idb_pack_*"). src is fp32 in torch layout.
 * Limits of these entries and of the fp32 latent-path and boundary helpers below (idb_embed_tokens, idb_cfg_ddpm_step, idb_postprocess,
 * idb_nhwc_to_nchw_f32, idb_f32_nhwc_to_nchw, idb_cast_f32, idb_vae_sample): every size positive and fewer than 2^39 elements per call
 * (idb_tile_weight: of the padded destination), IDB_EINVAL before any HIP call; also idb_ln_fold_vectors rows < 2^33,
 * idb_embed_tokens batch * n_tokens < 2^31 and idb_vae_sample channels < 2^30.  dst needs the element's own alignment only, except
 * where 16 bytes are stated.
 * Rounding.  idb_pack_conv_weight and idb_pack_matrix round each fp32 value once to the operand dtype (to nearest even).  Where a value
 * is computed first (idb_pack_matrix_scaled, idb_lora_merge, idb_lora_merge_scaled), the last operation's result is rounded EITHER once
 * to the operand dtype OR to fp32 and then to the operand dtype, as the compiler chose for that dtype (f16 has a fused
 * multiply-add-and-convert, bf16 converts from an fp32 register): two values at most, which differ only where the fp32 rounding lands
 * on a tie of the operand dtype.  tests/test_prep_matrix_gpu.py records which one each dtype produced. */
/* [Cout][Cin][kh][kw] fp32 -> [Cout][kh*kw][Cin] operand dtype. */
int idb_pack_conv_weight(const float* src, void* dst, int32_t cout, int32_t cin, int32_t ktaps,
                         int32_t dtype, void* stream);
/* [rows][cols] fp32 -> operand dtype, optional GEGLU row interleave (value/gate in 16-row groups). */
int idb_pack_matrix(const float* src, void* dst, int64_t rows, int64_t cols, int32_t geglu,
                    int32_t dtype, void* stream);
/* [n][k] operand dtype (k % 64 == 0) -> the K-tiled layout idb_gemm_desc.w_layout = 1 reads: [ceil(n/16)][k/64][16][64], rows
 * past n zero-filled; dst holds idb_tiled_weight_bytes(n, k) bytes and must not overlap src. */
size_t idb_tiled_weight_bytes(int64_t n, int64_t k);
int idb_tile_weight(const void* src, void* dst, int64_t n, int64_t k, int32_t dtype, void* stream);
/* dst[rows][cols] = W + scale * B[rows][r] * A[r][cols], fp32 in, operand dtype out: merged LoRA
 * (peft lora.Linear with merged weights; inference_ID-Booth.py:107). */
int idb_lora_merge(const float* w, const float* lora_a, const float* lora_b, void* dst, int64_t rows,
                   int64_t cols, int32_t rank, float scale, int32_t dtype, void* stream);
/* The same with every column k multiplied by col_scale[k] before the rounding described above (the gamma of a folded LayerNorm);
 * lora_a == NULL (rank 0): dst = round(W * col_scale), the exact product rounded once or through fp32. */
int idb_lora_merge_scaled(const float* w, const float* lora_a, const float* lora_b, void* dst, int64_t rows, int64_t cols,
                          int32_t rank, float scale, const float* col_scale, int32_t dtype, void* stream);
/* idb_pack_matrix with every column k multiplied by col_scale[k]: the exact product rounded once to the operand dtype, or to fp32 and
 * then to it (see above) (GEGLU projection behind a folded LayerNorm). */
int idb_pack_matrix_scaled(const float* src, void* dst, int64_t rows, int64_t cols, int32_t geglu, const float* col_scale,
                           int32_t dtype, void* stream);
/* The two column vectors of a LayerNorm folded into a projection (idb_gemm_desc.ln_u / ln_v), for output rows r = 0..rows-1
 * (r -> source row sr through the GEGLU interleave when geglu = 1):
 *   u[r] = sum_k float(w_folded[r][k])              w_folded: the ROUNDED gamma-scaled operand-dtype matrix the GEMM multiplies
 *   v[r] = sum_k (W[sr][k] + scale * (B A)[sr][k]) * beta[k] + (bias ? bias[r] : 0)      fp32, W / A / B as idb_lora_merge
 * lora_a == NULL or rank == 0: no adapter.  rank <= 16. */
int idb_ln_fold_vectors(const float* w, const float* lora_a, const float* lora_b, int32_t rank, float scale, const void* w_folded,
                        const float* beta, const float* bias, float* u, float* v, int64_t rows, int64_t cols, int32_t geglu,
                        int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1 (norm part) / K6 — GroupNorm and LayerNorm.
 * Replaces nn.GroupNorm(32, C) (+ SiLU) of ResnetBlock2D / Transformer2DModel.norm / conv_norm_out
 * and nn.LayerNorm(C) x3 of BasicTransformerBlock.
 * GroupNorm input may be the channel-concatenation of two NHWC tensors (skip connections); the
 * output is one dense [B][HW][C0+C1] tensor.  Statistics are one-pass fp32 ({sum, sum of squares}; var = E[x^2] - mean^2 formed in
 * double), deterministic (fixed summation order; no float atomics).  Measured on MI355X against float64 (tests/test_norm_matrix_gpu.py),
 * outputs of magnitude >= 1: within one output ulp of nn.GroupNorm for |mean| / std up to 256 in bf16 (worst 0.76 ulp at 1 Mi elements
 * per group) and up to 16 in f16 (0.53 ulp at 1 Mi elements per group); f16 at |mean| / std = 64 is off by 0.8 / 0.9 / 1.3 ulp and at 256
 * by 4 / 9 / 19 ulp for 2560 / 40960 / 1 Mi elements per group.  The error of the mean is absolute, so relative to outputs near zero no
 * bound holds at any conditioning.
 * sync: optional array of sync_len int32 counters that is ZERO on first use (the kernel leaves it
 * zero): when given, and the whole grid is resident on the chip at once (small batches), the two
 * passes run as ONE launch whose workgroups hand their partial sums over through these counters;
 * NULL selects the two-launch form.  One array may serve every call on the same stream.
 * partials_in: optional statistics already produced by idb_gemm (idb_gemm_desc.gn_partials) for x0 (then x1 must be NULL);
 * partials_chunks = hw / 64.  Only the normalise pass is launched.
 * ------------------------------------------------------------------------------------------ */
size_t idb_groupnorm_workspace_bytes(int32_t batch, int32_t hw, int32_t groups);
int idb_groupnorm(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t batch, int32_t hw,
                  int32_t groups, float eps, const float* gamma, const float* beta, int32_t silu,
                  void* out, int32_t dtype, void* workspace, size_t workspace_bytes, int32_t* sync,
                  int32_t sync_len, const float* partials_in, int32_t partials_chunks, void* stream);
int idb_layernorm(const void* x, void* out, int64_t rows, int32_t c, float eps, const float* gamma,
                  const float* beta, int32_t dtype, void* stream);
/* Host-only: what idb_groupnorm would launch for these arguments (same validation of the dims, no HIP call).  sync_len: length of
 * the hand-off counter array, 0 without one; partials_chunks: 0 without partials_in.  form: 0 two launches (statistics, normalise),
 * 1 single launch with hand-off, 2 normalise only (partials_in); slice_channels x slices = C0 + C1: the channel slice one workgroup
 * owns; chunks x chunk_len >= hw: the pixel chunks of the statistics ([batch][chunks][groups][2] partials; idb_groupnorm_stats
 * reports the chunks of form 0); rows_per_pass: pixels one workgroup covers per step (256 / (slice_channels / 8));
 * apply_blocks: pixel blocks of the normalise launch (0 in form 1).  idb_groupnorm_fp8 launches what sync_len = 0 reports. */
int idb_groupnorm_plan(int32_t c0, int32_t c1, int32_t batch, int32_t hw, int32_t groups, int32_t sync_len, int32_t partials_chunks,
                       int32_t* form, int32_t* slice_channels, int32_t* slices, int32_t* chunks, int32_t* chunk_len,
                       int32_t* rows_per_pass, int32_t* apply_blocks);
/* First GroupNorm pass only: partial {sum, sum of squares} per (sample, pixel chunk, group) of the channel concatenation x0 | x1,
 * fp32 [batch][*chunks][groups][2] in `partials` (capacity: idb_groupnorm_workspace_bytes) — for callers that
 * want the statistics of a tensor whose producer did not emit them (skip concatenations, conv_in).  *chunks receives the pixel-chunk count (<= 64). */
int idb_groupnorm_stats(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t batch, int32_t hw, int32_t groups,
                        float* partials, size_t partials_bytes, int32_t* chunks, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4/K5 — fused attention, head_dim 64: out = softmax(Q K^T * scale) V, online softmax in fp32.
 * Replaces F.scaled_dot_product_attention in AttnProcessor2_0 (self- and cross-attention).
 * q: [batch][n_q][heads*64] with row stride q_ld; k, v: [batch][n_kv_alloc][...] with row stride
 * kv_ld (n_kv_alloc rows allocated per batch entry, only the first n_kv are attended).
 * ------------------------------------------------------------------------------------------ */
int idb_attention(const void* q, int32_t q_ld, const void* k, const void* v, int32_t kv_ld,
                  void* out, int32_t out_ld, int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv,
                  int32_t n_kv_alloc, float scale, int32_t causal, int32_t dtype, void* stream);
/* causal != 0: query i attends keys 0..i only (CLIPTextModel's causal mask, n_q == n_kv). */
/* Host-only: the kernel form idb_attention would launch for these arguments (same validation of the dims, no HIP
 * call).  waves: 2, 4, 8 or 12 per workgroup; key_split: 1 or 2; rows: query rows per workgroup (64/128/192);
 * blocks: workgroups in the grid. */
int idb_attention_plan(int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t causal,
                       int32_t* waves, int32_t* key_split, int32_t* rows, int32_t* blocks);

/* Token + position embedding gather of CLIPTextModel: out[b][t][:] = tok[ids[b][t]][:] + pos[t][:]
 * (fp32 tables, operand-dtype output).  ids are int64 on the device; out-of-range ids are an error the
 * caller must exclude (checked on the host by the engine). */
int idb_embed_tokens(const int64_t* ids, const float* tok, const float* pos, void* out, int32_t batch,
                     int32_t n_tokens, int32_t dim, int32_t dtype, void* stream);
/* In-place row softmax over [rows][cols] (VAE mid-block single-head attention, d = 512). */
int idb_softmax_rows(void* x, int64_t rows, int32_t cols, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K7 — time embedding path in fp32: y = act_in(x) W^T + b for tiny M (30 timesteps).
 * Replaces Timesteps/TimestepEmbedding and ResnetBlock2D.time_emb_proj.
 * ------------------------------------------------------------------------------------------ */
int idb_timestep_sinusoid(const float* timesteps, float* out, int32_t n, int32_t dim, void* stream);
int idb_linear_f32(const float* x, const float* w, const float* bias, float* y, int32_t m, int32_t n,
                   int32_t k, int32_t silu_in, void* stream);

/* ------------------------------------------------------------------------------------------
 * conv_in (Cin = 4): fp32 NCHW latents -> operand-dtype NHWC features; `rep` replicates the batch
 * (CFG feeds the same latents twice).  Replaces UNet conv_in / VAE post_quant_conv + conv_in.
 * ------------------------------------------------------------------------------------------ */
int idb_conv_in(const float* x_nchw, const float* w, const float* bias, void* out, int32_t batch,
                int32_t rep, int32_t cin, int32_t h, int32_t w_, int32_t cout, float in_scale,
                const float* pre_w, const float* pre_b, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8 — classifier-free guidance + DDPMScheduler.step, fp32 (inference_ID-Booth.py:104,138;
 * train_ID-Booth.py:1081).  eps is [2B][HW][C] fp32 (uncond first); latents/noise are NCHW fp32.
 * coef points at 6 floats on the DEVICE: {sqrt_alpha_bar_t, sqrt_beta_bar_t, c_x0, c_x, sigma,
 * guidance_scale}; prediction_type 0 = epsilon, 1 = v_prediction.  x0_out may be NULL.
 * ------------------------------------------------------------------------------------------ */
int idb_cfg_ddpm_step(const float* eps, float* latents, const float* noise, const float* coef,
                      float* x0_out, int32_t batch, int32_t channels, int32_t hw, int32_t cfg,
                      int32_t prediction_type, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8b — classifier-free guidance + PNDMScheduler.step (PLMS, skip_prk_steps), fp32, one launch per step
 * (train_ID-Booth.py:562-583, :1211: the pipeline's default scheduler for SD-2.1).  eps is
 * [rep*B][HW][C] fp32 (uncond first; rep 1 = no guidance, 2 = CFG); latents are NCHW fp32, updated in place.
 * hist: IDB_PLMS_SLOTS NCHW fp32 slots of past guided eps, saved: one NCHW fp32 sample, both owned by the caller.
 * coef points at 9 floats on the DEVICE: {w0, w1, w2, w3, sqrt_alpha_bar_t, sqrt_beta_bar_t, c_sample, c_eps,
 * guidance_scale}.  Per element: e = e_u + g (e_c - e_u); hist[write_slot] = e unless write_slot is -1;
 * m = w0 e + w1 hist[slot1] + w2 hist[slot2] + w3 hist[slot3], the first n_terms (1..4) terms only: a slot past
 * n_terms is never read, whatever its weight; x = latents (IDB_PLMS_KEEP), latents which are also copied to
 * `saved` (IDB_PLMS_SAVE), or `saved` (IDB_PLMS_RESTORE); prediction_type 1: m = sqrt_alpha_bar m + sqrt_beta_bar x;
 * latents = c_sample x - c_eps m.  Everything structural is a host integer (fixed when a graph is captured),
 * every scalar is read on the device.  IDB_EINVAL on rep outside {1,2}, n_terms outside 1..4, a slot index
 * outside its range or a slot both read and written.
 * ------------------------------------------------------------------------------------------ */
#define IDB_PLMS_SLOTS 4
#define IDB_PLMS_KEEP 0
#define IDB_PLMS_SAVE 1
#define IDB_PLMS_RESTORE 2
int idb_cfg_plms_step(const float* eps, float* latents, float* hist, float* saved, const float* coef,
                      int32_t batch, int32_t channels, int32_t hw, int32_t rep, int32_t prediction_type,
                      int32_t write_slot, int32_t n_terms, int32_t slot1, int32_t slot2, int32_t slot3,
                      int32_t sample_mode, void* stream);

/* K10 — VaeImageProcessor.postprocess + save_image quantisation:
 * x [B][HW][C] fp32 -> img01 = clamp(x/2+0.5,0,1) (fp32 NHWC, may be NULL) and u8 = floor(255*img01+0.5). */
int idb_postprocess(const float* x, float* img01, uint8_t* u8, int64_t count, void* stream);

/* [B][HW][C] operand dtype -> [B][C][HW] fp32 (API boundary: unet(...)[0], vae.decode(...).sample). */
int idb_nhwc_to_nchw_f32(const void* x, float* out, int32_t batch, int32_t hw, int32_t c, int32_t dtype,
                         void* stream);
int idb_f32_nhwc_to_nchw(const float* x, float* out, int32_t batch, int32_t hw, int32_t c, void* stream);
/* [rows][cols] fp32 -> operand dtype (prompt embeddings). */
int idb_cast_f32(const float* x, void* out, int64_t count, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Face align-and-crop warp: cv2.warpAffine(img, M, (out_w, out_h), borderValue) for 8-bit images with
 * OpenCV's defaults (INTER_LINEAR, BORDER_CONSTANT) — utils/detect_align_crop_data.py:180.  src: uint8 [batch][h][w][channels];
 * m_inv: [batch][6] doubles, the INVERSE of each 2x3 matrix (cv::invertAffineTransform, computed on the host in double);
 * coordinates in 10-bit fixed point with a 5-bit sub-pixel fraction, 15-bit integer tap weights: integer-exact.
 * ------------------------------------------------------------------------------------------ */
int idb_warp_affine_u8(const uint8_t* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const double* m_inv,
                       uint8_t* dst, int32_t out_h, int32_t out_w, int32_t border_value, void* stream);

/* ------------------------------------------------------------------------------------------
 * MTCNN face detector (facenet_pytorch P-Net / R-Net / O-Net as used at
 * utils/detect_align_crop_data.py:18-20,99).  fp32 NCHW activations; the cascade's control logic (image pyramid, box generation,
 * NMS, regression) is host code in faceposegenerator_amd/mtcnn.py.
 *   idb_crop_resize_area_u8: out[k] = (F.interpolate(src[image_k, y0:y1, x0:x1], (out_h, out_w), mode="area") - sub) * mul for
 *       boxes [n][5] = {image, y0, y1, x0, x1} (int32 on the device, exclusive ends, clipped by the caller); uint8 NHWC in,
 *       fp32 [n][channels][out_h][out_w] out (upstream imresample + the (x - 127.5) / 128 normalisation)
 *   idb_conv2d_f32: nn.Conv2d(cin, cout, (kh, kw)) (stride 1, no padding) + optional nn.PReLU(cout); also the dense layers
 *       (a kernel as large as the map)
 *   idb_maxpool2d_f32: nn.MaxPool2d(k, stride, ceil_mode=True) over `planes` = batch * channels maps
 *   idb_softmax_pairs_f32: softmax over a channel pair, p1 = softmax(x[b][0:2][i])[1]
 *   idb_nms_mask: the suppression bit matrix of greedy NMS (torchvision.ops.batched_nms as detect_face.py calls it, use_min = 0, and
 *       upstream's nms_numpy "Min" with +1 widths, use_min = 1 / plus_one = 1): boxes fp32 [n][4] SORTED by descending score, optional
 *       image index int32 [n] (boxes of different images never suppress each other); mask uint64 [n][(n+63)/64], bit j of row i set
 *       when box i would remove box j > i.  The greedy scan over the rows stays with the caller (host: a few hundred words).
 *   Limits (IDB_EINVAL before any launch): one image or activation plane h * w < 2^31 elements and a filter cin * kh * kw < 2^31 (the
 *       kernels index inside them with int); pooling h, w <= 2^30 and k, stride <= 2^20; at most 2^28 boxes and, for idb_nms_mask, 2^20;
 *       fewer than 2^39 outputs per call; n = 0 boxes is IDB_OK without a launch.
 * ------------------------------------------------------------------------------------------ */
int idb_crop_resize_area_u8(const uint8_t* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* boxes, int32_t n,
                            float* out, int32_t out_h, int32_t out_w, float sub, float mul, void* stream);
int idb_conv2d_f32(const float* x, const float* w, const float* bias, const float* prelu, float* y, int32_t batch, int32_t cin, int32_t h,
                   int32_t w_, int32_t cout, int32_t kh, int32_t kw, void* stream);
int idb_maxpool2d_f32(const float* x, float* y, int32_t planes, int32_t h, int32_t w, int32_t k, int32_t stride, void* stream);
int idb_softmax_pairs_f32(const float* x, float* p1, int32_t batch, int32_t hw, void* stream);
int idb_nms_mask(const float* boxes, const int32_t* image, int32_t n, float thr, int32_t use_min, int32_t plus_one, uint64_t* mask,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * fp8 (OCP e4m3) implicit GEMM on v_mfma_scale_f32_16x16x128_f8f6f4 — BASELINE configs[4] "fp8 MFMA weight path" (the 768x768
 * v-prediction checkpoint selected at inference_ID-Booth.py:63-64,103), kernel level: out[m][n] = x_scale * w_scale[n] *
 * sum_k x8[m][k] * w8[n][k] (+ bias, per-sample bias, residual), both operands 8-bit, fp32 accumulation, operand-dtype output.
 * One source: NHWC fp8 [batch][in_h][in_w][channels] (taps 9: 3x3, padding 1; taps 1: the pixel itself), channels % 64 == 0.
 *   idb_quantize_fp8: out8 = e4m3(x * inv_scale), saturating at +-448 (x: bf16/f16, count % 8 == 0)
 *   idb_pack_weight_fp8: fp32 torch layout [cout][cin][ktaps] -> fp8 [cout][ktaps][cin rounded up to 128] (zero columns) with one
 *       scale per output channel, scales[n] = absmax(row n) / 448
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t out_dtype;            /* IDB_BF16 / IDB_F16: dtype of `out` and `residual` */
    int32_t batch, out_h, out_w, stride, n;
    const void* x;                /* fp8 e4m3 NHWC */
    int32_t channels, taps, in_h, in_w, upsample;
    float x_scale;                /* real value = x_scale * fp8 value (per tensor) */
    const void* w;                /* idb_pack_weight_fp8 layout */
    const float* w_scale;         /* [n] */
    const float* bias;
    const float* sample_bias;
    int32_t sample_bias_ld;
    const void* residual;
    void* out;
    int32_t out_ld;
    float* gn_partials;           /* optional out, as idb_gemm_desc.gn_partials: written by the kernel's own epilogue when the column tiles
                                     hold whole groups (n % 160 == 0, 160 % (n / gn_groups) == 0, out_h*out_w % 64 == 0, out_ld == n),
                                     else by an extra statistics launch */
    int32_t gn_groups;
} idb_gemm_fp8_desc;
int idb_quantize_fp8(const void* x, void* out, int64_t count, float inv_scale, int32_t dtype, void* stream);
/* idb_groupnorm (two-launch form) writing its output as fp8 e4m3 of y * out_inv_scale, saturating: the activation operand of
 * idb_gemm_fp8 straight from the normalisation — GroupNorm+SiLU outputs are bounded, so a fixed per-tensor scale serves. */
int idb_groupnorm_fp8(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t batch, int32_t hw, int32_t groups, float eps,
                      const float* gamma, const float* beta, int32_t silu, void* out8, float out_inv_scale, int32_t dtype,
                      void* workspace, size_t workspace_bytes, const float* partials_in, int32_t partials_chunks, void* stream);
int idb_pack_weight_fp8(const float* src, void* dst, float* scales, int32_t cout, int32_t cin, int32_t ktaps, void* stream);
int idb_gemm_fp8(const idb_gemm_fp8_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * ArcFace IResNet (insightface arcface_torch iresnet.py; ID-Booth's identity network) — the layers that are not idb_gemm calls.
 *   idb_arcface_stem: conv1 3->64 (3x3, stride 1, pad 1) with bn1 folded into `weight` (fp32 [64][3][3][3] as [cout][ky][kx][cin]) and
 *       `bias` (fp32 [64]), then PReLU (`slope` [64]).  x: uint8 NHWC crops [batch][h][w][3] when x_u8 (preprocessing
 *       (x / 255 - 0.5) / 0.5 fused), else normalised fp32 NCHW [batch][3][h][w]; the input is rounded to the operand dtype first.
 *       out: NHWC [batch][h][w][64] operand dtype; out2 (optional, as idb_gemm_desc.out2): fma(out, out2_scale, out2_shift) rounded.
 *       w <= 256.
 *   idb_arcface_head: y[m][n] = sum_k float(x[m][k]) * w[n][k] + bias[n] in fp32 (head bn2 + fc + features folded into w / bias),
 *       x operand dtype [m][k], w fp32 [n][k]; n % 64 == 0, k % 32 == 0; K-sliced with a deterministic reduce through `workspace`
 *       (idb_arcface_head_workspace_bytes).
 * ------------------------------------------------------------------------------------------ */
int idb_arcface_stem(const void* x, int32_t x_u8, int32_t batch, int32_t h, int32_t w, const float* weight, const float* bias,
                     const float* slope, const float* out2_scale, const float* out2_shift, void* out, void* out2, int32_t dtype,
                     void* stream);
size_t idb_arcface_head_workspace_bytes(int32_t m, int32_t n, int32_t k);
int idb_arcface_head(const void* x, const float* w, const float* bias, float* y, int32_t m, int32_t n, int32_t k, int32_t dtype,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 6DRepNet head pose (sixdrepnet SixDRepNet_Detector: RepVGG-B1g2 deploy form + 6D rotation head; ID-Booth's pose evaluation) — the
 * layers that are not idb_gemm calls (the 27 3x3 blocks are idb_gemm with act = 3).
 *   idb_resize_aa_u8: uint8 HWC RGB [batch][s][s][3] -> constant-zero border of `pad` pixels -> Pillow's antialiased BILINEAR resize
 *       (Image.resize((d, d), BILINEAR), 8-bit fixed point) -> [batch][d][d][3]; bit-exact with Pillow.  d <= 256, at most 16 taps
 *       per axis ((s + 2 pad) / d <= 7).
 *   idb_pose_stem: conv 3->64 (3x3, stride 2, pad 1) + bias + ReLU; weight fp32 [64][3][3][3] as [cout][ky][kx][cin].  x: uint8 NHWC
 *       [batch][h][w][3] when x_u8 (ToTensor + ImageNet Normalize fused, fp32), else normalised fp32 NCHW [batch][3][h][w].
 *       out: NHWC [batch][ceil(h/2)][ceil(w/2)][64] operand dtype.  w <= 512.
 *   idb_pose_head: global average pool of x [batch][hw][c] (operand dtype, fixed summation order), linear c->6 (weight fp32 [6][c],
 *       bias [6]), Gram-Schmidt to R (fp32 [batch][3][3], the columns x y z) and Euler angles (fp32 [batch][3]: pitch, yaw, roll in
 *       degrees).  c % 8 == 0; deterministic.
 * ------------------------------------------------------------------------------------------ */
int idb_resize_aa_u8(const void* src, int32_t batch, int32_t s, int32_t pad, int32_t d, void* dst, void* stream);
int idb_pose_stem(const void* x, int32_t x_u8, int32_t batch, int32_t h, int32_t w, const float* weight, const float* bias, void* out,
                  int32_t dtype, void* stream);
int idb_pose_head(const void* x, int32_t batch, int32_t hw, int32_t c, const float* weight, const float* bias, float* rot, float* angles,
                  int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * DINOv2 ViT image encoder (facebookresearch/dinov2 DinoVisionTransformer, ViT-S/B/L with 14x14 patches; the `--model dinov2` encoder of
 * ID-Booth's dgm-eval run) — the layers that are not idb_layernorm / idb_gemm / idb_attention calls.
 *   idb_resize_bicubic_aa_u8: replaces torchvision Resize((d, d), BICUBIC) on a PIL image = Image.resize((d, d), BICUBIC): uint8 HWC RGB
 *       [batch][s][s][3] -> [batch][d][d][3] with Pillow's antialiased Keys cubic (a = -0.5, support 2 max(s / d, 1)), 22-bit fixed-point
 *       coefficients, horizontal pass clipped to 8 bits, then the vertical pass; bit-exact with Pillow.  d <= 256, at most 16 taps per
 *       axis (ceil(2 s / d) <= 7: 768 -> 224 needs 15); a larger reduction is IDB_EINVAL before any launch.
 *   idb_vit_patchify: replaces the unfold of PatchEmbed.proj (Conv2d(3, D, 14, stride 14)): 224x224 input -> [batch * 256][640] operand
 *       dtype, one row per patch in row-major patch order, column (c * 14 + ky) * 14 + kx (the conv weight's own flattening), columns
 *       588..639 zero.  x: uint8 NHWC [batch][224][224][3] when x_u8 (ToTensor + ImageNet Normalize fused, fp32), else normalised fp32
 *       NCHW [batch][3][224][224].
 *   idb_vit_tokens: replaces prepare_tokens_with_masks (no masks): out[b][0] = cls + pos[0], out[b][1 + t] = patches[b n_patches + t] +
 *       pos[1 + t]; cls [dim] and pos [1 + n_patches][dim] fp32, patches / out operand dtype, fp32 add, one rounding.  dim % 8 == 0.
 *   idb_vit_head: replaces the final nn.LayerNorm for x_norm_clstoken (head = Identity): LayerNorm of row b * row_stride of x [..][dim]
 *       (operand dtype) for b < batch, in fp32 (two passes, fixed summation order: deterministic) -> fp32 [batch][dim].
 * ------------------------------------------------------------------------------------------ */
int idb_resize_bicubic_aa_u8(const void* src, int32_t batch, int32_t s, int32_t d, void* dst, void* stream);
int idb_vit_patchify(const void* x, int32_t x_u8, int32_t batch, void* out, int32_t dtype, void* stream);
int idb_vit_tokens(const void* patches, const float* cls, const float* pos, void* out, int32_t batch, int32_t n_patches, int32_t dim,
                   int32_t dtype, void* stream);
int idb_vit_head(const void* x, int64_t row_stride, int32_t batch, int32_t dim, const float* gamma, const float* beta, float eps, float* out,
                 int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * All-pairs metrics over fp32 image features [N][D] (dgm-eval's PRDC, KD and AuthPct as ID-Booth's evaluation runs them on DINOv2
 * features), on the exact f32-input MFMA.  d2(i, j) = max(|a_i - s|^2 + |b_j - s|^2 - 2 (a_i - s).(b_j - s), 0) with the caller's
 * shift s [D] (NULL: none) subtracted where the operands are loaded; any d >= 1 (K is zero-padded in the kernel), rows dense with
 * stride d.  Only idb_pair_dist2 writes the N x N matrix.  Every entry takes a workspace of idb_pair_workspace_bytes(mode, ...) bytes,
 * 16-byte aligned, writes all of its outputs, uses integer atomics and fixed-order float sums only (bit-identical from run to run)
 * and validates its arguments before any HIP call.  n <= 2^22, d <= 2^16.
 *   idb_pair_workspace_bytes(mode, na, nb, subsets): mode IDB_PAIR_*; KNN takes n as na; POLY takes the subset size m as na and the
 *       number of subsets; 0 for arguments the entry would refuse.
 *   idb_pair_dist2: replaces sklearn.metrics.pairwise_distances(a, b) ** 2 / torch.cdist(a, b) ** 2: out [na][nb].  The test hook
 *       that pins the engine's numerics, and the form for tiny inputs.
 *   idb_pair_knn_radii: replaces prdc.py's compute_nearest_neighbour_distances (get_kth_value(pairwise_distances(x, x), k =
 *       nearest_k + 1)), squared: r2[i] = the kth smallest of row i of d2(x, x) with the diagonal forced to exactly 0 (the point
 *       itself is the first), equal distances counted with their multiplicity.  1 <= kth <= min(8, n).
 *   idb_pair_prdc_counts: replaces the three N x N comparisons of prdc.py's compute_prdc in one pass over d2(real, gen), given the
 *       squared radii of both sets: in_real_sphere[j] = #{i : d2(i, j) < r2_real[i]} (precision = mean(> 0), density = sum / (k ng)),
 *       covered[i] = any_j d2(i, j) < r2_gen[j] as 0 / 1 (recall), row_min[i] = min_j d2(i, j) (coverage = mean(row_min < r2_real)).
 *   idb_pair_nearest: replaces torch.cdist(a, b).min(dim = 0) of authpct.py: min_d2[j] = min_i d2(i, j) and argmin[j] = that i, the
 *       lowest on an exact tie; exclude_diag leaves i == j out (a set against itself; needs na >= 2).
 *   idb_pair_poly_sums: replaces the three polynomial_kernel matrices of mmd.py's polynomial_mmd, per subset: rows idx_x[s][m] of x
 *       [nx][d] and idx_y[s][m] of y [ny][d] (int32 device arrays, every index in range: not checked) are gathered where the operands
 *       are loaded, k(a, b) = (gamma a.b + coef0)^3 on the unshifted features; sums[s][0] = sum_{i != j} k(x_i, x_j), sums[s][1] =
 *       sum_{i != j} k(y_i, y_j), sums[s][2] = sum_{i, j} k(x_i, y_j), double: fp32 per 128 x 128 tile, the tiles added in row-major
 *       order in double on the device.  One launch covers the 3 * subsets matrices; subsets <= 21845, 2 <= m <= min(nx, ny).
 * ------------------------------------------------------------------------------------------ */
#define IDB_PAIR_DIST2 0
#define IDB_PAIR_KNN 1
#define IDB_PAIR_PRDC 2
#define IDB_PAIR_NEAREST 3
#define IDB_PAIR_POLY 4
size_t idb_pair_workspace_bytes(int32_t mode, int32_t na, int32_t nb, int32_t subsets);
int idb_pair_dist2(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const float* shift, float* out, void* ws,
                   size_t ws_bytes, void* stream);
int idb_pair_knn_radii(const float* x, int32_t n, int32_t d, const float* shift, int32_t kth, float* r2, void* ws, size_t ws_bytes,
                       void* stream);
int idb_pair_prdc_counts(const float* real, int32_t nr, const float* gen, int32_t ng, int32_t d, const float* shift, const float* r2_real,
                         const float* r2_gen, int32_t* in_real_sphere, int32_t* covered, float* row_min, void* ws, size_t ws_bytes,
                         void* stream);
int idb_pair_nearest(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const float* shift, int32_t exclude_diag,
                     float* min_d2, int32_t* argmin, void* ws, size_t ws_bytes, void* stream);
int idb_pair_poly_sums(const float* x, int32_t nx, const float* y, int32_t ny, int32_t d, const int32_t* idx_x, const int32_t* idx_y,
                       int32_t subsets, int32_t m, float gamma, float coef0, double* sums, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Identity-verification statistics (ID-Booth's Evaluation/PyEER_analysis: genuine / impostor cosine scores of ArcFace embeddings, then
 * pyeer's get_eer_stats).  Everything is double.  Every entry validates its arguments before any HIP call, writes all of its outputs,
 * uses fixed-order float sums and no float atomics (bit-identical from run to run) and never synchronises.
 *   idb_verif_cos_scores: replaces utils.pairwise_cos_sim (1 - scipy.spatial.distance.cosine(e1, e2) per pair, a Python loop in 5-10
 *       processes): out[p] = 1 - clip(1 - uv / sqrt(uu vv), 0, 2) for rows u = a[idx_a[p]], v = b[idx_b[p]] of the dense fp32 matrices
 *       a [na][d], b [nb][d] (a == b allowed); uv, uu, vv summed in double from the fp32 operands (exact products), all three in one
 *       order, so a row against itself is within 2^-52 of 1.  idx_a, idx_b: int32 [n_pairs] device arrays; an index out of range
 *       reads nothing and gives NaN, as does a zero row (upstream's 0 / 0).  Any d >= 1 (16-byte loads when d % 4 == 0 and both
 *       bases are 16-byte aligned), 1 <= n_pairs <= 2^30.
 *   idb_verif_workspace_bytes(ng, ni): the workspace of idb_verif_roc; 0 for counts it would refuse.
 *   idb_verif_roc: replaces pyeer's calculate_roc (a Python sort of (score, label) tuples, cumsum, unique) and the reductions of
 *       get_eer_stats over it, from the ascending finite score arrays g_sorted [ng] and i_sorted [ni], 1 <= ng, ni <= 2^30.  The
 *       thresholds are the distinct scores; at threshold t, fnm = #{genuine < t}, fm = #{impostor >= t}, fmr = fm / ni and fnmr =
 *       fnm / ng as IEEE double quotients.  points [IDB_VERIF_POINTS] receives the threshold of every selected point below and ints
 *       [2 p], ints [2 p + 1] its fm and fnm (NaN and -1, -1 when no threshold qualifies, which only the two EER points can):
 *         IDB_VERIF_EER_T2 the smallest t with fmr - fnmr <= 0; IDB_VERIF_EER_T1 the largest t with fmr - fnmr > 0 (get_eer_values;
 *           the caller chooses between them and handles the no-crossing case as upstream does);
 *         IDB_VERIF_FMR0 / 1000 / 100 / 20 / 10 the first (smallest t) argmin of |fmr - op|, op = 0, 0.001, 0.01, 0.05, 0.1 (get_fmr_op);
 *         IDB_VERIF_FNMR0 / 100 / 1000 the last (largest t) argmin of |fnmr - op|, op = 0, 0.01, 0.001 (get_fnmr_op);
 *         IDB_VERIF_YOUDEN the first argmax of 1 - fnmr - fmr (get_youden_index); IDB_VERIF_MCC the first argmax of upstream's
 *           Matthews expression, separate square roots and a zero denominator replaced by 1 (get_matthews_ccoef);
 *         IDB_VERIF_FIRST the smallest threshold (upstream's index 0).
 *       ints [2 IDB_VERIF_POINTS + 0] = the number of thresholds, [+ 1] = those with fmr - fnmr <= 0, [+ 2] = the exact integer
 *       2 ni ng AUC = the sum over consecutive thresholds of (fm1 - fm2) (2 ng - fnm1 - fnm2) (calculate_roc_auc; <= 2^61).
 *       moments [4] = gmean, gstd, imean, istd: np.mean and np.std (population, two passes).  ws 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define IDB_VERIF_POINTS 13
#define IDB_VERIF_EER_T2 0
#define IDB_VERIF_EER_T1 1
#define IDB_VERIF_FMR0 2
#define IDB_VERIF_FMR1000 3
#define IDB_VERIF_FMR100 4
#define IDB_VERIF_FMR20 5
#define IDB_VERIF_FMR10 6
#define IDB_VERIF_FNMR0 7
#define IDB_VERIF_FNMR100 8
#define IDB_VERIF_FNMR1000 9
#define IDB_VERIF_YOUDEN 10
#define IDB_VERIF_MCC 11
#define IDB_VERIF_FIRST 12
int idb_verif_cos_scores(const float* a, int32_t na, const float* b, int32_t nb, int32_t d, const int32_t* idx_a, const int32_t* idx_b,
                         int32_t n_pairs, double* out, void* stream);
size_t idb_verif_workspace_bytes(int32_t ng, int32_t ni);
int idb_verif_roc(const double* g_sorted, int32_t ng, const double* i_sorted, int32_t ni, double* points, int64_t* ints, double* moments,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The LFW-style 10-fold pair benchmark of a face-recognition backbone (ID-Booth's FR_training/utils/verification.py, behind
 * test_FR.py's accuracies on LFW, CFP-FP, AgeDB-30, CALFW, CPLFW).  Everything is double.  Every entry validates its arguments before
 * any HIP call, uses fixed-order float sums and no float atomics (bit-identical from run to run) and never synchronises.
 *   idb_frb_pair_dist: replaces embedding_preprocessing (embeddings_list[0] + embeddings_list[1], sklearn.preprocessing.normalize, the
 *       per-row np.linalg.norm loop behind _xnorm) and calculate_roc's np.subtract / np.square / np.sum.  e0, e1: dense fp32
 *       [2 n_pairs][d], the embeddings of the images and of their horizontal mirrors; rows 2p and 2p + 1 are pair p.  Per row
 *       s = (double) e0 + (double) e1 (exact), n = sqrt(sum s_k^2), x = s / n, or x = s when n == 0 (sklearn's rule for a zero row);
 *       dist[p] = sum_k (x[2p][k] - x[2p+1][k])^2.  norms: double [2][2 n_pairs], the Euclidean norms of the rows of e0, then of e1
 *       (upstream's _xnorm is their mean).  Both rows of a pair take the same elements in the same order: identical inputs give
 *       exactly 0.  1 <= n_pairs <= 2^30, 1 <= d <= 8192 (16-byte loads when d % 4 == 0 and both bases are 16-byte aligned).
 *   idb_frb_workspace_bytes(n_pairs, nfolds, n_thr): the workspace of idb_frb_fold_counts; 0 for arguments it would refuse.
 *   idb_frb_fold_counts: replaces the calculate_accuracy loops of calculate_roc (nfolds x 2 x n_thr numpy passes over the pairs).
 *       dist: double [n_pairs]; issame: uint8 [n_pairs], non-zero = same identity; fold_start: int32 [nfolds + 1] device array, fold f
 *       is the contiguous test block [fold_start[f], fold_start[f + 1]) of KFold(n_splits, shuffle=False) (a pair outside
 *       [fold_start[0], fold_start[nfolds]) is counted nowhere); thresholds: double [n_thr], non-decreasing.  counts: int32
 *       [nfolds][n_thr][2], [f][t][0] = #{p in fold f : issame[p] and dist[p] < thresholds[t]}, [f][t][1] the same for not issame[p];
 *       the comparison is np.less, strict, double against double (a NaN distance is below nothing).  A histogram over
 *       u = #{t : thresholds[t] <= dist[p]} per (fold, label) with integer atomics, then a prefix sum over t:
 *       O(n_pairs log n_thr + nfolds n_thr).  1 <= n_pairs <= 2^30, 1 <= nfolds <= min(64, n_pairs), 1 <= n_thr <= 16384; ws 16-byte
 *       aligned.
 * ------------------------------------------------------------------------------------------ */
int idb_frb_pair_dist(const float* e0, const float* e1, int32_t n_pairs, int32_t d, double* dist, double* norms, void* stream);
size_t idb_frb_workspace_bytes(int32_t n_pairs, int32_t nfolds, int32_t n_thr);
int idb_frb_fold_counts(const double* dist, const uint8_t* issame, int32_t n_pairs, const int32_t* fold_start, int32_t nfolds,
                        const double* thresholds, int32_t n_thr, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CR-FIQA face-image quality (ID-Booth's Evaluation/CR-FIQA/getQualityScore_FR_ID-Booth_12-2024.py: an IResNet with a `qs` linear
 * head, run on the whole generated image squashed to 112x112) — the two pieces that are not ArcFace IResNet calls.  Both validate
 * their arguments before any HIP call and never synchronise.
 *   idb_resize_linear_u8: replaces `image = cv2.resize(image, (112, 112))` of get_batch_feature (:61; OpenCV INTER_LINEAR on 8-bit data) and,
 *       with swap_rb, the BGR order `cv2.imread(image_path)` (:59) delivers: uint8 NHWC [batch][h][w][3] -> [batch][dh][dw][3], channels 0
 *       and 2 exchanged on the way out when swap_rb.  h, w, dh, dw are independent (1..32768 each).  The caller supplies OpenCV's
 *       per-axis tables, built on the host in OpenCV's float32 / float64 types (fiqa.coef_tables): ofs_* int32 [d] = the first source
 *       index, coef_* int16 [d][2] = the two taps on an 11-bit scale (c0 + c1 = 2048); the second tap is min(ofs + 1, size - 1).  The
 *       kernel is integer arithmetic only (int32 horizontal pass, then (((b0 (r0 >> 4)) >> 16) + ((b1 (r1 >> 4)) >> 16) + 2) >> 2),
 *       and clamps the offsets to the image.  h == 2 dh and w == 2 dw takes OpenCV's 2x2 box (a + b + c + d + 2) >> 2 instead (the
 *       tables are then unused but still required).  The tables must be 4-byte aligned.
 *   idb_fiqa_tail: replaces `qs = self.qs(x)` of iresnet.py's forward (:178) and `features = normalize(features)` (:72; sklearn, l2) of
 *       get_batch_feature, on emb fp32 [batch][d] (the output of idb_arcface_head): qs[b] = fp32(sum_i emb[b][i] weight[i] + bias[0]) and
 *       emb_norm[b] = fp32(emb[b] / sqrt(sum_i emb[b][i]^2)), both sums in double in a fixed order (no atomics: bit-identical from run
 *       to run), one rounding each; a zero row stays zero.  weight fp32 [d], bias fp32 [1], device memory.  1 <= d <= 8192.
 * ------------------------------------------------------------------------------------------ */
int idb_resize_linear_u8(const void* src, int32_t batch, int32_t h, int32_t w, const int32_t* ofs_x, const int16_t* coef_x,
                         const int32_t* ofs_y, const int16_t* coef_y, int32_t dh, int32_t dw, int32_t swap_rb, void* dst, void* stream);
int idb_fiqa_tail(const float* emb, const float* weight, const float* bias, int32_t batch, int32_t d, float* qs, float* emb_norm,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * AutoencoderKL.encode tail (train_ID-Booth.py:1001-1002): DiagonalGaussianDistribution.sample()/.mode() times
 * vae.config.scaling_factor.  moments: fp32 [batch][hw][2*channels] (mean channels first, then log-variance), the
 * output of the encoder's conv_out with quant_conv folded in; noise: NCHW fp32 [batch][channels][hw] or NULL (mode);
 * latents, and optional mean / logvar (clamped to [-30, 20]) outputs: NCHW fp32.
 * ------------------------------------------------------------------------------------------ */
int idb_vae_sample(const float* moments, const float* noise, float scale, float* latents, float* mean_out,
                   float* logvar_out, int32_t batch, int32_t channels, int32_t hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * The training objective's forward pass (train_ID-Booth.py:996-1134, evaluated under no_grad: a checkpoint's validation losses) — the
 * kernels between vae.encode, the UNet, vae.decode, MTCNN.detect and ArcFace.  fp32 in and out, asynchronous on `stream`, no
 * synchronisation; every entry validates its arguments before any HIP call (IDB_EINVAL, or IDB_EUNSUPPORTED for a prediction type or
 * an embedding width the kernels do not implement).  Sums are accumulated in double in a fixed order without floating-point atomics:
 * bit-identical from run to run.
 *   Schedule arguments (idb_diffuse_targets, idb_objective_mse_x0): timesteps int32 [batch] and alphas_cumprod fp32 [n_train], both in
 *       device memory; sample b uses a = alphas_cumprod[t_b], sqrt(a) and sqrt(1 - a) taken in double.  A timestep outside
 *       [0, n_train) cannot be refused without a synchronisation: it is CLAMPED into the table.  prediction_type 0 = epsilon,
 *       1 = v_prediction.  1 <= batch <= 65535, channels * hw < 2^31.
 *   idb_diffuse_targets: replaces `noise_scheduler.add_noise(model_input, noise, timesteps)` (:1018) and the target selection
 *       (:1055-1058: `noise`, or `noise_scheduler.get_velocity(model_input, noise, timesteps)`) in one launch.  x0, noise, noisy, target:
 *       NCHW [batch][channels][hw].  noisy = sqrt(a) x0 + sqrt(1 - a) noise; target = noise, or sqrt(a) noise - sqrt(1 - a) x0; each
 *       evaluated in double and rounded to fp32 once.  target may be NULL.  16-byte accesses when channels * hw % 4 == 0 and every
 *       tensor is 16-byte aligned.
 *   idb_objective_mse_x0: replaces `F.mse_loss(model_pred.float(), target.float())` per sample (:1072-1074; sse[b] is the SUM of squared
 *       differences as double, the caller divides by the element count and averages the samples of a chunk) and
 *       `noise_scheduler.step(model_pred, t, noisy).pred_original_sample` (:1081, :1109), in one pass.  pred: NCHW, or with pred_nhwc the
 *       [batch][hw][channels] layout idb_gemm writes the UNet's output in; target, noisy, x0_pred: NCHW.  x0_pred (optional; needs noisy):
 *       epsilon (noisy - sqrt(1 - a) pred) / sqrt(a), v_prediction sqrt(a) noisy - sqrt(1 - a) pred, no clipping (SD-2.1's scheduler has
 *       clip_sample = false), evaluated in double and rounded once.  Per-workgroup partial sums go to ws (8-byte aligned, at least
 *       idb_objective_workspace_bytes), then one workgroup per sample adds them in ascending order; the order does not depend on pred's
 *       layout.  Two launches.
 *   idb_objective_workspace_bytes(batch, channels * hw): enough for any split of that product into channels and hw; 0 for arguments
 *       idb_objective_mse_x0 would refuse.
 *   idb_crop_resize_bilinear_f32: replaces the bounding-box crop `img[y0:y1, x0:x1]` (:1090, :1124) and cropped_image_to_arcface_input
 *       (:445-455: permute, torchvision `resize(img, (112, 112), antialias=None)`, `((img / 255) - 0.5) / 0.5`).  src: float NHWC
 *       [batch][h][w][channels] in [0, 255]; boxes as for idb_crop_resize_area_u8; out fp32 NCHW [n][channels][out_h][out_w].  The resize
 *       is F.interpolate(mode="bilinear", align_corners=False, antialias=False) restated from ATen (PARITY UNPINNED against a torchvision
 *       binary): half-pixel centres, the source coordinate clamped at 0, second tap min(i + 1, size - 1), no antialiasing when
 *       shrinking.  Coordinates and weights are computed in double and rounded to fp32 once; the taps are combined in fp32.
 *   idb_crop_resize_area_f32: idb_crop_resize_area_u8 for a float image (facenet-pytorch's detect casts a tensor image to float
 *       unrounded; the reference hands it `image * 255` as floats, latents_to_image_for_mtcnn :433-442): same boxes, sub, mul, limits
 *       and summation order; on integer-valued floats in [0, 255] the output equals the u8 entry's bit for bit.
 *   idb_identity_losses: replaces `cos(pred_arcface_features, gt_arcface_embed[0])` with nn.CosineSimilarity(dim=1, eps=1e-6) (:972,
 *       :1096), `1 - arcface_cos_similarity` (:1098) and, with neg, TripletMarginWithDistanceLoss(distance_function=cosine_distance)
 *       at its default margin 1 (:974-979, :1133; F.cosine_similarity's eps 1e-8).  feat, pos, neg: fp32 [n][d]; cos, identity,
 *       triplet: fp32 [n]; neg and triplet are both given or both NULL.  cos_eps(a, b) = a.b / (max(|a|, eps) max(|b|, eps)) (torch
 *       clamps each norm); identity = 1 - cos_1e-6(feat, pos); triplet = max((1 - cos_1e-8(feat, pos)) - (1 - cos_1e-8(feat, neg)) + 1, 0).
 *       Dot products and norms in double, one rounding per output.  1 <= d <= 8192.
 * ------------------------------------------------------------------------------------------ */
int idb_diffuse_targets(const float* x0, const float* noise, const int32_t* timesteps, const float* alphas_cumprod, int32_t n_train,
                        int32_t prediction_type, int32_t batch, int32_t channels, int32_t hw, float* noisy, float* target, void* stream);
size_t idb_objective_workspace_bytes(int32_t batch, int64_t chw);
int idb_objective_mse_x0(const float* pred, int32_t pred_nhwc, const float* target, const float* noisy, const int32_t* timesteps,
                         const float* alphas_cumprod, int32_t n_train, int32_t prediction_type, int32_t batch, int32_t channels, int32_t hw,
                         double* sse, float* x0_pred, void* ws, size_t ws_bytes, void* stream);
int idb_crop_resize_bilinear_f32(const float* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* boxes, int32_t n,
                                 float* out, int32_t out_h, int32_t out_w, void* stream);
int idb_crop_resize_area_f32(const float* src, int32_t batch, int32_t h, int32_t w, int32_t channels, const int32_t* boxes, int32_t n,
                             float* out, int32_t out_h, int32_t out_w, float sub, float mul, void* stream);
int idb_identity_losses(const float* feat, const float* pos, const float* neg, int32_t n, int32_t d, float* cos, float* identity,
                        float* triplet, void* stream);

/* ------------------------------------------------------------------------------------------
 * The FR-training input stage (ID-Booth's FR_training/utils/augmentation.py:49-54 `aug_rand_4_16` and its kin: RandomHorizontalFlip ->
 * RandAugment -> ToTensor -> Normalize(0.5, 0.5), applied there per PIL image inside DataLoader workers, utils/dataset.py:154-196).
 * Validates its arguments before any HIP call and never synchronises.
 *   idb_randaug: replaces `img.transpose(FLIP_LEFT_RIGHT)`, the op chain of FR_training/utils/rand_augment.py:_apply_op (:69-152, the
 *       13 ops of :191-210 on PIL images, interpolation NEAREST, fill None) and `ToTensor()` + `normalize`, for a uint8 RGB batch
 *       in [n][h][w][3] in ONE launch: one workgroup per image, the image in LDS for the whole chain.  flip: uint8 [n] (NULL: no flip).
 *       Slot s of image i is (slot_op[i * num_ops + s], slot_iarg[(i * num_ops + s) * 6 ...], slot_farg[i * num_ops + s]); op ids in the
 *       reference's dict order: 0 Identity, 1 ShearX, 2 TranslateX, 3 Rotate, 4 Brightness, 5 Color, 6 Contrast, 7 Sharpness,
 *       8 Posterize, 9 Solarize, 10 AutoContrast, 11 Equalize, 12 Grayscale (any other id is Identity).  The host (augment.slot_tables)
 *       supplies: for 1-3 the six 16.16 integers a0..a5 of Pillow's affine_fixed (source = ((a2 + a1 y + a0 x) >> 16, (a5 + a4 y + a3 x)
 *       >> 16), black outside; every read is range-checked); for 4-7 farg = the blend factor 1 + magnitude (Image.blend in float32
 *       against black / luma / the mean luma / ImageFilter.SMOOTH, no FMA); for 8 iarg[0] = the bit mask; for 9 farg = the threshold.
 *       10 and 11 build their per-channel LUTs from an LDS histogram (integer atomics, a fixed-order prefix sum; the AutoContrast
 *       LUT in double): bit-identical from run to run.  out_u8: uint8 [n][h][w][3] (the augmented image) or NULL; out_f32_nchw: fp32
 *       [n][3][h][w] = ((x / 255) - 0.5) / 0.5, each step rounded once, or NULL; at least one.  num_ops >= 0 (0: flip and conversion only;
 *       the slot pointers may then be NULL).  n >= 1, h, w >= 8: IDB_EINVAL otherwise.  h * w * 3 > 49152 bytes (128 x 128): IDB_EUNSUPPORTED
 *       — two image buffers plus the tables must fit the LDS of a CU.  `in` is only read.  Slot arrays and out_f32_nchw 4-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int idb_randaug(const uint8_t* in, int32_t n, int32_t h, int32_t w, const uint8_t* flip, const int32_t* slot_op, const int32_t* slot_iarg,
                const float* slot_farg, int32_t num_ops, uint8_t* out_u8, float* out_f32_nchw, void* stream);

/* ------------------------------------------------------------------------------------------
 * The FR-training loss head (ID-Booth's FR_training/utils/losses.py: CosFace :58-81, ArcFace :32-55, AdaFace :126-204, then
 * train_FR.py:288 CrossEntropyLoss and :302 / :373-377 multi_class_acc), forward only, fp32 operands on the exact f32-input MFMA.
 * Every entry validates its arguments before any HIP call, uses fixed-order sums and no floating-point atomics (bit-identical from
 * run to run) and never synchronises.
 *   idb_head_pack: replaces `l2_norm(self.kernel, axis=0)` (losses.py:26-29, :44 / :70 / :161, recomputed upstream on every call).
 *       kernel: fp32 [d][c] row-major, as torch stores the parameter.  wn: fp32 [c][d], column j of kernel divided by its norm (the
 *       norm summed in double, one division, one rounding).  col_norm: double [c].  bad_cols: int32 [1] device, the number of columns
 *       whose norm is zero or not finite (upstream gives NaN logits for them; the caller refuses).  1 <= d <= 4096, 1 <= c <= 2^20.
 *   idb_head_workspace_bytes(b, d, c, row_tiles, col_blocks): the workspace of idb_head_loss / idb_head_logits, 0 for shapes they
 *       refuse; row_tiles / col_blocks (either may be NULL) receive the loss kernel's grid: tiles of 128 rows, and the blocks of
 *       columns whose partial log-sum-exp, maximum and argmax are merged in ascending order.
 *   idb_head_loss: replaces the header's forward, `criterion(thetas, labels)` and `multi_class_acc(thetas, labels)` without writing
 *       the b x c matrix.  Launches: (AdaFace: batch statistics,) per-row prep, loss tiles, merge, mean.
 *       Per row i: n_i = |emb_i| and x_i = emb_i / n_i (double, rounded once; AdaFace takes emb as it is, as upstream), the target
 *       cosine c_i = <emb_i, kernel[:, label_i]> / (n_i col_norm[label_i]) in double, and the target logit in double:
 *         CosFace  s (clamp(c, -1, 1) - m)                         ArcFace  s cos(acos(clamp(c, -1, 1)) + m)
 *         AdaFace  e = 1e-3, safe = clip(norms, 0.001, 100), mean / std = its batch mean / unbiased std, ada_state[0 / 1] <-
 *                  mean (std) t_alpha + (1 - t_alpha) ada_state[0 / 1] (updated in place on every call, as upstream),
 *                  scaler = clip((safe - ada_state[0]) / (ada_state[1] + e) h, -1, 1),
 *                  s (cos(clip(acos(clamp(c, -1 + e, 1 - e)) - m scaler, e, pi - e)) - (m + m scaler)).
 *       Every other logit is fp32 s * clamp(<x_i, wn_j>, -1, 1) (AdaFace: -1 + e, 1 - e, on every entry); column label_i is REPLACED
 *       by the fp32 rounding of the target logit.  rows: double [5][b]: log-sum-exp, loss_i = lse - target logit, target logit,
 *       target cosine (before the clamp), AdaFace's margin scaler (else 0).  pred: int32 [b], the argmax, the lowest column among
 *       equal logits (torch.argmax).  mean_loss: double [1], the rows' losses summed in a fixed order / b.  correct: int32 [1],
 *       #{pred == label}.  A label outside [0, c) reads nothing and gives that row NaN (callers refuse it: upstream's
 *       CrossEntropyLoss raises).  1 <= b <= 65536 (AdaFace: b >= 2), d and c as above; s in (0, 1e4]; t_alpha in [0, 1];
 *       wn == NULL (an unpacked header) is IDB_EINVAL.  ws 16-byte aligned.
 *   idb_head_logits: the `thetas` [b][c] fp32 the header returns upstream (API parity and per-element tests; not on the loss path):
 *       (statistics,) prep, one tile launch with a store epilogue.  rows as above; its first two planes are left untouched.
 * ------------------------------------------------------------------------------------------ */
#define IDB_HEAD_COSFACE 0
#define IDB_HEAD_ARCFACE 1
#define IDB_HEAD_ADAFACE 2
typedef struct idb_head_desc {
    int32_t kind;            /* IDB_HEAD_* */
    int32_t b, d, c;
    double s, m, h, t_alpha; /* h, t_alpha: AdaFace */
    const float* emb;        /* [b][d] */
    const float* norms;      /* [b], AdaFace (else NULL) */
    const int32_t* label;    /* [b] */
    const float* kernel;     /* [d][c], the header's parameter */
    const float* wn;         /* [c][d], idb_head_pack */
    const double* col_norm;  /* [c], idb_head_pack */
    double* ada_state;       /* [2] batch_mean, batch_std: read and updated (AdaFace, else NULL) */
} idb_head_desc;
int idb_head_pack(const float* kernel, int32_t d, int32_t c, float* wn, double* col_norm, int32_t* bad_cols, void* stream);
size_t idb_head_workspace_bytes(int32_t b, int32_t d, int32_t c, int32_t* row_tiles, int32_t* col_blocks);
int idb_head_loss(const idb_head_desc* h, double* rows, int32_t* pred, double* mean_loss, int32_t* correct, void* ws, size_t ws_bytes,
                  void* stream);
int idb_head_logits(const idb_head_desc* h, float* thetas, double* rows, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The loss head's backward and the header's optimiser step: what `accelerator.backward(loss_v)` (train_FR.py:290) leaves in
 * `header.kernel.grad` and hands back through the embeddings, then `clip_grad_norm_(header.parameters(), 5)` and `opt_header.step()`
 * (train_FR.py:293, :296; SGD with momentum 0.9 and weight decay 5e-4, :203-208).  The b x c matrix is never written, neither the
 * probabilities nor their gradient; no floating-point atomics, every sum in an order the shapes alone decide.
 *   With r_ij the raw cosine, (lo, hi) the forward's clamp, p_ij = exp(z_ij - lse_i) from the forward's log-sum-exp and
 *   G_ij = (p_ij - [j == label_i]) / b * s * d_ij * [lo <= r_ij <= hi] (inclusive, as torch's clamp backward), where d_ij = 1 off the
 *   target (the limit of sin(acos c) / sqrt(1 - c^2), which upstream evaluates to NaN at c = +-1 exactly) and the target's slope is
 *     CosFace 1      ArcFace sin(acos(c) + m) / sqrt(1 - c^2)
 *     AdaFace sin(t) / sqrt(1 - c^2) with t = acos(c) - m scaler if e <= t <= pi - e, else 0 (c after the clamp),
 *   d_emb_i = (dX_i - x_i <x_i, dX_i>) / |e_i| with dX = G Wn (AdaFace: dX_i, its rows are taken as they are and `norms` is detached),
 *   d_kernel[:, j] = (dW_j - w_j <w_j, dW_j>) / col_norm[j] with dW = G^T X; both projections and divisions in double, one rounding.
 *   idb_head_grad_workspace_bytes(b, d, c, row_tiles, class_blocks, d_chunks): the workspace of idb_head_loss_grad (the forward's
 *       included), 0 for shapes it refuses: those of idb_head_workspace_bytes, and class_blocks * b * d > 2^27 floats (512 MiB) of dX
 *       partials.  The three outputs (any may be NULL) receive the dX launch's grid: tiles of 128 rows, blocks of classes whose
 *       partial dX rows are merged in ascending order, and chunks of 128 columns of d (walked inside a
 *       workgroup after each cosine tile; with several row tiles the dW launch gives every chunk its own workgroups).
 *   idb_head_loss_grad: idb_head_loss (same launches, same values, AdaFace's buffers updated ONCE), then: per-row slopes, dX tiles,
 *       dX merge + projection, dW tiles + projection.  grad_rows: double [3][b]: the target's slope d_i with its clamp / clip mask
 *       folded in (not finite for an ArcFace target cosine of +-1 exactly: callers refuse), that mask, |e_i|.  d_emb: fp32 [b][d].
 *       d_kernel: fp32 [d][c], as torch stores kernel.grad.  Arguments as idb_head_loss; IDB_EUNSUPPORTED past the partials' limit.
 *   idb_head_sgd_step: the clipped SGD step all three entries share (its arithmetic: csrc/idb_sgd.h), here on the kernel alone:
 *       total_norm = |grad|_2 (double, fixed order; written to total_norm [1] on the device),
 *       coef = min(1, max_norm / (total_norm + 1e-6)), g = coef grad + weight_decay kernel, momentum_buf = g on the first step, else
 *       momentum momentum_buf + g, kernel -= lr momentum_buf (each element in double, each fp32 state rounded once), then
 *       idb_head_pack(kernel, ...) so that wn / col_norm / bad_cols follow the kernel.  kernel, grad, momentum_buf: fp32 [d][c].
 *       ws: IDB_HEAD_SGD_WS_BYTES, 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
#define IDB_HEAD_SGD_WS_BYTES 8192
size_t idb_head_grad_workspace_bytes(int32_t b, int32_t d, int32_t c, int32_t* row_tiles, int32_t* class_blocks, int32_t* d_chunks);
int idb_head_loss_grad(const idb_head_desc* h, double* rows, int32_t* pred, double* mean_loss, int32_t* correct, double* grad_rows,
                       float* d_emb, float* d_kernel, void* ws, size_t ws_bytes, void* stream);
int idb_head_sgd_step(float* kernel, const float* grad, float* momentum_buf, int32_t d, int32_t c, double lr, double momentum,
                      double weight_decay, double max_norm, int32_t first_step, float* wn, double* col_norm, int32_t* bad_cols,
                      double* total_norm, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The backbone's embedding stage in training (ID-Booth's FR_training/backbones/iresnet.py: bn2 -> flatten -> dropout -> fc ->
 * features, then train_FR.py's F.normalize), forward and backward, and the loop's joint clip_grad_norm_ + SGD step over a list of
 * tensors.  fp32 state and operands on the exact f32-input MFMA; every statistic and reduction in double in an order the shapes
 * alone decide; no floating-point atomics (bit-identical from run to run); no synchronisation; every argument is validated before
 * any HIP call.
 *   Layout: x is NHWC [b][hw][ch] in x_dtype; with K = hw ch and k = p ch + c, sample i's flattened row is x[i K + k].  fc_weight is
 *   fp32 [n][K] with that column order (upstream's is c hw + p), as are its gradient, the uint8 keep-mask [b][K] and d_x.
 *   2 <= b <= 1024 in training (1 <= b in eval), ch % 64 == 0 <= 2048, 1 <= hw <= 64, n % 64 == 0 <= 1024, 0 <= p < 1.
 *   idb_tail_workspace_bytes(b, ch, hw, n, k_slices, row_tiles): the workspace of forward and backward, 0 for refused shapes; the
 *       outputs (either may be NULL) receive the fc forward's split over K and the tiles of 128 rows.
 *   idb_tail_forward.  Training: per channel over the b hw rows mean and biased variance (shifted sums in double; the slices in
 *       ascending order), invstd = 1 / sqrt(var + eps2), running_mean / running_var <- (1 - momentum) old + momentum new (the unbiased
 *       variance, in double, rounded once); the fp32 affine sc = gamma invstd, sh = beta - mean sc (each rounded once);
 *       d = fma(x, sc, sh) * (keep ? 1 / (1 - p) : 0) formed in the product's load path and never written (keep == NULL: all kept);
 *       z = d W^T over K slices merged in ascending order in double, plus fc_bias, rounded once; features: the same statistics over
 *       the batch per feature with eps1; f = (z - mean) invstd feat_weight + feat_bias in double, rounded once;
 *       norm = |f| (double, of the rounded row); emb = f / max(norm, 1e-12).  Eval: both BatchNorms use their running statistics,
 *       which stay unchanged; keep must be NULL.
 *       Outputs: emb fp32 [b][n], norms double [b], bn2_stat double [2][ch] (mean, invstd), affine fp32 [2][ch] (sc, sh; 16-byte
 *       aligned), z fp32 [b][n], feat_stat double [2][n], f fp32 [b][n], flags int32 [4] (device): [0] a statistic or, in either mode, a row's norm is not finite
 *       (a NaN or infinity in x), [1] / [2] a bn2 / features variance of exactly 0 with eps = 0.  Callers refuse on any flag.
 *   idb_tail_backward (training descriptors only), given g_emb fp32 [b][n] and the forward's outputs:
 *       renormalised: g <- (g - y <y, g>) / |emb| with y = emb / |emb| (the loop's AdaFace branch); g_f = (g - u <u, g>) / norm with
 *       u = f / norm; S1 = sum_b g_f, S2 = sum_b g_f zhat; g_z = feat_weight invstd (g_f - S1 / b - zhat S2 / b), fp32;
 *       d_feat_bias = S1, d_fc_bias = sum_b g_z; g_y = (g_z W) (keep ? 1 / (1 - p) : 0), fp32 [b][K] in the workspace, with per
 *       (row tile, k) partial sums of g_y and g_y xhat merged over tiles then positions in ascending order: d_bn2_bias, d_bn2_weight;
 *       d_x = gamma invstd (g_y - mean(g_y) - xhat mean(g_y xhat)), fp32 [b][K] (NULL: that launch is skipped);
 *       d_fc_weight[j][k] = sum_b g_z[b][j] d[b][k] with d recomputed as in the forward, the batch ascending inside one workgroup.
 *   idb_sgd_clip_step: clip_grad_norm_(params, max_norm) and torch.optim.SGD(momentum, weight_decay).step() over 1..8 fp32
 *       tensors given as host arrays of device pointers: total_norm = the L2 norm over all gradients (double partials per tensor,
 *       tensor after tensor; written to total_norm [1] on the device), then idb_head_sgd_step's arithmetic per element without the
 *       repack.  ws: IDB_SGD_CLIP_WS_BYTES, 16-byte aligned; total_norm 8-byte aligned; no weight or momentum buffer may appear
 *       twice in the lists (IDB_EINVAL).
 * ------------------------------------------------------------------------------------------ */
typedef struct idb_tail_desc {
    int32_t b, ch, hw, n;
    int32_t x_dtype;          /* IDB_F16, IDB_BF16 or IDB_F32 */
    int32_t training;         /* 1: batch statistics, dropout, running statistics updated; 0: running statistics */
    double p;                 /* dropout probability */
    double eps2, eps1;        /* bn2's and features' eps */
    double momentum;          /* of both BatchNorms */
    const void* x;            /* [b][hw][ch] */
    const uint8_t* keep;      /* [b][hw ch], training only; NULL: nothing dropped */
    const float* bn2_weight;  /* [ch] */
    const float* bn2_bias;
    float* bn2_mean;          /* running statistics [ch]: read, and updated in training */
    float* bn2_var;
    const float* fc_weight;   /* [n][hw ch], column p ch + c */
    const float* fc_bias;     /* [n] */
    const float* feat_weight; /* [n], frozen upstream */
    const float* feat_bias;
    float* feat_mean;         /* running statistics [n] */
    float* feat_var;
} idb_tail_desc;
#define IDB_SGD_CLIP_WS_BYTES 65536
size_t idb_tail_workspace_bytes(int32_t b, int32_t ch, int32_t hw, int32_t n, int32_t* k_slices, int32_t* row_tiles);
int idb_tail_forward(const idb_tail_desc* d, float* emb, double* norms, double* bn2_stat, float* affine, float* z, double* feat_stat, float* f,
                     int32_t* flags, void* ws, size_t ws_bytes, void* stream);
int idb_tail_backward(const idb_tail_desc* d, const float* g_emb, const float* emb, const double* norms, const double* bn2_stat,
                      const float* affine, const float* z, const double* feat_stat, const float* f, int32_t renormalised, float* d_bn2_weight,
                      float* d_bn2_bias, float* d_fc_weight, float* d_fc_bias, float* d_feat_bias, float* d_x, void* ws, size_t ws_bytes,
                      void* stream);
int idb_sgd_clip_step(int32_t count, float* const* weights, const float* const* grads, float* const* momentum_bufs, const int64_t* numel,
                      double lr, double momentum, double weight_decay, double max_norm, int32_t first_step, double* total_norm, void* ws,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The backbone's convolutional trunk in training (iresnet.py's stem and IBasicBlock), as the pieces a block is composed of
 * (faceposegenerator_amd/frtrunk.py composes them), forward and backward, and the joint clipped SGD step over a table of tensors.
 * idb_tail's conventions: fp32 state, every product on the exact f32-input MFMA, statistics and cross-workgroup reductions in
 * double in an order the shapes alone decide, no floating-point atomics (bit-identical from run to run), no synchronisation,
 * every argument validated before any HIP call.
 *   Layout: activations and their gradients NHWC [b][h][w][c]; conv weights and their gradients [cout][ky][kx][cin].
 *   Bounds: cin == 4 or cin % 64 == 0, cout % 64 == 0, both <= 2048; 1 <= h, w <= 128; 1 <= b <= 1024; BatchNorm over
 *   rows = b h w >= 2 in training, ch % 64 == 0; ksize 3 (pad 1) or 1 (pad 0); stride 1 or 2; ho = (h + 2 pad - ksize) / stride + 1.
 *   idb_blk_bn_forward: BatchNorm2d over [rows][ch].  Training: shifted sums per (row slice, channel) in double (the shift is row 0),
 *       merged by one wave per channel (lane l adds slices l, l + 64, ... ascending, then an xor butterfly); mean, biased variance,
 *       invstd = 1 / sqrt(var + eps), running <- (1 - momentum) old + momentum new (the unbiased variance; in double, rounded once).
 *       Eval: the running statistics, unchanged.  Outputs: stat double [2][ch] (mean, invstd), affine fp32 [2][ch]
 *       (sc = gamma invstd, sh = beta - mean sc, each rounded once).  flags int32 [2] is only ever raised (the caller zeroes it):
 *       [0] a statistic is not finite, [1] var + eps == 0.  idb_blk_bn_workspace_bytes(rows, ch, slices): the workspace of
 *       idb_blk_bn_forward and idb_blk_bn_backward, 0 for refused shapes.
 *   idb_blk_conv_forward: out[b][oy][ox][co] = sum a[b][oy s + ky - pad][ox s + kx - pad][ci] w[co][ky][kx][ci] as an fma chain over
 *       k = (ky, kx, ci) ascending, with a = x, or fma(x, sc, sh) with `affine` (cin's pair), then a > 0 ? a : slope a with `slope`,
 *       formed in the operand load and never written; an out-of-image tap is an exact 0.
 *   idb_blk_conv_dgrad: g_in[b][y][x][ci] = sum g_out[b][(y + pad - ky) / s][(x + pad - kx) / s][co] w[co][ky][kx][ci] over the taps
 *       where the division is exact and in range: the gradient with respect to a (not x).  One grid slab per stride-parity class
 *       of input pixels, each reducing over the taps that reach it only.  cin % 64 == 0.
 *   idb_blk_conv_wgrad: d_weight[co][ky][kx][ci] = sum over b, oy, ox of g_out a, a recomputed as in the forward; the reduction in
 *       `wgrad_slices` slices (idb_blk_conv_workspace_bytes reports them, the dgrad's tiles of 128 rows, and the workspace), the
 *       slices merged in ascending order in double and rounded once.
 *   idb_blk_bn_backward: for y = fma(c, sc, sh) and p = slope ? prelu(y) : y with g the gradient of p: g_y = y > 0 ? g : slope g
 *       (y == 0 takes the slope), d_slope = sum g min(y, 0), d_beta = S1 = sum g_y, d_gamma = S2 = sum g_y xhat,
 *       g_c = gamma invstd (g_y - S1 / rows - xhat S2 / rows) (+ add, a second gradient of c's shape, NULL: none), in double,
 *       rounded once.  The sums per (row slice, channel) in double, merged as in idb_blk_bn_forward.
 *   idb_blk_affine: out = prelu(fma(c, sc, sh)) (slope NULL: no PReLU) + identity (NULL: none), or + fma(identity, scd, shd) with
 *       id_affine: the stem's activation and the block's residual in one elementwise launch.
 *   idb_blk_pack_images: float NCHW [b][3][h][w] -> NHWC [b][h][w][4], the fourth channel 0.
 *   idb_sgd_clip_step_table: idb_sgd_clip_step over 1..1024 tensors whose pointer and numel tables (count entries each) lie in
 *       DEVICE memory; the same kernels on the same geometry, bit-identical to idb_sgd_clip_step for up to 8 tensors (csrc/idb_sgd.hip).  The tables'
 *       contents cannot be validated on the host: the caller guarantees 1 <= numel <= 2^32 and distinct buffers.
 *       ws: idb_sgd_clip_table_workspace_bytes(count), 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
typedef struct idb_blk_conv_desc {
    int32_t b, h, w, cin, cout, ksize, stride;
    const float* x;           /* [b][h][w][cin] */
    const float* affine;      /* [2][cin] sc, sh applied while loading; NULL: x as it is */
    const float* slope;       /* [cin] PReLU after the affine; NULL: none */
    const float* weight;      /* [cout][ksize][ksize][cin] */
} idb_blk_conv_desc;
size_t idb_blk_conv_workspace_bytes(int32_t b, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ksize, int32_t stride,
                                    int32_t* wgrad_slices, int32_t* dgrad_row_tiles);
int idb_blk_conv_forward(const idb_blk_conv_desc* d, float* out, void* stream);
int idb_blk_conv_dgrad(const idb_blk_conv_desc* d, const float* g_out, float* g_in, void* stream);
int idb_blk_conv_wgrad(const idb_blk_conv_desc* d, const float* g_out, float* d_weight, void* ws, size_t ws_bytes, void* stream);
size_t idb_blk_bn_workspace_bytes(int64_t rows, int32_t ch, int32_t* slices);
int idb_blk_bn_forward(const float* x, int64_t rows, int32_t ch, int32_t training, double eps, double momentum, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, double* stat, float* affine, int32_t* flags, void* ws,
                       size_t ws_bytes, void* stream);
int idb_blk_bn_backward(const float* c, const float* g, int64_t rows, int32_t ch, const double* stat, const float* affine, const float* gamma,
                        const float* slope, const float* add, float* d_gamma, float* d_beta, float* d_slope, float* g_c, void* ws,
                        size_t ws_bytes, void* stream);
int idb_blk_affine(const float* c, const float* affine, const float* slope, const float* identity, const float* id_affine, int64_t rows,
                   int32_t ch, float* out, void* stream);
int idb_blk_pack_images(const float* images, int32_t b, int32_t h, int32_t w, float* out, void* stream);
size_t idb_sgd_clip_table_workspace_bytes(int32_t count);
int idb_sgd_clip_step_table(int32_t count, float* const* weights, const float* const* grads, float* const* momentum_bufs, const int64_t* numel,
                            double lr, double momentum, double weight_decay, double max_norm, int32_t first_step, double* total_norm,
                            void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA fine-tuning of one attention module (train_ID-Booth.py: rank-4 adapters on to_q / to_k / to_v / to_out.0): the attention that
 * saves its row statistic, its backward, and the adapter gradients.  Layouts as idb_attention: q, out, dout, dq [batch][n_q][heads*64]
 * with a row stride each; k, v, dk, dv [batch][n_kv_alloc][...] with one row stride per pair, only the first n_kv rows attended; the
 * packed [q|k|v] buffer (stride 3 * heads * 64) serves for the inputs and, another one, for the gradients.  f16 / bf16 operands, fp32
 * accumulation; no atomics and no inter-workgroup waiting anywhere: every result is bit-identical from run to run.
 *   idb_attention_fwd_train: idb_attention without the causal mask, plus lse[batch][heads][n_q] (fp32) = ln sum_j exp(scale q.k_j).
 *   idb_attention_bwd: with delta_i = sum_d dout out (fp32), P = exp(scale Q K^T - lse), dP = dout V^T, dS = P o (dP - delta):
 *       dV = P^T dout, dQ = scale dS K, dK = scale dS^T Q; P and dS are rounded to the operand dtype for these products, each gradient
 *       is summed in fp32 and rounded once.  Rows n_kv .. n_kv_alloc - 1 of k and v are never read and those of dk and dv never
 *       written.  dQ comes from a kernel that owns query blocks of 128 rows and recomputes S (no sum across workgroups exists); dK and
 *       dV from one that owns key blocks of IDB_ATTN_BWD_KEY_BLOCK keys and sweeps the queries in slices of IDB_ATTN_BWD_SLICE rows:
 *       form 0 sweeps all of them; form 1 (fewer than IDB_ATTN_BWD_FULL_GRID key-block workgroups and more than two slices) cuts the
 *       query range into chunks of `query_rows` rows, whose fp32 slabs in the workspace a plain pass sums in ascending order.
 *       launches: 3 (form 0) or 4.  A gradient may not share a byte with an input or the workspace.
 *   idb_lora_grad: x [m][in] and dy [m][out] in the operand dtype (row strides x_ld, dy_ld: dy may be a column slice of the packed
 *       gradient buffer), lora_a [rank][in] and lora_b [out][rank] fp32 (peft's layouts); db[out][rank] = scale dy^T (x A^T) and
 *       da[rank][in] = scale (dy B)^T x in fp32.  The out x in weight gradient is never formed.  The sum over m runs in fp32 within
 *       chunks of IDB_LORA_GRAD_CHUNK_ROWS rows (more once m exceeds that times IDB_LORA_GRAD_MAX_CHUNKS), the chunks merged in
 *       ascending order in double and rounded once.  rank 1..IDB_LORA_MAX_RANK; in and out multiples of 64.
 * Refusals (IDB_EINVAL, a dtype other than f16 / bf16: IDB_EUNSUPPORTED) name the argument and come before any launch.
 * ------------------------------------------------------------------------------------------ */
#define IDB_ATTN_BWD_KEY_BLOCK 128
#define IDB_ATTN_BWD_SLICE 32
#define IDB_ATTN_BWD_FULL_GRID 128
#define IDB_LORA_MAX_RANK 16
#define IDB_LORA_GRAD_CHUNK_ROWS 32
#define IDB_LORA_GRAD_MAX_CHUNKS 256
int idb_attention_fwd_train(const void* q, int32_t q_ld, const void* k, const void* v, int32_t kv_ld, void* out, int32_t out_ld, float* lse,
                            int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t n_kv_alloc, float scale, int32_t dtype,
                            void* stream);
size_t idb_attention_bwd_workspace_bytes(int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv);
int idb_attention_bwd_plan(int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t* form, int32_t* key_block, int32_t* query_rows,
                           int32_t* launches);
int idb_attention_bwd(const void* q, int32_t q_ld, const void* k, const void* v, int32_t kv_ld, const void* out, int32_t out_ld,
                      const void* dout, int32_t dout_ld, const float* lse, void* dq, int32_t dq_ld, void* dk, void* dv, int32_t dkv_ld,
                      void* workspace, size_t workspace_bytes, int32_t batch, int32_t heads, int32_t n_q, int32_t n_kv, int32_t n_kv_alloc,
                      float scale, int32_t dtype, void* stream);
size_t idb_lora_grad_workspace_bytes(int64_t m, int32_t in, int32_t out, int32_t rank);
int idb_lora_grad(const void* x, int32_t x_ld, const void* dy, int32_t dy_ld, const float* lora_a, const float* lora_b, float* da, float* db,
                  int64_t m, int32_t in, int32_t out, int32_t rank, float scale, void* workspace, size_t workspace_bytes, int32_t dtype,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA fine-tuning of one transformer block (diffusers' BasicTransformerBlock, SD-2.1's form): what the block's backward needs
 * besides the attention modules above, and the optimiser step of the adapters.  f16 / bf16 operands, fp32 arithmetic, every result
 * rounded once; no atomics and no inter-workgroup waiting: bit-identical from run to run (csrc/idb_tblock.hip, csrc/idb_adamw.hip).
 *   idb_layernorm_bwd: the input gradient of idb_layernorm.  x [rows][c] is the forward's raw input; mean, rstd and xhat are
 *       recomputed with the forward's own arithmetic (no statistic is saved).  With g = dy gamma:
 *       dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ add), rounded once.  add: an operand-dtype tensor of dx's shape (the residual
 *       stream's gradient) or NULL.  dx may be add or dy themselves (a wave owns whole rows and reads them before it stores), nothing
 *       else.  c a multiple of 8, at most 1536, as idb_layernorm.  d_gamma and d_beta are NOT computed: LayerNorm's affine is frozen
 *       in this fine-tuning (peft marks only the adapters trainable).
 *   idb_geglu_fwd: hg [rows][2 inner] (row stride hg_ld), value then gate, diffusers' order (hidden, gate = proj(x).chunk(2, -1));
 *       out[rows][inner] = value gelu(gate), the exact-GELU approximation of idb_gemm's GEGLU epilogue.
 *   idb_geglu_bwd: dhg[rows][2 inner] dense: dvalue = dout gelu(gate), dgate = dout value (Phi(gate) + gate phi(gate)), Phi the
 *       same approximation, phi sharing its exponential.  inner a multiple of 8; rows * inner / 8 below 2^31.
 *   idb_adamw_clip_step_table: GradScaler.unscale_ + clip_grad_norm_(params, max_norm) + torch.optim.AdamW(non-amsgrad).step() over
 *       1..1024 fp32 tensors whose pointer and numel tables (count entries each) lie in DEVICE memory, as idb_sgd_clip_step_table's
 *       (the same norm arithmetic and geometry).  total_norm = inv_scale ||g|| in double.  Per element, in double from the fp32
 *       states, each fp32 state rounded once: g^ = coef inv_scale g, coef = min(1, max_norm / (total_norm + 1e-6));
 *       w <- w (1 - lr weight_decay); m <- beta1 m + (1 - beta1) g^; v <- beta2 v + (1 - beta2) g^2;
 *       w <- w - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  step >= 1 is the number of this step; the two
 *       bias corrections are computed on the host in double.  If total_norm is not finite nothing is written to w, m, v and
 *       *skipped = 1 (GradScaler.step's skip), otherwise 0; the scale's growth and backoff stay the caller's.  total_norm (double)
 *       and skipped (int32) are device memory.  ws: idb_adamw_clip_table_workspace_bytes(count), 16-byte aligned.  The tables'
 *       contents cannot be validated on the host: the caller guarantees 1 <= numel <= 2^32 and distinct buffers.  Three launches.
 * Refusals (IDB_EINVAL, a dtype other than f16 / bf16: IDB_EUNSUPPORTED) name the argument and come before any launch.
 * ------------------------------------------------------------------------------------------ */
int idb_layernorm_bwd(const void* x, const void* dy, const void* add, const float* gamma, void* dx, int64_t rows, int32_t c, float eps,
                      int32_t dtype, void* stream);
int idb_geglu_fwd(const void* hg, int32_t hg_ld, void* out, int64_t rows, int32_t inner, int32_t dtype, void* stream);
int idb_geglu_bwd(const void* hg, int32_t hg_ld, const void* dout, void* dhg, int64_t rows, int32_t inner, int32_t dtype, void* stream);
size_t idb_adamw_clip_table_workspace_bytes(int32_t count);
int idb_adamw_clip_step_table(int32_t count, float* const* weights, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              const int64_t* numel, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                              double inv_scale, int64_t step, double* total_norm, int32_t* skipped, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA fine-tuning across UNet stages: the input gradient of idb_groupnorm (diffusers' ResnetBlock2D.norm1 / norm2 with the SiLU that
 * follows them, Transformer2DModel.norm without), csrc/idb_gnbwd.hip.  The convolutions' and Linears' input gradients are idb_gemm
 * with flipped / transposed weights (faceposegenerator_amd/lorastage.py) and need no entry of their own.
 *   x0 [batch][hw][c0], x1 [batch][hw][c1] or NULL (c1 == 0): the forward's RAW input(s), the channel concatenation x0 | x1.
 *   stat_partials [batch][stat_chunks][groups][2] fp32: what idb_groupnorm_stats wrote for x0 | x1 (1 <= stat_chunks <= 64).
 *   dy [batch][hw][c0 + c1] dense: the gradient w.r.t. the forward's output (after the SiLU when silu = 1).
 *   add [batch][hw][c0 + c1] dense or NULL: added to dx (a residual's or shortcut's gradient, at no launch of its own).
 *   dx0 [batch][hw][c0], dx1 [batch][hw][c1] (NULL exactly when c1 == 0).
 * Per (sample, group), n = hw * channels per group: mean and rstd are formed from stat_partials with idb_groupnorm's own expressions
 * (chunks summed in a fixed order in fp32, then in double mean = a / n, var = max(0, q / n - mean^2), rstd = 1 / sqrt(var + eps)).
 * Per element xhat = (x - mean) rstd, y = xhat gamma + beta, d = dy (silu = 0) or dy s (1 + y (1 - s)) with s = 1 / (1 + exp(-y))
 * (silu = 1; one v_exp_f32 and one v_rcp_f32), g = d gamma; m1 = sum g / n, m2 = sum g xhat / n;
 * dx = rstd (g - m1 - xhat m2) (+ add), rounded once.  fp32 arithmetic; the two sums are fp32 per (sample, pixel chunk, group) in
 * fixed-order trees and merged over the chunks in double in a fixed order.  Two launches (sums into the workspace, then dx), no
 * atomics, no workgroup waits for another: bit-identical from run to run.  d_gamma and d_beta are NOT computed: GroupNorm's affine is
 * frozen in this fine-tuning (peft marks only the adapters trainable).
 * When c1 == 0, dx0 may be dy or add themselves (pass 1 has finished before pass 2 stores, and a thread of pass 2 has read the
 * elements it writes); nothing else may overlap an output.  workspace: idb_groupnorm_bwd_workspace_bytes, 16-byte aligned.
 * Limits are idb_groupnorm's: c0, c1 multiples of 8, groups dividing c0 + c1 with at least 2 channels per group, a slice of
 * lcm(channels per group, 8) channels (doubled up to 8 vector columns) of at most 256 columns and 64 groups; eps > 0.
 * Refusals (IDB_EINVAL; a dtype other than f16 / bf16: IDB_EUNSUPPORTED) name the argument and come before any HIP call.
 * idb_groupnorm_bwd_plan is host-only: the same validation of the dims and what would be launched: slice_channels x slices = c0 + c1,
 * chunks x chunk_len >= hw the pixel chunks of pass 1 (grid chunks x slices x batch), apply_blocks the pixel blocks of pass 2.
 * ------------------------------------------------------------------------------------------ */
size_t idb_groupnorm_bwd_workspace_bytes(int32_t batch, int32_t hw, int32_t groups);
int idb_groupnorm_bwd_plan(int32_t c0, int32_t c1, int32_t batch, int32_t hw, int32_t groups, int32_t* slice_channels, int32_t* slices,
                           int32_t* chunks, int32_t* chunk_len, int32_t* apply_blocks);
int idb_groupnorm_bwd(const void* x0, int32_t c0, const void* x1, int32_t c1, const float* stat_partials, int32_t stat_chunks, const void* dy,
                      const void* add, const float* gamma, const float* beta, float eps, int32_t silu, void* dx0, void* dx1, int32_t batch,
                      int32_t hw, int32_t groups, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
