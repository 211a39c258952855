/* gmk.h — C ABI of libgmk.so: MI355X (gfx950) kernels for the DDPM train + sample hot path.
 *
 * The reference (matwilso/generative_models) has no FFI: every arithmetic op of its diffusion path is a
 * stock torch op.  Each entry point below names the reference call site(s) it replaces (paths relative to
 * the reference checkout).  Conventions:
 *   - returns 0 on success, GMK_ERR_ARG (<0) for an argument error, or a positive hipError_t;
 *     gmk_last_error() returns a per-thread message.  No exceptions, no allocation, no synchronisation.
 *   - every pointer is a BORROWED device pointer (e.g. torch `tensor.data_ptr()`), contiguous, 16-byte aligned;
 *     workspaces are passed in by the caller; all work is enqueued on `stream` (a hipStream_t).
 *   - re-entrant: callable from any host thread (autograd's backward thread, one process per GPU).
 *   - activations inside the network are NHWC `[B][H][W][C]` in `dtype` (GMK_F32, GMK_BF16 or GMK_F16), C a
 *     multiple of 128; a kernel that reads forward activations next to gradients takes the two types separately (`x_dtype`); parameters, statistics, embeddings and everything in the diffusion algebra are fp32;
 *     images at the model boundary are NCHW fp32 exactly as the reference passes them.
 */
#ifndef GMK_H
#define GMK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMK_F32 0
#define GMK_BF16 1
#define GMK_F16 2   /* fp16 storage: forward activations and forward weight packs of the 16-bit mode (gradients stay GMK_BF16); the
                     * reference's GPU path computes its forward under fp16 autocast (diffusion_model.py:68) */
#define GMK_ERR_ARG (-1)

/* gather modes of the implicit-GEMM convolution (how an output pixel + filter tap maps to a source pixel) */
#define GMK_CONV_NORMAL 0      /* stride 1                      simple_unet.py:163,172,117 */
#define GMK_CONV_STRIDE2 1     /* stride 2 (Downsample)         simple_unet.py:81,97,100   */
#define GMK_CONV_UPSAMPLE2 2   /* nearest x2 folded into a stride-1 conv   simple_unet.py:120-121 */
#define GMK_CONV_TRANSPOSED2 3 /* data-gradient of GMK_CONV_STRIDE2 (a transposed convolution) */

int gmk_version(void);
const char* gmk_last_error(void);
/* The kernel table: X(symbol, id, profile name) for every kernel a launcher reports.  This list is the only place where an id or a profile
 * name is written: the launchers pass GMK_K_<symbol>, the name lookup below is generated from it, and the Python binding parses it (K.<symbol>,
 * kernel_name).  A name is the device function's; a bracketed suffix tells apart launches of one function that the profile keeps on lines of
 * their own.  The stem / head kernels start at 31. */
#define GMK_KERNEL_TABLE(X)                                                                                                               \
    X(CONV_IGEMM, 1, "conv_igemm_kernel")                                                                                                 \
    X(CONV_IGEMM_DMA, 2, "conv_igemm_dma_kernel")                                                                                         \
    X(CONV_HALO, 3, "conv3x3_halo_kernel")                                                                                                \
    X(CONV_HALO_WS, 4, "conv3x3_halo_ws_kernel")                                                                                          \
    /* a halo kernel on the zero-stuffed source of GMK_CONV_TRANSPOSED2: 4x the algorithmic MFMA work by construction */                  \
    X(CONV_HALO_STUFFED, 5, "conv3x3_halo_ws_kernel[zero-stuffed transposed conv]")                                                       \
    /* GMK_CONV_TRANSPOSED2 where the halo family declines: four output-parity phase launches of the LDS-DMA kernel */                    \
    X(CONV_DMA_PHASES, 6, "conv_igemm_dma_kernel[stride-2 dgrad phases]")                                                                 \
    /* gmk_conv3x3_skipfold: conv2 of an up-path ResBlock with its 1x1 skip convolution folded in (K = 9 x 128 + 256) */                  \
    X(CONV_HALO_SKIPFOLD, 7, "conv3x3_halo_ws_kernel[+1x1 skip]")                                                                         \
    X(CONV_SUBPIXEL_UPSAMPLE, 8, "conv_subpixel_ws_kernel[upsample]")                                                                     \
    X(CONV_SUBPIXEL_TRANSPOSED, 9, "conv_subpixel_ws_kernel[transposed]")                                                                 \
    X(CONV_SUBPIXEL_UPSAMPLE_DGRAD, 10, "conv_subpixel_ws_kernel[upsample dgrad]")                                                        \
    X(CONV_WGRAD, 11, "conv_wgrad_kernel")                                                                                                \
    X(CONV_WGRAD_SLOTS, 12, "conv_wgrad_slots_kernel")                                                                                    \
    X(CONV_WGRAD_SLOTS_WS, 13, "conv_wgrad_slots_ws_kernel")                                                                              \
    X(CONV1X1_PAIR_STREAM, 14, "conv1x1_pair_stream_kernel")                                                                              \
    X(CONV1X1_WGRAD_STREAM, 15, "conv1x1_wgrad_stream_kernel")                                                                            \
    X(CONV_WGRAD_SUBPIXEL, 16, "conv_wgrad_subpixel_ws_kernel")                                                                           \
    /* the slot kernel on the four parity planes of a stride-2 convolution's input (4 - 16 MFMAs per step, not 36) */                    \
    X(CONV_WGRAD_SLOTS_S2, 17, "conv_wgrad_slots_ws_kernel[stride-2 planes]")                                                             \
    X(GN_FWD_REG, 21, "gn_silu_fwd_reg_kernel")                                                                                           \
    X(GN_FWD, 22, "gn_silu_fwd_kernel")                                                                                                   \
    X(GN_BWD_HYBRID, 23, "gn_silu_bwd_hybrid_kernel")                                                                                     \
    X(GN_BWD, 24, "gn_silu_bwd_kernel")                                                                                                   \
    X(GN_BWD_PAIR, 25, "gn_silu_bwd_pair_kernel")                                                                                         \
    X(GN_FWD_PAIR, 26, "gn_silu_fwd_pair_kernel")                                                                                         \
    X(EXPAND, 31, "expand3x3_kernel")                                                                                                     \
    X(EXPAND_MFMA, 32, "expand3x3_mfma_kernel")                                                                                           \
    X(EXPAND_TILE16, 33, "expand3x3_tile16_kernel")                                                                                       \
    X(WGRAD3, 34, "wgrad3x3_kernel")                                                                                                      \
    X(WGRAD3_MFMA, 35, "wgrad3x3_mfma_kernel")                                                                                            \
    X(WGRAD3_TILE16, 36, "wgrad3x3_tile16_kernel")                                                                                        \
    X(HEAD_FWD, 37, "head_fwd_kernel")                                                                                                    \
    X(HEAD_FWD_MFMA, 38, "head_fwd_mfma_kernel")                                                                                          \
    X(STEM_DGRAD, 39, "stem_dgrad_kernel")                                                                                                \
    X(STEM_DGRAD_MFMA, 40, "stem_dgrad_mfma_kernel")
enum {
#define GMK_K_ENUM(symbol, id, name) GMK_K_##symbol = id,
    GMK_KERNEL_TABLE(GMK_K_ENUM)
#undef GMK_K_ENUM
};
/* profiling aid: the table id of the kernel that the calling thread's last convolution, weight-gradient, GroupNorm or stem / head call
 * launched (per thread and sticky: a call that launches nothing leaves it); its profile name, NULL for 0 or an id outside the table */
int gmk_last_kernel(void);
const char* gmk_kernel_name(int id);
/* development aid: force kernel variants (0 = automatic; see GMK_CONV_KERNEL / GMK_WGRAD_KERNEL / GMK_GN_KERNEL); -1 = unset */
int gmk_set_kernel_choice(int conv, int wgrad, int gn);
/* development aid: a free integer (GMK_DEV_VARIANT) that experimental code paths may read for in-process A/B runs
 * (tools/small_batch_probe.py, tools/step_stamps.py); 0 / unset = the shipped behaviour */
int gmk_set_dev_variant(int v);
/* development aid (tools/step_stamps.py): while a device buffer of at least 512 bytes per workgroup is set, the wave-specialised 3x3 halo
 * launches (gmk_conv_igemm's 16-bit stride-1 3x3 path, gmk_conv3x3_skipfold) run an instrumented instantiation whose wave 4 (producer) and
 * wave 0 (consumer) write per-K-step shader-cycle sums [workgroup][2][64] into it; buf = NULL returns to the shipped kernels */
int gmk_dev_set_stamp_buffer(void* buf, int64_t bytes);
/* number of CUs the persistent convolution kernels may occupy (8..256, default 256 = the whole chip).  New with the build (the
 * reference has no multi-GPU path): data-parallel runs leave a few CUs to RCCL's all-reduce kernels, which otherwise queue
 * behind a chip-filling persistent grid */
int gmk_set_cu_limit(int n);
int gmk_get_cu_limit(void);
/* fp32 mode (dtype GMK_F32: the reference's own precision, gms/main.py:161-168 runs the test loss in fp32).  Default: exact fp32 MFMA chains
 * (v_mfma_f32_32x32x2_f32) - the parity mode, 1e-3 on every reference vector including the ill-conditioned closed-form set.  Round 6 adds a
 * fast form, gmk_set_fp32_exact(0) / GMK_FP32_SPLIT=1: the convolutions and weight gradients split each fp32 operand into bf16 hi + lo and form
 * a product as hi hi + hi lo + lo hi on the bf16 matrix cores with fp32 accumulation (~ 1e-5 per product, a fifth of the exact chains' matrix
 * time; the fp32 weight packs are then stored split, so re-pack after switching).  gmk_fp32_split() says which is active. */
int gmk_set_fp32_exact(int exact);
int gmk_fp32_split(void);
/* number of bytes of scratch gmk_conv_wgrad needs for the given problem (split-K slabs) */
int64_t gmk_conv_wgrad_workspace_bytes(int64_t n_pixels, int taps, int cout, int ktot);

/* ---- parameter packing -------------------------------------------------------------------------------
 * nn.Conv2d weight `[Cout][Cin][k][k]` fp32 (simple_unet.py:81,117,163,172,177) ->
 *   w_fwd   `[tap][Cout][Cin]`  dtype  (K-contiguous rows for the forward implicit GEMM)
 *   w_dgrad `[tap'][Cin][Cout]` dtype, tap' = spatially flipped tap (rows for the data-gradient GEMM)
 * either output may be NULL. */
int gmk_pack_conv_weight(const float* w, void* w_fwd, void* w_dgrad, int cout, int cin, int ksize, int dtype,
                         void* stream);
/* the same for up to 40 convolutions in ONE launch (the re-pack after every optimiser step): tensor e is the fp32
 * weight at arena + w_off[e] (elements) and is written as [w_fwd | w_dgrad], n = cout*cin*ksize^2 elements each, at
 * packs + pack_off[e] (elements of `dtype`).  fwd_f16 (optional; with dtype GMK_BF16 only): entries with a non-zero flag get their
 * w_fwd half in fp16 (same 2-byte slots), the operand type of the 16-bit mode's forward.  The six tables are HOST arrays of `count` ints. */
int gmk_pack_conv_weights_multi(const float* arena, void* packs, int count, const int* w_off, const int* pack_off,
                                const int* cout, const int* cin, const int* ksize, const int* fwd_f16, int dtype, void* stream);

/* ---- GroupNorm + SiLU (simple_unet.py:39-40,161-162,169-170; always adjacent in the reference) ---------
 * x,y: NHWC [B][HW][C]; `groups` groups over these C channels (a 2C-channel concatenated input is handled as
 * two calls of 16 groups each, simple_unet.py:150,161); mean/rstd: fp32 [B][groups] (written).
 * groups < 0: -groups channels per group (1..16, any size: nn.GroupNorm(32, 96) has 3), ceil(C / -groups) groups whose last one may be
 * partial - for zero-padded widths, where it lies in the padding; mean/rstd then have ceil(C / -groups) columns.  Same convention in
 * gmk_gn_silu_bwd.
 * Precision of the statistics: ONE pass of fp32 sums over the group's n = HW * C / groups values (sum and sum of squares, biased
 * var = E[x^2] - mean^2 clamped at 0, rstd = 1 / sqrt(var + eps)), for every storage type.  With m and sigma the group's exact mean and
 * standard deviation the results lie within
 *     |rstd - exact| / exact <= 4 * 2^-24 * log2(n) * (1 + m^2 / sigma^2)        |mean - exact| <= 4 * 2^-24 * log2(n) * sqrt(m^2 + sigma^2)
 * (measured: a tenth to a fifth of that).  The subtraction E[x^2] - mean^2 is where the m^2 / sigma^2 comes from: centred activations
 * give rstd to 1e-7, a group whose mean lies 8 sigma from zero to 1e-5 against a bound of 1.7e-4 - the size of fp16's rounding.
 * tests/test_gpu_gn_conformance.py holds every kernel form to this bound. */
int gmk_gn_silu_fwd(const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd,
                    int B, int HW, int C, int groups, float eps, const float* stats_part, int tile_pixels, int ntiles,
                    float drop_p, uint64_t drop_seed, uint64_t drop_offset, const float* xadd, int xadd_stride, int dtype,
                    void* stream);
/* xadd (optional, fp32 [B][xadd_stride]): x enters as x[b][p][c] + xadd[b][c] — the producing convolution's bias and the
 * embedding broadcast-add of simple_unet.py:183 (`h + emb_out[..., None, None]`) are applied here, in the HBM-bound kernel,
 * instead of in the MFMA kernel's epilogue; pass the same pointer to gmk_gn_silu_bwd.
 * stats_part (optional): partial sums emitted by the producing convolution (see gmk_conv_igemm gn_stats); when given,
 * the statistics pass over x is skipped (x is read once).
 * drop_p > 0: nn.Dropout(p) behind the SiLU (simple_unet.py:171, training mode): element e of y (NHWC order) is kept and
 * scaled by 1/(1-p) iff gmk_rng_uniform(seed = drop_seed, offset = drop_offset)[e] >= drop_p, else zeroed; pass the same
 * triple to gmk_gn_silu_bwd. */
/* backward of the above.  dx = d/dx + dadd1 + dadd2 (optional NHWC addends, e.g. the identity-skip gradient).
 * dgamma_part/dbeta_part: fp32 [B][C] per-sample partials (reduce with gmk_colsum); dxsum: optional fp32
 * [B][dxsum_stride] per-sample channel sums of the final dx (bias / embedding gradients).
 * dtype: type of dy / dadd1 / dadd2 / dx; x_dtype: type of the saved input x (the same, or GMK_F16 next to GMK_BF16 gradients). */
int gmk_gn_silu_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                    const float* rstd, const void* dadd1, const void* dadd2, void* dx, float* dgamma_part,
                    float* dbeta_part, float* dxsum, int dxsum_stride, int B, int HW, int C, int groups,
                    float drop_p, uint64_t drop_seed, uint64_t drop_offset, const float* xadd, int xadd_stride, int dtype,
                    int x_dtype, void* stream);
/* Paired backward: ONE tensor x with TWO GroupNorm + SiLU consumers (a down-path tensor of the U-Net: the down ResBlock's GroupNorm(32, C) and the
 * skip half of an up ResBlock's GroupNorm(32, 2C), other gamma / beta / groups).  x is read once; every output is bit-identical to the two
 * gmk_gn_silu_bwd calls it replaces.  gmk_gn_pair_ok: 1 if the paired kernel takes the shape (HW = 32 x 32 or 16 x 16, C a multiple of 32,
 * groups of 4 / 8 / 16 channels, 16-bit x, bf16 gradients), else 0 - the caller then makes the two calls. */
int gmk_gn_pair_ok(int HW, int C, int groups_a, int groups_b, int x_dtype, int grad_dtype);
/* Paired forward of the same two consumers: x read once, (y, mean, rstd) of each bit-identical to its own gmk_gn_silu_fwd call (no dropout, no
 * producer statistics).  gmk_gn_pair_fwd_ok: 1 where it runs (HW = 16 x 16, C a multiple of 64, groups of 4 / 8 / 16 channels, 16-bit x). */
int gmk_gn_pair_fwd_ok(int HW, int C, int groups_a, int groups_b, int dtype);
int gmk_gn_silu_fwd_pair(const void* x, void* y_a, void* y_b, const float* gamma_a, const float* beta_a, const float* gamma_b,
                         const float* beta_b, float* mean_a, float* rstd_a, float* mean_b, float* rstd_b, int B, int HW, int C,
                         int groups_a, int groups_b, float eps, const float* xadd, int xadd_stride, int dtype, void* stream);
/* dx = GNbwd_dn(dy_dn) + dadd_dn + bf16(GNbwd_up(dy_up) + dadd_up): the up consumer's input gradient (the tensor the two-call form hands over
 * through HBM as the second call's dadd2) stays in registers, rounded to bf16 where the stored one is.  Both addends are required.
 * dgamma / dbeta partials of both consumers are written; dxsum (optional): per-sample channel sums of dx.  Gradients are bf16. */
int gmk_gn_silu_bwd_pair(const void* x, const void* dy_up, const void* dadd_up, const float* gamma_up, const float* beta_up,
                         const float* mean_up, const float* rstd_up, float* dgamma_part_up, float* dbeta_part_up, int groups_up,
                         const void* dy_dn, const void* dadd_dn, const float* gamma_dn, const float* beta_dn, const float* mean_dn,
                         const float* rstd_dn, float* dgamma_part_dn, float* dbeta_part_dn, int groups_dn, void* dx, float* dxsum,
                         int dxsum_stride, int B, int HW, int C, const float* xadd, int xadd_stride, int x_dtype, void* stream);
/* dst[i] = (dst type) src[i], n a multiple of 8: fp16 <-> bf16 storage conversion (fp16 results saturate at the largest finite value).
 * No reference call site: the self-attention extension (north_star, BASELINE configs[4]) keeps bf16 internals and converts the fp16
 * forward stream at its boundary. */
int gmk_cast16(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);
/* out[b][c] = sum over pixels of x[b][:, c]  (NHWC, fp32 result [B][out_stride]) */
int gmk_chansum(const void* x, float* out, int out_stride, int B, int HW, int C, int dtype, void* stream);
/* out[c] (+)= sum_r part[r*stride + c], r < R, c < C  (fp32) */
int gmk_colsum(const float* part, int64_t stride, float* out, int R, int C, int accumulate, void* stream);
/* up to 16 independent gmk_colsum problems in one launch (host arrays of length n) */
int gmk_colsum_multi(int n, const float* const* part, const int64_t* stride, float* const* out, const int* R,
                     const int* C, void* stream);
/* 2x2 sum-pool NHWC [B][2H][2W][C] -> [B][H][W][C]: backward of F.interpolate(nearest, x2), simple_unet.py:120 */
int gmk_sumpool2x2(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);

/* ---- 3x3 / 1x1 convolution, C_out = 128-wide tiles, MFMA implicit GEMM ---------------------------------
 * out[b][oy][ox][n] = bias[n] + emb[b*emb_stride + n] + residual[b][oy][ox][n]
 *                     + sum_{tap,k} srcK[b][sy][sx][k] * w[tap][n][k]
 * src0/src1: NHWC sources of c0 / c1 channels (c1 = 0: one source) — the channel concatenation
 * torch.cat([x, skip], 1) (simple_unet.py:150) is never materialised.  (hs, ws): source spatial size;
 * (ho, wo): output spatial size; `mode` one of GMK_CONV_*.  w: packed rows `[tap][w_rows][c0+c1]` of
 * `dtype`; output channels n0 .. n0+cout-1 use rows n0.. of each tap (cout % 128 == 0).  bias/emb/residual
 * may be NULL.  Forward convolutions pass a w_fwd pack; data gradients pass a w_dgrad pack.
 * gn_stats (optional, may be NULL): the convolution that PRODUCES a GroupNorm input can emit that GroupNorm's
 * statistics from its epilogue, saving the consumer one full read of the tensor.  Only conv3x3_halo_kernel
 * (gmk_last_kernel() == 3) fills it: fp32 [ntiles][8][2][cout/4][2] = for every 32-pixel group of every tile
 * (tile = 256/wo whole rows of the global row list b*ho + y) and each of the <= 2 samples the group touches, the sum
 * and the sum of squares of the stored (rounded) outputs of every 4-channel unit.  Pass the same buffer to
 * gmk_gn_silu_fwd together with tile_pixels = (256/wo)*wo and ntiles = ceil(B*ho / (256/wo)). */
int gmk_conv_igemm(const void* src0, const void* src1, int c0, int c1, int B, int hs, int ws, int ho, int wo,
                   int ksize, int mode, const void* w, int w_rows, int n0, int cout, const float* bias,
                   const float* emb, int emb_stride, const void* residual, void* out, int out_cstride,
                   float* gn_stats, int64_t gn_stats_bytes, const float* gn_scale, const float* gn_shift, int gn_stride,
                   int dtype, void* stream);
/* gn_scale / gn_shift (optional, fp32 [B][gn_stride], gn_stride >= c0 + c1): the sources are RAW tensors and the convolution
 * applies nn.GroupNorm + nn.SiLU to them on the way into LDS, y = silu(x * gn_scale[b][k] + gn_shift[b][k]) with the tables of
 * gmk_gn_stats (simple_unet.py:161-163,169-172: the normalised tensor is never materialised).  Only where
 * gmk_conv_gn_fusable(...) returns 1; otherwise the call fails. */
int gmk_conv_gn_fusable(int B, int H, int W, int c0, int c1, int cout);
/* 1x1 convolution with TWO 128-channel output blocks (packed weight rows n0 .. n0+127 -> out_a, n0+128 .. n0+255 -> out_b, both
 * NHWC [B][H][W][128]) from ONE pass over the source: the data gradient of the up-path ResBlocks' 1x1 skip_connection
 * (simple_unet.py:176, Conv2d(2C, C, 1)) with respect to the two halves of its concatenated input (torch.cat, :141-147).
 * Two gmk_conv_igemm calls would read the output gradient twice. */
int gmk_conv1x1_pair(const void* src, int c, int B, int H, int W, const void* w, int w_rows, int n0, void* out_a, void* out_b,
                     int dtype, void* stream);
/* conv2 of an up-path ResBlock with its 1x1 skip convolution folded in - `skip_connection(x) + h` of simple_unet.py:174-186 as ONE launch
 * (the reference evaluates Conv2d(2C, C, 1) on torch.cat([x, skip]) and adds the result to out_layers' 3x3 convolution, :177-186):
 *   out[b][y][x][n] = bias[n] + bias_sk[n] + sum_{tap,k} src[b][y+dy][x+dx][k] * w[tap][n0+n][k]
 *                                          + sum_k cat(sk0, sk1)[b][y][x][k] * wsk[nsk0+n][k]
 * src: NHWC, c0 channels (the GroupNorm+SiLU output, simple_unet.py:169-172); sk0 / sk1: the two NHWC halves of the block input, cs
 * channels each; w: packed `[9][w_rows][c0]`, wsk: packed `[wsk_rows][2 cs]` (a w_fwd pack of the 1x1 convolution).  The skip output is
 * never written to or read back from HBM and is added in fp32 (the two-launch path rounds it to 16 bits in between).  Shapes: where
 * gmk_conv3x3_skipfold_ok(...) returns 1 (c0 = cs = cout = 128, a problem the LDS-halo kernel takes); otherwise the call fails. */
int gmk_conv3x3_skipfold_ok(int B, int H, int W, int c0, int cs, int cout);
int gmk_conv3x3_skipfold(const void* src, int c0, int B, int H, int W, const void* w, int w_rows, int n0, int cout,
                         const float* bias, const void* sk0, const void* sk1, int cs, const void* wsk, int wsk_rows, int nsk0,
                         const float* bias_sk, void* out, int out_cstride, int dtype, void* stream);
/* Sub-pixel (output-parity) form of the two x2 resampling convolutions: a LOW-resolution source [B][H][W][cin] -> out [B][2H][2W][cout].
 *   GMK_SUBPIXEL_UPSAMPLE    `Upsample` (simple_unet.py:112-122: F.interpolate(nearest, x2), then Conv2d(C, C, 3, padding=1)).  Output pixel
 *                            (2i + a, 2j + b) only meets low-resolution rows {i + a - 1, i + a} and columns {j + b - 1, j + b}: w is the pack of
 *                            gmk_pack_upsample_weight, `[4 (2a + b) + 2 ty + tx][w_rows][cin]` = the 3x3 weights that land on one low-resolution
 *                            pixel summed in fp32 and rounded once - 16 tap-products per low-resolution pixel instead of the 36 of
 *                            gmk_conv_igemm(GMK_CONV_UPSAMPLE2) (same sum, other rounding order: not bit-identical to it)
 *   GMK_SUBPIXEL_TRANSPOSED  data gradient of `Downsample` (simple_unet.py:75-84, Conv2d(C, C, 3, stride=2, padding=1)): w is the ordinary
 *                            w_dgrad pack `[9][w_rows][cin]` of gmk_pack_conv_weight; parities meet 1 / 2 / 2 / 4 of its taps (the same products
 *                            in the same order as gmk_conv_igemm(GMK_CONV_TRANSPOSED2) on the zero-stuffed gradient, minus its 27 of 36 multiplications by zero)
 * bias optional; residual (NHWC, the output's shape) optional with GMK_SUBPIXEL_TRANSPOSED only.  16-bit types, cin = cout = 128, shapes where gmk_conv_subpixel_ok(...) returns 1; otherwise
 * the call fails (callers fall back to gmk_conv_igemm).  GMK_SUBPIXEL=0 in the environment makes gmk_conv_subpixel_ok answer 0 (A/B switch).
 *   GMK_SUBPIXEL_UPSAMPLE_DGRAD  the data gradient of `Upsample` - HIGH -> LOW: src is the output gradient [B][2H][2W][cin], out [B][H][W][cout] =
 *                            sumpool2x2(dgrad3x3(src)) of the reference's autograd in ONE launch: the transpose of the sub-pixel forward, 16 tap-products
 *                            per low-resolution pixel over the four parity views of src; w = the w_sub_dgrad pack of gmk_pack_upsample_weight
 *                            (`[16][w_rows = Cin of the convolution][Cout]`); (H, W) is the LOW-resolution grid in every mode
 * gmk_pack_upsample_weight: w fp32 [Cout][Cin][3][3] -> w_sub (forward, `dtype`) and / or w_sub_dgrad (`dgrad_dtype`), either may be NULL. */
#define GMK_SUBPIXEL_UPSAMPLE 0
#define GMK_SUBPIXEL_TRANSPOSED 1
#define GMK_SUBPIXEL_UPSAMPLE_DGRAD 2
int gmk_conv_subpixel_ok(int B, int H, int W, int cin, int cout, int dtype);
int gmk_pack_upsample_weight(const float* w, void* w_sub, void* w_sub_dgrad, int cout, int cin, int dtype, int dgrad_dtype, void* stream);
int gmk_conv_subpixel(const void* src, int B, int H, int W, int cin, const void* w, int w_rows, int n0, int cout, int mode,
                      const float* bias, const void* residual, void* out, int out_cstride, int dtype, void* stream);
/* Weight gradient of `Upsample` (simple_unet.py:112-122) in the sub-pixel form: dy = the HIGH-resolution output gradient [B][2H][2W][dy_cstride]
 * (bf16), x = the saved LOW-resolution input [B][H][W][cin] (bf16, or fp16 re-rounded to bf16 on its way into LDS), dw = the reference's
 * [Cout][Cin][3][3] fp32 (overwritten).  The 16 tap gradients of the pre-summed 2x2-tap matrices are accumulated over the low-resolution slots
 * (16 tap-products per low-resolution pixel; gmk_conv_wgrad(GMK_CONV_UPSAMPLE2) multiplies 36) and folded onto the 9 taps by a deterministic
 * two-stage reduce.  cin = cout = 128, W <= 62, where gmk_conv_wgrad_subpixel_ok(...) returns 1 (GMK_SUBPIXEL=0 / GMK_WGRAD_KERNEL != 0: never);
 * workspace: gmk_conv_wgrad_subpixel_workspace_bytes(...) bytes. */
int gmk_conv_wgrad_subpixel_ok(int B, int H, int W, int cin, int cout);
int64_t gmk_conv_wgrad_subpixel_workspace_bytes(int B, int H, int W, int cin, int cout);
int gmk_conv_wgrad_subpixel(const void* dy, int dy_cstride, const void* x, int B, int H, int W, int cin, int cout, float* dw,
                            void* workspace, int64_t workspace_bytes, int dtype, int x_dtype, void* stream);
/* statistics-only GroupNorm for the above: mean / rstd [B][groups] and the affine tables (columns [0, C) of rows of tab_stride
 * floats: a concatenated input passes the same table with a column offset); xadd as in gmk_gn_silu_fwd */
int gmk_gn_stats(const void* x, const float* gamma, const float* beta, float* mean, float* rstd, float* tab_scale,
                 float* tab_shift, int tab_stride, int B, int HW, int C, int groups, float eps, const float* xadd,
                 int xadd_stride, int dtype, void* stream);
/* weight gradient: dw[n][k][tap] (reference layout `[Cout][Cin][k][k]`, fp32, overwritten or accumulated) =
 *   sum_pixels dy[b][oy][ox][n0_dy + n] * srcK[b][sy][sx][k],  same gather as the forward of `mode`.
 * workspace: gmk_conv_wgrad_workspace_bytes(B*ho*wo, ksize*ksize, cout, c0+c1) bytes.
 * dtype: type of dy; x_dtype: type of the saved activations src0 / src1 - the same, or GMK_F16 next to GMK_BF16 gradients (the
 * activations are re-rounded to bf16 on their way into LDS: bf16 x bf16 products, fp32 accumulation). */
int gmk_conv_wgrad(const void* dy, int dy_cstride, const void* src0, const void* src1, int c0, int c1, int B,
                   int hs, int ws, int ho, int wo, int ksize, int mode, float* dw, int cout, void* workspace,
                   int64_t workspace_bytes, int dtype, int x_dtype, void* stream);

/* ---- stem / head convolutions (degenerate channel counts; simple_unet.py:92-94 and :41) ----------------
 * stem: x NCHW fp32 [B][cin][H][W] (cin <= 4) -> y NHWC [B][H][W][C]; w [C][cin][3][3], bias [C] */
int gmk_stem_fwd(const float* x, const float* w, const float* bias, void* y, int B, int cin, int H, int W, int C,
                 int dtype, void* stream);
/* dw_part: fp32 [nblk][C*cin*9] partials in the reference layout [C][cin][3][3], nblk = gmk_stem_wgrad_blocks(B*H*W);
 * reduce over nblk with gmk_colsum */
int gmk_stem_wgrad_blocks(int64_t n_pixels);
int gmk_stem_wgrad(const float* x, const void* dy, float* dw_part, int B, int cin, int H, int W, int C, int dtype,
                   void* stream);
/* head: a NHWC [B][H][W][C] -> out NCHW fp32 [B][cout][H][W] (cout <= 4); w [cout][C][3][3], bias [cout] */
int gmk_head_fwd(const void* a, const float* w, const float* bias, float* out, int B, int cout, int H, int W, int C,
                 int dtype, void* stream);
int gmk_head_dgrad(const float* dout, const float* w, void* da, int B, int cout, int H, int W, int C, int dtype,
                   void* stream);
/* dw_part: fp32 [nblk][cout*C*9 + cout]: weight partials in the reference layout [cout][C][3][3], then cout bias
 * partials; nblk = gmk_head_wgrad_blocks(B*H*W); reduce over nblk with gmk_colsum */
int gmk_head_wgrad_blocks(int64_t n_pixels);
int gmk_head_wgrad(const float* dout, const void* a, float* dw_part, int B, int cout, int H, int W, int C, int dtype,
                   void* stream);
/* stem data gradient (the network's input gradient; an extension, the reference never forms it): dy NHWC [B][H][W][C] (dtype: the
 * compute type, bf16 or fp32; fp16 accepted) -> dx NCHW fp32 [B][cin][H][W] (cin <= 4), the transposed 3x3 / stride-1 / pad-1 convolution
 * with the stem weight w [C][cin][3][3]: dx[b,s,p] = sum_{c,t} dy[b, p - off(t), c] w[c][s][t].  No bias. */
int gmk_stem_dgrad(const void* dy, const float* w, float* dx, int B, int cin, int H, int W, int C, int dtype, void* stream);

/* ---- embedding path (simple_unet.py:20-34,45-64,166,205-224), fp32 -------------------------------------- */
/* out[b][0:32] = cos(t[b]*f_k), out[b][32:64] = sin(t[b]*f_k); freqs: fp32 [32] table computed by the host
 * exactly as simple_unet.py:215-219 does */
int gmk_timestep_embedding(const float* t, const float* freqs, float* out, int B, void* stream);
/* onehot[b][0:10]: F.one_hot(guide with -1 -> 0) as fp32 (simple_unet.py:53-56); keep[b] = guide[b] != -1 */
int gmk_guide_onehot(const int64_t* guide, float* onehot, float* keep, int B, void* stream);
/* classifier-free label drop of DiffusionModel.train_step (diffusion_model.py:67 `y[torch.rand(B) < cf_drop_prob] = -1`), in
 * place on the caller's labels like the reference: y[b] = -1 where gmk_rng_uniform(seed, offset)[b] < p */
int gmk_label_drop(int64_t* y, int B, float p, uint64_t seed, uint64_t offset, void* stream);
/* one training batch from a dataset that lives on the device as the bytes it came as: the reference's transform chain
 * (gms/common.py:104-111: ToTensor, then the threshold or 2 x - 1, then F.pad) applied to images[index], in one launch - what the
 * reference's DataLoader workers do on the host (:116-131).  An extension (data.DeviceDataset), off by default.
 *   images [N][C][H][W] uint8, labels [N] uint8, index [B] int64 with values in [0, N) - the caller guarantees it (ops.batch_gather checks)
 *   x [B][C][H + 2 pad][W + 2 pad] fp32 (16-byte aligned; images / labels / index need their natural alignment only), y [B] int64
 *   x = the bits of the CPU chain: float32(u8) / 255 (correctly rounded), binarize 1: > 0.5 ? 1 : 0, binarize 0: 2 x - 1; then a border of
 *     `pad` ZEROS on each side (F.pad(x, (p, p, p, p)): 0 also for the [-1, 1] data, as in the reference)
 *   flip: image b is mirrored along W (inside its border) where element b of gmk_rng_uniform(seed, offset) over B values is < flip_p -
 *     gmk_label_drop's convention; flip_p = 0 draws nothing, flip_p = 1 mirrors every image
 *   y[b] = labels[index[b]].  Any C H W: rows of whole 16-byte groups ((W + 2 pad) % 4 == 0) take the vector path, others a per-element one. */
int gmk_batch_gather(const uint8_t* images, const uint8_t* labels, const int64_t* index, int B, int64_t N, int C, int H, int W, int pad,
                     int binarize, float flip_p, uint64_t seed, uint64_t offset, float* x, int64_t* y, void* stream);
/* samples as bytes, the inverse direction of gmk_batch_gather: q(x) = (uint8) trunc(min(max((x + 1) * 127.5, 0), 255)), the rule of the
 * reference's `proc` (gms/diffusion/diffusion_model.py:92 `((x + 1) * 127.5).clamp(0, 255).to(torch.uint8)`) with the add and the multiply
 * rounded separately as torch evaluates them; NaN -> 0, -inf -> 0, +inf and overflow -> 255.  An extension, no reference call site except
 * the quantisation rule.
 *   x [n_images][C][H][W] fp32 (16-byte aligned), out [n_images][C][H - 2 crop][W - 2 crop] uint8 (4-byte aligned), planar: the layout
 *   data.load_npy reads.  crop >= 0, 2 crop < min(H, W): the pad32 crop x[..., 2:-2, 2:-2].  Any C, H, W >= 1.  One pass, no temporaries. */
int gmk_to_uint8(const float* x, uint8_t* out, int64_t n_images, int C, int H, int W, int crop, void* stream);
/* T frames of N images each, quantised by the same rule and tiled into pictures, in one launch.  An extension, no reference call site
 * except the quantisation rule (the reference tiles on the host for tensorboard, gms/common.py:177-193).
 *   x [T][N][C][H][W] fp32 (16-byte aligned), C 1 or 3; out_channels = C, or 3 with C = 1 (the grey value repeated)
 *   h = H - 2 crop, w = W - 2 crop, nrow = ceil(N / ncol); a frame has GH = gap + nrow (h + gap) lines of GW = gap + ncol (w + gap) pixels;
 *   image j sits at tile (j / ncol, j % ncol); the border, the gaps and the empty tiles of a partial last row hold `fill` (0..255) in
 *   every channel
 *   out [T][GH][row_prefix + GW out_channels] uint8, channels interleaved; row_prefix 1: every line starts with one byte 0 (PNG filter type
 *   "None"), so a frame is the byte stream zlib turns into an IDAT payload; row_prefix 0: a plain [GH][GW][out_channels] picture
 *   Every source element is read once and every output byte written once; out needs no alignment. */
int gmk_image_grid(const float* x, uint8_t* out, int T, int N, int C, int H, int W, int crop, int ncol, int gap, int fill, int out_channels,
                   int row_prefix, void* stream);
/* out[0] = mean(x[0..n)), fixed summation order: the batch mean of the per-sample losses (diffusion_model.py:78) */
int gmk_mean(const float* x, int n, float* out, void* stream);
/* C[i][j] = (accumulate ? C[i][j] : 0) + rowscale[i] * (bias[j] + bias2[j] + sum_k fa(A[i*sa0 + k*sa1]) * fb(B[k*sb0 + j*sb1]))
 * fa / fb = SiLU when bit 0 / bit 1 of `silu` is set, else identity; bias / bias2 / rowscale may be NULL (bias2: the conv1
 * bias that rides with the 12 emb_layers of simple_unet.py:166,183; rowscale = the
 * `guide != -1` row mask of simple_unet.py:57).  Small strided fp32 GEMM behind every nn.Linear forward/backward
 * of the embedding path. */
int gmk_gemm_f32(const float* A, int64_t sa0, int64_t sa1, const float* B, int64_t sb0, int64_t sb1, float* C,
                 int64_t ldc, int M, int N, int K, const float* bias, const float* bias2, const float* rowscale,
                 int silu, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* scratch the GEMM wants for its deterministic split-K (few output tiles, long K); 0 if none */
int64_t gmk_gemm_f32_workspace_bytes(int M, int N, int K);
/* dpre[i] = dpost[i] * SiLU'(pre[i]) * (rowscale ? rowscale[i / ncols] : 1) */
int gmk_silu_bwd(const float* dpost, const float* pre, const float* rowscale, float* dpre, int64_t n, int ncols,
                 void* stream);
/* out[i] = in[i] * rowscale[i / ncols] */
int gmk_scale_rows(const float* in, const float* rowscale, float* out, int64_t n, int ncols, void* stream);

/* ---- diffusion algebra (gaussian_diffusion.py, diffusion_utils.py), fp32, images as flat [B][n] ---------- */
/* counter-based Philox4x32-10 streams: element i of stream (seed, offset) is reproducible anywhere */
int gmk_rng_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int gmk_rng_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* logsnr[b] = -2 log(tan(a u[b] + b)) (diffusion_utils.py:198-201); z = x sqrt(sigmoid(l)) + eps sqrt(sigmoid(-l))
 * (gaussian_diffusion.py:95-100, diffusion_utils.py:65-73) */
int gmk_q_sample(const float* x, const float* eps, const float* u, float* logsnr, float* z, int B, int64_t n,
                 void* stream);
/* gmk_q_sample under any of the reference's closed-form log-SNR schedules (diffusion_utils.py:169-201; its GaussianDiffusion picks
 * 'cosine', -20, 20, gaussian_diffusion.py:33-34, which gmk_q_sample holds as constants), logsnr(u) =
 *   GMK_SCHED_COSINE       -2 log(tan(a u + b))       b = atan(exp(-lmax / 2)), a = atan(exp(-lmin / 2)) - b
 *   GMK_SCHED_UNIFORM      lmin u + lmax (1 - u)      (the only kind that reads lmin / lmax; the others take their range through a, b)
 *   GMK_SCHED_BETA_CONST   -log(expm1(a u + b))       b = softplus(-lmax), a = softplus(-lmin) - b
 *   GMK_SCHED_BETA_LINEAR  -log(expm1(a u^2 + b))     as beta_const
 * then + shift unless shift == 0 (an additive log-SNR shift, Hoogeboom et al. 2023; no reference call site).  a, b: float64 on the host,
 * rounded to fp32; every operation on the device is one fp32 operation in the reference's order.  With (GMK_SCHED_COSINE, the two
 * constants, shift 0) the bits of gmk_q_sample.  Any n > 0 (gmk_q_sample asks n % 4 == 0).  An unknown kind is GMK_ERR_ARG. */
#define GMK_SCHED_COSINE 0
#define GMK_SCHED_UNIFORM 1
#define GMK_SCHED_BETA_CONST 2
#define GMK_SCHED_BETA_LINEAR 3
int gmk_q_sample_sched(const float* x, const float* eps, const float* u, float* logsnr, float* z, int B, int64_t n, int kind, float a,
                       float b, float lmin, float lmax, float shift, void* stream);
/* gaussian_diffusion.py:58-77,165-169 and their backward in one pass over each sample:
 * x_hat = clip(x_from_output(v)); eps_hat = eps_from_x; loss_b = max(mean (x_hat-x)^2, mean (eps_hat-eps)^2);
 * dv (optional) = d(grad_scale * sum_b loss_b)/dv.  loss_b/x_mse/eps_mse: fp32 [B].
 * mean_type (the reference's `mean_type`, :58-73) says what the network output v is: GMK_MEAN_V 'v' (x = alpha z - sigma v),
 * GMK_MEAN_EPS 'eps' (x = (z - sigma v)/alpha), GMK_MEAN_X 'x' (x = v).  ('both' splits a 1-channel output along W in the reference — dead.) */
#define GMK_MEAN_V 0
#define GMK_MEAN_EPS 1
#define GMK_MEAN_X 2
int gmk_v_loss(const float* v, const float* z, const float* x, const float* eps, const float* logsnr, float* loss_b,
               float* x_mse, float* eps_mse, float* dv, float grad_scale, int loss_type, int mean_type, int B, int64_t n,
               void* stream);
/* loss_type 0 = 'snr_trunc' (max of the two MSEs, :168-169), 1 = 'snr' (eps MSE only, :170-171, distillation step1);
 * x / eps are the denoising targets (x0, eps) or the teacher's (x_target, eps_target). */
/* weighted x-space losses; an extension, no reference call site.  Per image b with l = logsnr[b] (SNR = e^l):
 *   x_hat = clip(x_from_output(v), -1, 1) by mean_type (gmk_v_loss's three formulas), m_b = mean_i (x_hat_i - x_i)^2,
 *   loss_b[b] = w(l) m_b, x_mse[b] = m_b, with
 *     weight_type GMK_LOSS_W_SNR_PLUS1: w = 1 + e^l        (Salimans & Ho 2022, "Progressive Distillation for Fast Sampling of Diffusion
 *                                                           Models", section 4: the 'SNR+1' weighting, the MSE in v space)
 *     weight_type GMK_LOSS_W_MIN_SNR:   w = min(e^l, gamma) (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy")
 *   dv (optional) = d(grad_scale * sum_b loss_b)/dv: dv_i = grad_scale w (2 / n) (x_hat_i - x_i) dx/dout where the raw prediction lies in
 *   [-1, 1] (ends included), else 0 - gmk_v_loss's clip rule; w depends on l alone, so the min routes nothing.
 * x_mse carries the bits gmk_v_loss writes to its x_mse for the same (v, z, x, logsnr, mean_type): the same element-to-thread assignment and
 * summation order, on the 16-byte path (n % 4 == 0 and v, z, x, dv 16-byte aligned) and on the scalar one.  Images of up to 12,288 values keep
 * their residuals in LDS between the reduction and the gradient (v, z, x are read once); larger ones are read again.  gamma: finite, > 0
 * (checked for either weight_type).  loss_b, x_mse: fp32 [B], both required. */
#define GMK_LOSS_W_SNR_PLUS1 0
#define GMK_LOSS_W_MIN_SNR 1
#define GMK_X_LOSS_KEEP 12288      /* the "12,288 values" above (covers 3 x 64 x 64) */
int gmk_x_loss_w(const float* v, const float* z, const float* x, const float* logsnr, float* loss_b, float* x_mse, float* dv,
                 float grad_scale, int weight_type, float gamma, int mean_type, int B, int64_t n, void* stream);
/* low-discrepancy training times (Kingma et al. 2021, "Variational Diffusion Models", App. I.1); an extension: u[b] = frac(u0[0] + b / B) as
 *   s = fdiv(b, B), c = fsub(1, s), u[b] = u0 >= c ? fsub(u0, c) : min(fadd(u0, s), 1 - 2^-24)
 * - single correctly rounded fp32 operations; the wrap comes before the sum because fadd(u0, s) is not exact at or above 1.  With B a power
 * of two and u0 a multiple of 2^-24 (gmk_rng_uniform's values) all of it is exact and every [k / B, (k + 1) / B) holds exactly one u; u lies in
 * [0, 1) for every B.  u0: one value in [0, 1); u: fp32 [B], 1 <= B <= 2^24. */
int gmk_u_stratified(const float* u0, float* u, int B, void* stream);
/* the per-log-SNR loss profile and the loss-aware time sampler (Nichol & Dhariwal 2021, "Improved DDPM", section 3.3); extensions.
 * GMK_PROFILE_BINS bins of equal width in the time variable u in [0, 1) (one per lane of a wavefront; equal mass under uniform draws).
 * state: fp32 [5][64] - row 0 W, the decayed sample count; rows 1, 2 S1, S2, the decayed sum and sum of squares of value channel 0; rows 3, 4
 * the same of value channel 1.  Single correctly rounded fp32 operations in a stated order, as gmk_u_stratified: numpy float32 restates both
 * entries bit for bit.
 * gmk_loss_profile: sample b belongs to bin k = min((int)fmul(u[b], 64), 63); it is skipped entirely when u[b] is not in [0, 1) or v0[b] (or
 * v1[b], when given) is not finite.  Per bin, over its samples in ascending b: n = their count, a_c = the sequential fadd of the values (from
 * 0), q_c = the sequential fadd(q, fmul(v, v)).  A bin with n > 0 takes W = fadd(fmul(decay, W), n), S1_c = fadd(fmul(decay, S1_c), a_c),
 * S2_c = fadd(fmul(decay, S2_c), q_c): a per-bin window over the bin's own samples (decay = 1: plain sums).  A bin with n = 0 keeps its five
 * words' bits; rows 3 and 4 keep theirs when v1 is NULL.  No atomics: a pure function of the inputs.  One workgroup.
 * u, v0, v1: fp32 [B], 1 <= B <= 2^24; 0 < decay <= 1. */
#define GMK_PROFILE_BINS 64
int gmk_loss_profile(const float* u, const float* v0, const float* v1, int B, float decay, float* state, void* stream);
/* gmk_u_importance: the inverse-CDF draw from the profile and its importance weight.  The table, in bin order:
 *   ready = every W_k >= warm;  r_k = fsqrt(fdiv(S2_k, W_k)) on channel 0;  R = the sequential fadd of r_k (from 0)
 *   p_k = fadd(fmul(fdiv(r_k, R), fsub(1, floor)), fdiv(floor, 64)) when ready and R is finite and > 0, else 2^-6
 *   c_0 = 0, c_{k+1} = fadd(c_k, p_k), C = c_64;  w_k = fdiv(C, fmul(64, p_k))
 * per draw: t = fmul(u0[b], C), k = the largest index in 0..63 with c_k <= t, f = min(fdiv(fsub(t, c_k), p_k), 1 - 2^-24),
 *   u[b] = min(fmul(fadd((float)k, f), 2^-6), nextafterf((k + 1) 2^-6, 0)),  w[b] = w_k
 * - the last min keeps u inside bin k and below 1, so w[b] == w_out[floor(64 u[b])].  With p_k = 2^-6 every operation is exact for every fp32
 * u0 in [0, 1): u == u0 bit for bit and w == 1.  E[w g(u)] over uniform u0 is the integral of g.
 * u0, u, w: fp32 [B], u0 in [0, 1), 1 <= B <= 2^24; warm >= 0; 0 < floor <= 1; p_out, w_out: NULL or fp32 [64], the table's p_k and w_k. */
int gmk_u_importance(const float* state, const float* u0, float* u, float* w, int B, float warm, float floor, float* p_out, float* w_out,
                     void* stream);
/* one reverse step on a batch (gaussian_diffusion.py:189-243,174-187,292):
 *   v: conditional net output; v_uncond/cond_w: NULL or the unconditional output + per-sample guidance weight;
 *   noise: NULL -> DDIM update, else ancestral ('noisy') update with that noise; is_last: the i == 0 select.
 *   z_next is written; x_pred / eps_pred are optional outputs.
 *   z_dup (optional): a second copy of z_next - the other half of the 2B-image batch the guided sampler feeds the network (:176-177
 *   evaluates the net twice on the same z); logsnr_next (optional, B floats, 2B with z_dup): filled with logsnr_s, which is the next
 *   iteration's logsnr_t (u_t(i-1) = u_s(i), :288-290) - the loop then needs neither torch.cat nor torch.full per step. */
int gmk_sampler_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* noise,
                     float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred, float* eps_pred,
                     float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream);
/* one DPM-Solver++(2M) step (Lu et al. 2022, Algorithm 2, data prediction) on the same time grid; an extension, no reference call site:
 *   v, v_uncond, cond_w, mean_type: as gmk_sampler_step - x_hat is the clipped (guided) data prediction of that step, eps_hat = eps(x_hat, z).
 *   x_hist: B x n, in place: the previous step's x_hat on entry (not read when coef_prev == 0), this step's x_hat on exit.
 *   coef_z = sigma_s / sigma_t, coef_x = -alpha_s expm1(-h), coef_prev = 1 / (2 r) with h = (logsnr_s - logsnr_t) / 2 and r = h_prev / h
 *   (0 on the first step: DDIM's update; the host passes 0 on the last step too); z_next = coef_z z + coef_x ((1 + coef_prev) x_hat - coef_prev x_prev), or x_hat when is_last.
 *   logsnr_t: the network's time (x_hat, eps_hat); logsnr_s: written to logsnr_next.  x_pred / eps_pred (optional) receive x_hat and eps_hat;
 *   z_dup / logsnr_next: gmk_sampler_step's conventions.  The host computes the coefficients in double from the fp32 log-SNRs. */
int gmk_dpm_solver_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float* x_hist, float logsnr_t,
                        float logsnr_s, float coef_z, float coef_x, float coef_prev, int is_last, float* z_next, float* x_pred,
                        float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream);
/* dynamic thresholding of the data prediction (Saharia et al. 2022, Imagen, section 2.3); an extension, no reference call site.
 *   x_raw: the UNCLIPPED prediction of one network evaluation at (z, logsnr_t): x_c = x(v) by mean_type (gmk_v_loss's formulas); unguided
 *     x_raw = x_c; guided e_c = eps(z, x_c), e_u = eps(z, x(v_uncond)), e = (1 + w_b) e_c + (-w_b) e_u, x_raw = x(z, e) - gmk_sampler_step's
 *     guidance without its three clips (a prediction clipped at +-1 before the extrapolation would defeat the threshold).  eps(z, .) and x(z, .)
 *     are affine and inverse to each other, so this is (1 + w_b) x_c + (-w_b) x(v_uncond), the form the kernels evaluate: the round trip through
 *     eps space cancels in fp32 at low SNR (1e-3 relative in x_raw at logsnr -20).
 *   gmk_dyn_threshold: per image b, q_b = a[k_lo] + frac (a[hi] - a[k_lo]) in fp32, a = |x_raw[b]| sorted ascending, hi = min(k_lo + 1, n - 1):
 *     torch.quantile's linear rule for p with p (n - 1) = k_lo + frac (the host splits it in double).  a[k_lo] and a[hi] are exact order
 *     statistics (a radix select over the values' bits in LDS, one workgroup per image; no floating-point atomics: the same call gives the same
 *     bits).  s_out[b] = max(1, q_b); q_out (optional, B floats) receives q_b itself.  0 <= k_lo < n < 2^31, 0 <= frac < 1; any n >= 1 (images of up
 *     to 12,288 values are read once and selected in LDS, larger ones are re-read per pass).  Non-finite inputs give unspecified values, nothing else.
 *   gmk_sampler_step_dt / gmk_dpm_solver_step_dt: gmk_sampler_step / gmk_dpm_solver_step with x_hat = min(max(x_raw, -thr_b), thr_b) / thr_b (a true
 *     division) in place of the clipped prediction; eps_hat = eps(z, x_hat) and everything after it (the update, x_hist, the is_last select, z_dup,
 *     logsnr_next) unchanged.  thr: B floats, required (gmk_dyn_threshold's s_out).  With thr = 1 and no guidance they give the bits of the entries
 *     without _dt: the same kernels, instantiated a second time. */
#define GMK_DYN_THRESHOLD_KEYS 12288      /* the "12,288 values" of gmk_dyn_threshold */
int gmk_dyn_threshold(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, int k_lo, float frac,
                      float* s_out, float* q_out, int mean_type, int B, int64_t n, void* stream);
int gmk_sampler_step_dt(const float* v, const float* v_uncond, const float* cond_w, const float* thr, const float* z, const float* noise,
                        float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                        float* logsnr_next, int mean_type, int B, int64_t n, void* stream);
int gmk_dpm_solver_step_dt(const float* v, const float* v_uncond, const float* cond_w, const float* thr, const float* z, float* x_hist,
                           float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_prev, int is_last, float* z_next,
                           float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream);
/* the rescale factor of classifier-free guidance (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4:
 * the guided prediction scaled back towards the conditional prediction's standard deviation), which the samplers apply on the steps inside the
 * guidance interval (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and Distribution Quality in Diffusion
 * Models"); an extension, no reference call site.  Per image b, in fp32, with x_c = x(v) and x_raw = (1 + w_b) x_c + (-w_b) x(v_uncond) exactly
 * as gmk_dyn_threshold forms them (the same device function, the same bits, no clip anywhere):
 *   m_c = (sum x_c) / n, m_r = (sum x_raw) / n;  q_c = sum (x_c - m_c)^2, q_r = sum (x_raw - m_r)^2   (two passes with centred squares)
 *   ratio = sqrtf(q_c / q_r) = std(x_c) / std(x_raw);  f = fadd(1, fmul(phi, fsub(ratio, 1)));  thr_out[b] = 1 / f, a true division;
 *   thr_out[b] = 1 where q_r == 0, f is not finite or f <= 0.  ratio_out (optional, B floats) receives ratio (NaN where q_c = q_r = 0).
 * clamp(x, -thr, thr) / thr = clip(f x, -1, 1) for thr = 1 / f > 0, so gmk_sampler_step_dt / gmk_dpm_solver_step_dt called with thr_out ARE the
 * rescaled update; ratio == 1 or phi == 0 gives thr = 1 exactly.  One workgroup of 256 threads per image; every sum runs in one order (thread t
 * adds the elements t, t + 256, ... ascending, then the workgroup's tree: ceil(n / 256) + 8 additions per chain) without floating-point atomics, so
 * the same call gives the same bits, a half-batch gives the whole batch's rows, and w_b = 0 gives q_r == q_c bit for bit (thr = ratio = 1).
 * Images of up to 12,288 values are read once (12 bytes per value) and kept in registers between the passes, larger ones are read again.
 * 16-byte loads when n % 4 == 0 and v, v_uncond, z are 16-byte aligned, else element by element.  v, v_uncond, cond_w, z, thr_out required;
 * 0 <= phi <= 1; B, n >= 1; logsnr_t finite.  Non-finite inputs give thr = 1 or unspecified values, nothing else. */
#define GMK_CFG_RESCALE_KEEP 12288      /* the "12,288 values" of gmk_cfg_rescale; a multiple of 1024 */
int gmk_cfg_rescale(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, float phi, float* thr_out,
                    float* ratio_out, int mean_type, int B, int64_t n, void* stream);
/* DDNM restoration for box-mean operators (Wang, Yu & Zhang 2023, "Zero-Shot Image Restoration Using Denoising Diffusion Null-Space Model",
 * eq. 13-14, noise-free); an extension, no reference call site.  Images are NCHW fp32, n = C H W.  The operator A has parameters (cf, N):
 * cf in {1, C} channels are averaged together (cf = C: colourisation), N >= 1 is the side of the spatial box (H % N == 0, W % N == 0), k = cf N^2.
 * Box g = (c', i, j), c' < C / cf, i < H / N, j < W / N, holds the elements (c' cf + dc, i N + dy, j N + dx); the low-resolution layout is
 * [B][C / cf][H / N][W / N] fp32, n_box = n / k values per image.
 *   A x [g] = fdiv(s, (float)k), s the sequential fp32 add, from 0, of the members in row-major (dc, dy, dx) order (nothing contracted: the same
 *     call gives the same bits).  A+ u replicates u[g] over the members of g, so A A+ = I and x + A+(y - A x) projects onto {x : A x = y}.
 *   gmk_box_mean: out = A x.  Any k >= 1.
 *   gmk_box_residual: r[b][g] = fsub(obs[b][g], (A x_hat)[b][g]), x_hat exactly the clipped (and, with v_uncond / cond_w, guided) data prediction
 *     gmk_sampler_step forms for (v, v_uncond, cond_w, z, logsnr_t, mean_type): the same device function, the same bits.  One thread per box;
 *     v, z (and v_uncond) are read once, n_box floats per image are written.
 *   gmk_sampler_step_ns / gmk_dpm_solver_step_ns: gmk_sampler_step / gmk_dpm_solver_step with x_hat' = fadd(x_hat, r[b][box of the element]) in
 *     place of x_hat and eps_hat = eps(z, x_hat'); everything after it (the DDIM / ancestral / solver update, x_hist, the is_last select, z_dup,
 *     logsnr_next, x_pred, eps_pred) unchanged and on x_hat'.  x_hat' is not clipped again (a second clip would break A x_hat' = obs); it lies in
 *     [-3, 3].  r: B x n_box floats, required (gmk_box_residual's output); n must equal C H W.  With r = 0 they give the bits of the entries
 *     without _ns: the same kernels, instantiated once more.
 * Errors (GMK_ERR_ARG): cf not in {1, C}; N not dividing H or W; B n_box >= 2^31; C H W >= 2^31. */
int gmk_box_mean(const float* x, float* out, int B, int C, int H, int W, int cf, int N, void* stream);
int gmk_box_residual(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* obs, float logsnr_t, float* r,
                     int mean_type, int B, int C, int H, int W, int cf, int N, void* stream);
int gmk_sampler_step_ns(const float* v, const float* v_uncond, const float* cond_w, const float* r, const float* z, const float* noise,
                        float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                        float* logsnr_next, int mean_type, int B, int64_t n, int C, int H, int W, int cf, int N, void* stream);
int gmk_dpm_solver_step_ns(const float* v, const float* v_uncond, const float* cond_w, const float* r, const float* z, float* x_hist,
                           float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_prev, int is_last, float* z_next,
                           float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, int C, int H,
                           int W, int cf, int N, void* stream);
/* Diffusion posterior sampling (DPS: Chung et al. 2023, "Diffusion Posterior Sampling for General Noisy Inverse Problems", Algorithm 1); an
 * extension, no reference call site.  The observation is y = A x + noise, A linear on NCHW fp32 images, n = C H W:
 *   GMK_DPS_BOX   the box mean (cf, N) above: y is [B][C / cf][H / N][W / N]; A^T e = fdiv(e[g], (float)k) replicated over the members of box g.
 *   GMK_DPS_BLUR  a separable Gaussian blur per channel with zero padding, y of the image's shape.  taps: 2 R + 1 device floats, taps[k + R] the
 *     weight of offset k (the host normalises them), 1 <= R <= GMK_BLUR_MAX_R, H, W <= GMK_BLUR_MAX_SIDE (a plane is staged in LDS).  Rows
 *     first, t[y][x] = sum_k taps[k + R] x[y][x + k], then columns, out[y][x] = sum_k taps[k + R] t[y + k][x]; each sum starts from 0 and adds
 *     fmul(tap, value) for k = -R ... R in that order, the terms outside the plane left out.  Symmetric taps make A symmetric: A^T = A.
 *   gmk_gauss_blur: out = A x.  One workgroup per image, which loops over the channels.
 *   gmk_dps_backproject: x_hat the UNCLIPPED, unguided data prediction of (v, z, logsnr_t, mean_type) (a clip has zero gradient where the early
 *     steps saturate), e = fsub(obs, A x_hat), u = A^T e (B x n), enorm2[b] = |e_b|^2: per thread the sequential fp32 sum of fmul(e, e) over
 *     its elements, then a 256-leaf binary tree in LDS - no atomics, the same call gives the same bits.  One workgroup per image; v and z are
 *     read once.  The blur is gmk_gauss_blur's device function: its bits.  box: cf, N are read; blur: taps, R.
 *   gmk_dps_correct: in place, z = fadd(z, fmul(s_b, fadd(fmul(c_z, u), fmul(c_o, g)))), s_b = min(fdiv(2 zeta, max(sqrt(enorm2[b]), FLT_MIN)),
 *     FLT_MAX) - the paper's step zeta_i = zeta / |y - A x_hat| along -grad |y - A x_hat|^2 = 2 (c_z u + c_o g), g = (d out / d z)^T u the
 *     network's input VJP and (c_z, c_o) = d x_hat / d (z, out).  n % 4 == 0, 16-byte aligned rows; zeta finite, >= 0; zeta = 0 launches
 *     nothing (z keeps its bits).  No rows of GMK_KERNEL_TABLE. */
#define GMK_DPS_BOX 0
#define GMK_DPS_BLUR 1
#define GMK_BLUR_MAX_R 15
#define GMK_BLUR_MAX_SIDE 64
int gmk_gauss_blur(const float* x, float* out, const float* taps, int R, int B, int C, int H, int W, void* stream);
int gmk_dps_backproject(const float* v, const float* z, const float* obs, float logsnr_t, int op, int cf, int N, const float* taps, int R,
                        float* u, float* enorm2, int mean_type, int B, int C, int H, int W, void* stream);
int gmk_dps_correct(float* z, const float* u, const float* g, const float* enorm2, float c_z, float c_o, float zeta, int B, int64_t n,
                    void* stream);
/* RePaint inpainting merge (Lugmayr et al. 2022, Algorithm 1, jump length 1); an extension, no reference call site.  In place on z (B x n,
 * fp32), after the sampler update of a step t -> s has written it.  mask: uint8 B x n in x's element order, nonzero = known pixel; x0: the
 * known image (B x n fp32).  n % 4 == 0.
 *   known = is_last ? x0 : alpha_s x0 + sigma_s eps1;  z = mask ? known : z  (a select: unknown pixels keep their bits)
 *   renoise (never with is_last): z = a z + b eps2, a = alpha_t / alpha_s, b = sqrt(1 - alpha_t^2 / alpha_s^2): back to time t.
 * alpha^2 = sigmoid(logsnr), sigma^2 = sigmoid(-logsnr); the host computes the four coefficients in double from the fp32 log-SNRs.
 * eps1 / eps2 are Philox normals drawn in the kernel and never stored: with N = B_total n / 4, element j of this chunk is element j of
 * gmk_rng_normal(seed, offset + q0) (eps1) and of gmk_rng_normal(seed, offset + N + q0) (eps2) - so a chunk of rows at counter offset q0
 * inside a batch of B_total rows draws exactly what the whole batch would.  z_dup (optional): a second copy of z (the guided 2B batch's
 * other half); logsnr_next (optional, B floats, 2B with z_dup): filled with logsnr_t when renoise, else logsnr_s. */
int gmk_inpaint_merge(float* z, const float* x0, const uint8_t* mask, float alpha_s, float sigma_s, float a, float b, int is_last,
                      int renoise, float logsnr_t, float logsnr_s, uint64_t seed, uint64_t offset, uint64_t q0, int B_total, float* z_dup,
                      float* logsnr_next, int B, int64_t n, void* stream);
/* continuous-time variational bound (Kingma et al. 2021, VDM eq. 17 in lambda = logsnr, lambda in [-20, 20]); an extension, no reference
 * call site.  Any n (rows of 4k floats take the vector path).
 *   gmk_q_sample_logsnr: z = alpha x + sigma eps at the given per-sample logsnr[B] (alpha^2 = sigmoid(l), sigma^2 = sigmoid(-l)).
 *   gmk_vlb_term: acc[b] += weight[b] * sum_i (eps - eps_hat)^2, eps_hat the UNCLIPPED noise prediction of the net output `out` at z, logsnr:
 *     mean_type 0 'v' sigma z + alpha out, 1 'eps' out, 2 'x' (z - alpha out) / sigma.  acc is read and written (accumulates).
 *   gmk_vlb_endpoints: per image, out_prior[b] = sum_i KL(N(alpha_1 x, sigma_1^2) || N(0, 1)) at lambda = -20 and
 *     out_dec[b] = sum_i -log[Phi((x + delta - m) / s) - Phi((x - delta - m) / s)], the discretised Gaussian at lambda = 20 with
 *     m = z_0 / alpha_0, s = sigma_0 / alpha_0, z_0 = alpha_0 x + sigma_0 eps0 (nats).  Bins are centred on x; the top bin's upper edge
 *     (x > 1 - delta) is +inf, the bottom bin's lower edge (x < lo + delta) -inf, lo = 0 for binarised data (delta = 1/2, values {0, 1}),
 *     else -1 (delta = 1/255 for [-1, 1] data).  0 < delta <= 1/2. */
int gmk_q_sample_logsnr(const float* x, const float* eps, const float* logsnr, float* z, int B, int64_t n, void* stream);
int gmk_vlb_term(const float* out, const float* z, const float* eps, const float* logsnr, const float* weight, float* acc, int mean_type,
                 int B, int64_t n, void* stream);
int gmk_vlb_endpoints(const float* x, const float* eps0, float delta, float* out_prior, float* out_dec, int B, int64_t n, void* stream);
/* probability-flow ODE (Song et al. 2021, section 4.3 / App. D.2) in lambda = logsnr; an extension, no reference call site.
 *   gmk_rng_rademacher: out[i] = +1 where u >= 1/2, -1 elsewhere, u = element i of gmk_rng_uniform(seed, offset) (Hutchinson probes).
 *   gmk_dequantize: y = x + delta (2 u - 1), u = element i of gmk_rng_uniform(seed, offset) (drawn in the kernel, never stored).
 *   gmk_pf_ode_step: one network evaluation `out` at (z, logsnr_i), B x n fp32.  eps_hat = the UNCLIPPED noise prediction of gmk_vlb_term,
 *     x_hat = 'v' alpha z - sigma out, 'eps' (z - sigma out) / alpha, 'x' out (= (z - sigma eps_hat) / alpha).
 *     update != 0: z = alpha_j x_hat + sigma_j eps_hat in place (alpha_j, sigma_j at logsnr_j: DDIM's update without the clip).
 *     x_out (optional): receives x_hat.
 *     acc (optional, B floats): acc[b] += div_a + div_b sum_i r g, the trapezoid-weighted divergence of the ODE's drift (host coefficients:
 *       w_i (1/2 sigma_i^2 n - 1/2 sigma_i c_z n) and -w_i 1/2 sigma_i c_o); needs r (the probe) and g (the input VJP of `out` along r).
 *     prior (optional, B floats, never with update): prior[b] = 1/2 sum_i z^2 + prior_c, i.e. -log N(z; 0, I) with prior_c = n/2 log(2 pi).
 *   With acc or prior the grid is one workgroup per image (a fixed-order reduction: repeated calls give the same bits).  Any n. */
int gmk_rng_rademacher(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int gmk_dequantize(const float* x, float* y, float delta, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int gmk_pf_ode_step(const float* out, float* z, const float* r, const float* g, float* acc, float* prior, float* x_out, float logsnr_i,
                    float logsnr_j, int update, float div_a, float div_b, float prior_c, int mean_type, int B, int64_t n, void* stream);
/* spherical interpolation between two batches of latent codes (Shoemake 1985; the DDIM paper's interpolation of x_T, Song et al. 2021,
 * section 5.3); an extension, no reference call site.  a, b: B x n fp32; t: K fp32 values on the device; out: K x B x n.  Per image, in fp32:
 *   dot = sum a b, na = sum a^2, nb = sum b^2, c = clamp(dot / sqrt(na nb), -1, 1), theta = acosf(c), s = sinf(theta)
 *   out[k] = w_a a + w_b b with w_a = sinf((1 - t_k) theta) / s, w_b = sinf(t_k theta) / s
 *   fallback (s < 1e-6 or c not finite: parallel, antipodal and all-zero rows): w_a = 1 - t_k, w_b = t_k - the lerp, which writes no NaN for
 *   finite inputs.
 * t_k = 0 gives a's values and t_k = 1 gives b's exactly on either branch (s / s = 1, sinf(0) = 0; IEEE division, nothing contracted).
 * cos_out (optional, B floats) receives c (NaN for an all-zero row: the clamp keeps it).  One launch, one workgroup per image; the sums run in
 * a fixed order without floating-point atomics, so the same call gives the same bits.  Images of up to 12,288 values stay in registers between
 * the reduction and the K output passes (a and b are read once), larger ones are read again per k.  B, K >= 1, n >= 4, n % 4 == 0; a, b and
 * out 16-byte aligned (16-byte loads and stores). */
#define GMK_SLERP_KEEP 12288      /* the "12,288 values" above; a multiple of 1024 */
int gmk_slerp(const float* a, const float* b, const float* t, float* out, float* cos_out, int B, int64_t n, int K, void* stream);

/* ---- self-attention core (north_star "optional self-attention block", BASELINE config 5) -------------
 * The reference SimpleUnet has no attention block: these have NO reference call site (parity unpinned; their definition is the
 * CPU restatement `attention_block` the tests check them against).  QK^T / PV and their gradients are one batched GEMM on the matrix cores:
 *   C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k]      (both operands K-contiguous; leading dimensions and batch
 *   strides in elements; bf16 operands: K and all strides multiples of 8; out_dtype GMK_F32 or GMK_BF16) */
int gmk_bgemm_nt(const void* A, int64_t a_batch, int64_t lda, const void* B, int64_t b_batch, int64_t ldb, void* C,
                 int64_t c_batch, int64_t ldc, int batch, int M, int N, int K, float alpha, int in_dtype, int out_dtype,
                 void* stream);
/* out[b][c][r] = in[b][r][c]  (R x Cc matrices, leading dimensions / batch strides in elements) */
int gmk_transpose(const void* in, int64_t in_batch, int64_t ld_in, void* out, int64_t out_batch, int64_t ld_out, int batch,
                  int R, int Cc, int dtype, void* stream);
/* P[r][:] = softmax(scale * S[r][:]) over rows of N <= 1024 fp32 scores; P in out_dtype */
int gmk_softmax_fwd(const float* S, void* P, int64_t rows, int N, float scale, int out_dtype, void* stream);
/* dS = scale * P * (dP - sum_j dP_j P_j)  (P, dS in dtype; dP fp32) */
/* fused forward of the block's core: o[b] = softmax(scale * q[b] k[b]^T) v[b] with q, k, v the three C-column blocks of qkv
 * [B][N][3C] (bf16), one workgroup per sample, K / V resident in LDS, no N x N matrix in HBM unless p_out (bf16 [B][N][N], the
 * probabilities the backward pass needs) is given.  fp8 != 0: both contractions on the fp8 (OCP e4m3) matrix cores with fp32
 * accumulation - BASELINE config 5's "fp8 MFMA".  With fp8, q, k and v saturate to +-448, the largest e4m3 magnitude, before the e4m3
 * rounding (round to nearest even; NaN stays NaN).  C = 128, N in {64, 128, 256}. */
int gmk_attention_fwd(const void* qkv, void* o, void* p_out, int B, int N, int C, float scale, int fp8, void* stream);
/* fused backward of the same core (round 5): dqkv [B][N][3C] (bf16) = (dq | dk | dv) given d_o [B][N][C] (bf16), the forward's inputs qkv and output o.
 * P is recomputed block by block in registers: no N x N matrix in HBM (the three-kernel path kept P [B][N][N] and a fp32 dP of that shape).  stats:
 * fp32 scratch [B][N][2] (log2-domain LSE and sum_c dO O per query, written by the first of the two kernels).  bf16 arithmetic with fp32 accumulation
 * also behind the fp8 forward (straight-through for the e4m3 rounding); deterministic.  C = 128, N in {64, 128, 256}. */
int gmk_attention_bwd(const void* qkv, const void* o, const void* d_o, void* dqkv, float* stats, int B, int N, int C, float scale, void* stream);
int gmk_softmax_bwd(const void* P, const float* dP, void* dS, int64_t rows, int N, float scale, int dtype, void* stream);

/* ---- progressive distillation (gaussian_diffusion.py:87-91,105-154) ------------------------------------------ */
/* logsnr[b] = schedule(u[b] - shift) with u given, or u = fp32(i_times[b] + 1) / num_steps (discrete time, :90-91);
 * u_out (optional) receives the shifted u */
int gmk_logsnr_schedule(const float* u, const int64_t* i_times, int num_steps, float shift, float* u_out, float* logsnr,
                        int B, void* stream);
/* the same under a schedule of gmk_q_sample_sched (diffusion_utils.py:169-201): logsnr[b] = schedule(u[b] - u_shift) + shift */
int gmk_logsnr_schedule_sched(const float* u, const int64_t* i_times, int num_steps, float u_shift, int kind, float a, float b, float lmin,
                              float lmax, float shift, float* u_out, float* logsnr, int B, void* stream);
/* one DDIM step with per-sample times logsnr_t[b] -> logsnr_s[b] (teacher steps inside the loss, :116,:129-144) */
int gmk_ddim_step_vec(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* logsnr_t,
                      const float* logsnr_s, float* z_next, float* x_pred, float* eps_pred, int mean_type, int B, int64_t n,
                      void* stream);
/* x_target = (z_teacher - f z_t) / (alpha_s - f alpha_t), f = exp((softplus(l) - softplus(l_s)) / 2); the i == 0 rows
 * take x_pred_teacher; eps_target = eps_from_x(z_t, x_target, l)  (:147-154) */
int gmk_distill_target(const float* z_teacher, const float* z_t, const float* x_pred_teacher, const float* logsnr,
                       const float* logsnr_s, const int64_t* i_times, float* x_target, float* eps_target, int B, int64_t n,
                       void* stream);

/* ---- consistency distillation and multistep consistency sampling (Song, Dhariwal, Chen & Sutskever 2023, "Consistency Models", Algorithms 2
 * and 1); extensions, no reference call site.  alpha(l) = sqrt(sigmoid(l)), sigma(l) = sqrt(sigmoid(-l)); x_hat(out, z, l) is the CLIPPED data
 * prediction of gmk_sampler_step / gmk_v_loss for the three mean_types; eps_from_x(z, x, l) = (z - alpha x) / sigma in gmk_distill_target's form
 * sqrt(1 + e^l) (z - x / sqrt(1 + e^-l)).  All three work on fp32 images as flat [B][n], without floating-point atomics (the same call gives
 * the same bits); no row of GMK_KERNEL_TABLE: they carry no profile label.
 *   gmk_consistency_target: the distillation target of one batch.  z_s = the teacher's DDIM step from z_t (gmk_ddim_step_vec), x_pred_teacher its
 *     x_pred, v_tgt the target network's output at (z_s, logsnr_s):
 *       x_target[b] = i_times[b] == 0 ? x_pred_teacher[b] : x_hat(v_tgt[b], z_s[b], logsnr_s[b])
 *       eps_target[b] = eps_from_x(z_t[b], x_target[b], logsnr_t[b])
 *     The i == 0 rows are the boundary condition f(., t_min) = identity on the teacher's final prediction (v_tgt and z_s are not read there).
 *     x_hat is the device function behind gmk_ddim_step_vec's x_pred, eps_target the expression gmk_distill_target ends with: their bits.
 *     Any n: 16-byte accesses when n % 4 == 0 and the six image tensors are 16-byte aligned, else element by element.  B < 65536.
 *   gmk_x_loss_huber: the pseudo-Huber metric of Song & Dhariwal 2023, "Improved Techniques for Training Consistency Models", on x_hat:
 *       m_b = mean_j (x_hat_j - x_j)^2, loss_b[b] = sqrt(m_b + c^2) - c, x_mse[b] = m_b
 *     - the paper's sqrt(|d|^2 + c_paper^2) - c_paper with c_paper = c sqrt(n), scaled by 1 / sqrt(n) (its default 0.00054 sqrt(n) is c = 0.00054).
 *     dv (optional) = d(grad_scale sum_b loss_b)/dv: dv_j = grad_scale (x_hat_j - x_j) / (n sqrt(m_b + c^2)) dx_hat/dout where the raw prediction
 *     lies in [-1, 1] (ends included), else 0 - gmk_v_loss's clip rule.  gmk_x_loss_w's kernel, instantiated once more: one workgroup per image,
 *     residuals in LDS up to GMK_X_LOSS_KEEP values (larger images are read again), the same 16-byte / scalar rule, and x_mse carries the bits
 *     gmk_x_loss_w writes for the same inputs.  c: finite, > 0.  loss_b, x_mse: fp32 [B], both required.
 *   gmk_consistency_step: one step t -> s of multistep consistency sampling on the samplers' grid.  x_hat / eps_hat exactly as gmk_sampler_step
 *     forms them (v_uncond / cond_w: classifier-free guidance), then
 *       z_next = is_last ? x_hat : fadd(fmul(alpha_s, x_hat), fmul(sigma_s, eps))     (nothing contracted)
 *     alpha_s, sigma_s computed by the entry in double from the fp32 logsnr_s and rounded to fp32.  eps are Philox normals drawn in the kernel
 *     and never stored: element j of this chunk is element j of gmk_rng_normal(seed, offset + q0) - so rows [a, b) of a batch called with
 *     q0 = a n / 4 draw exactly what the whole batch would (gmk_inpaint_merge's convention).  Nothing is drawn when is_last.  n % 4 == 0.
 *     x_pred / eps_pred / z_dup / logsnr_next: gmk_sampler_step's conventions. */
int gmk_consistency_target(const float* v_tgt, const float* z_s, const float* x_pred_teacher, const float* z_t, const float* logsnr_t,
                           const float* logsnr_s, const int64_t* i_times, float* x_target, float* eps_target, int mean_type, int B, int64_t n,
                           void* stream);
int gmk_x_loss_huber(const float* v, const float* z, const float* x, const float* logsnr, float* loss_b, float* x_mse, float* dv,
                     float grad_scale, float c, int mean_type, int B, int64_t n, void* stream);
int gmk_consistency_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, float logsnr_s, int is_last,
                         uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                         float* logsnr_next, int mean_type, int B, int64_t n, void* stream);

/* ---- the stochastic samplers: one step t -> s on the samplers' grid, one launch, for three families that are the same linear update.
 *   'ancestral'    the posterior q(z_s | z_t, x_hat) of the reference's diffusion_reverse (gms/diffusion/diffusion_utils.py:34-62) with x_logvar
 *                  'small', 'large' (what gmk_sampler_step's noise path hard-codes) or 'medium:<frac>'
 *   'ddim_eta'     DDIM with eta in (0, 1] (Song, Meng & Ermon 2021, eq. 12 and 16); an extension, no reference call site
 *   'sde_dpmpp_2m' SDE-DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++", the SDE solver of its appendix); an extension, no reference call site
 * x_hat / eps_hat exactly as gmk_sampler_step forms them (v_uncond / cond_w: classifier-free guidance), or with thr (fp32 [B], nullable) as
 * gmk_sampler_step_dt forms them: one device function, the same bits.  Then, every operation singly rounded and nothing contracted,
 *     d      = coef_prev != 0 ? fsub(fmul(1 + coef_prev, x_hat), fmul(coef_prev, x_prev)) : x_hat
 *     z_next = is_last ? x_hat : fadd(fadd(fmul(coef_z, z), fmul(coef_x, d)), fmul(coef_noise, xi))
 * with the four coefficients from the host (gaussian_diffusion.stochastic_coefs, in double, rounded to fp32).  x_hist (nullable; required when
 * coef_prev != 0) holds x_prev, the previous step's x_hat, on entry - read only when coef_prev != 0 - and this step's x_hat on exit (same
 * element, same thread).  xi are Philox normals drawn in the kernel and never stored: element j of this chunk is element j of
 * gmk_rng_normal(seed, offset + q0), so rows [a, b) of a batch called with q0 = a n / 4 draw exactly what the whole batch would
 * (gmk_consistency_step's convention).  Nothing is drawn when is_last or when coef_noise == 0.  n % 4 == 0; times and coefficients finite;
 * coef_noise >= 0.  x_pred / eps_pred / z_dup / logsnr_next: gmk_sampler_step's conventions.  No floating-point atomics; no row of
 * GMK_KERNEL_TABLE. */
int gmk_stochastic_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float* x_hist, const float* thr,
                        float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_noise, float coef_prev, int is_last,
                        uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                        float* logsnr_next, int mean_type, int B, int64_t n, void* stream);

/* ---- a learned reverse-process variance (Nichol & Dhariwal 2021, "Improved Denoising Diffusion Probabilistic Models", section 3.1); extensions,
 * no reference call site.  The network's second head gives nu, fp32 [B][n] beside v; f_i = (nu_i + 1) / 2 (unclamped, as in the paper) is the
 * weight of diffusion_reverse's 'large' log-variance in its 'medium' interpolation, per element.
 * gmk_hybrid_loss: per image b with lt = logsnr[b], ls = logsnr_s[b] >= lt (the time one step of the bound's grid earlier),
 *   x_hat, eps_hat, x_mse, eps_mse, simple_b (by loss_type, mean_type) and dv: gmk_v_loss's, from the same device functions in the same order -
 *   x_mse, eps_mse and dv carry gmk_v_loss's bits for the same (v, z, x, eps, logsnr).
 *   D    = softplus(ls) - softplus(lt)                       (logvar_large - logvar_small)
 *   g    = -expm1(lt - ls) e^ls
 *   d_i  = x_hat_i - x_i                                     (the clipped prediction; the mean is a constant: stop-gradient)
 *   KL_i = (f_i D + expm1(-f_i D) + e^(-f_i D) g d_i^2) / 2  = normal_kl(q(z_s | z_t, x), p(z_s | z_t)) with diffusion_reverse's variances
 *   vlb_b[b] = mean_i KL_i (nats per dimension),  frac_b[b] = mean_i f_i,  loss_b[b] = simple_b + lambda vlb_b[b]
 *   dnu_i = grad_scale lambda / n  D / 4  (1 - e^(-f_i D) (1 + g d_i^2))        (dv, dnu: both or neither)
 * ls == lt gives KL = 0 and dnu = 0 from the formulas.  One workgroup per image; v, nu, z, x, eps are read once for images of up to
 * GMK_X_LOSS_KEEP values (larger ones read v, z, x, eps twice, nu once); 16-byte accesses when n % 4 == 0 and every tensor is 16-byte aligned,
 * scalar ones otherwise; any n.  lambda: finite, >= 0.  No floating-point atomics: the same call gives the same bits.  No row of GMK_KERNEL_TABLE. */
int gmk_hybrid_loss(const float* v, const float* nu, const float* z, const float* x, const float* eps, const float* logsnr,
                    const float* logsnr_s, float* loss_b, float* vlb_b, float* frac_b, float* x_mse, float* eps_mse, float* dv, float* dnu,
                    float grad_scale, float lambda, int loss_type, int mean_type, int B, int64_t n, void* stream);
/* gmk_stochastic_step for kind 'ancestral' (coef_prev = 0, no x_hist) with a noise multiplier per element:
 *     c_i    = fmul(coef_noise_small, exp(fmul(fmul(0.5, fadd(nu_i, 1)), half_delta)))
 *     z_next = is_last ? x_hat : fadd(fadd(fmul(coef_z, z), fmul(coef_x, x_hat)), fmul(c_i, xi))
 * coef_noise_small: the 'small' row of gaussian_diffusion.stochastic_row; half_delta = (softplus(ls) - softplus(lt)) / 2 >= 0, both from the host
 * in double, rounded to fp32.  nu: fp32 [B][n] (under guidance the conditional half's).  With nu = -1 everywhere z_next carries the bits of
 * gmk_stochastic_step under 'small'.  x_hat, thr, guidance, the Philox draw at (seed, offset + q0), is_last, x_pred / eps_pred / z_dup /
 * logsnr_next, n % 4 == 0: gmk_stochastic_step's.  No row of GMK_KERNEL_TABLE. */
int gmk_stochastic_step_lv(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* nu, const float* thr,
                           float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_noise_small, float half_delta, int is_last,
                           uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                           float* logsnr_next, int mean_type, int B, int64_t n, void* stream);
/* a[i] += b[i] (rounded once to dtype, GMK_F32 or GMK_BF16; n % 8 == 0, 16-byte aligned): the sum of the two heads' data gradients of a
 * learn_var network ahead of the last GroupNorm's backward. */
int gmk_add_into(void* a, const void* b, int64_t n, int dtype, void* stream);

/* ---- optimiser (torch.optim.Adam defaults as diffusion_model.py:56 uses it), flat fp32 arena ------------- */
int gmk_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, int step, float grad_scale, void* stream);
/* Adam exactly as gmk_adam_step (the same p, m, v bits), then an exponential moving average of the updated weights in the same pass:
 * ema = lerp(ema, p_new, ema_w), torch.lerp's formula (ema + ema_w (p_new - ema) for ema_w < 0.5, p_new - (p_new - ema)(1 - ema_w) above),
 * ema_w = 1 - decay in [0, 1].  No reference call site: the reference keeps no EMA of its weights (an extension, off by default in
 * DiffusionModel, DG.ema_decay).  ema: a second arena of n floats, same layout.  36 B / parameter against Adam's 28. */
int gmk_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                      float eps, int step, float grad_scale, float ema_w, void* stream);
/* Global L2 norm of the gradient arena and this step's decision, on the device (no host sync).  No reference call site for the clipping; the
 * guard is what GradScaler.step does in the reference's train step (diffusion_model.py:71).  Writes the four floats of `state`:
 *   [GMK_GRAD_NORM]  total_norm = grad_scale sqrt(sum g^2)                 the norm of the gradient Adam consumes
 *   [GMK_CLIP_COEF]  coef       = min(1, max_norm / (total_norm + 1e-6))   torch.nn.utils.clip_grad_norm_; max_norm <= 0: no clipping, 1
 *   [GMK_APPLY]      apply      = 1 if total_norm is finite, else 0        (an overflowing sum of squares counts as non-finite)
 *   [GMK_SKIPPED]    skipped    += 1 - apply                               a running count: zero it once, before the first call
 * Two launches: one partial sum of squares per workgroup into `workspace` (gmk_grad_norm_workspace_bytes(n) bytes; the grid depends on n
 * alone, not on gmk_set_cu_limit), then one workgroup adds the partials in a fixed order.  No atomics: the same bits on every call. */
#define GMK_GRAD_NORM 0
#define GMK_CLIP_COEF 1
#define GMK_APPLY 2
#define GMK_SKIPPED 3
int64_t gmk_grad_norm_workspace_bytes(int64_t n);
int gmk_grad_norm(const float* g, int64_t n, float grad_scale, float max_norm, float* workspace, int64_t workspace_bytes, float* state,
                  void* stream);
/* gmk_adam_step (ema NULL) or gmk_adam_ema_step steered by gmk_grad_norm's `state`: the gradient is (g grad_scale) coef - with coef = 1 the
 * bits of those two, with coef < 1 the bits of gmk_adam_step(grad_scale = 1) on a gradient pre-scaled the same way - and when apply is 0 the
 * launch returns before it touches p, m, v or ema. */
int gmk_adam_step_ctl(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2, float eps,
                      int step, float grad_scale, float ema_w, const float* state, void* stream);
/* The Adam step of gmk_adam_step (state NULL) or gmk_adam_step_ctl (state: gmk_grad_norm's record, same semantics: when apply is 0 the launch
 * returns before it touches any memory), then optionally the classic average (ema may be NULL; else gmk_adam_ema_step's bits), then n_pema
 * more averages of the updated weights, 1 <= n_pema <= 3: the rows of one fp32 [n_pema][pema_stride] arena,
 *     row_k = lerp(row_k, p_new, pw_k),   k < n_pema,   pw_k in [0, 1]   (pw_k with k >= n_pema is not read)
 * each row the bits gmk_adam_ema_step would write into it under ema_w = pw_k.  No reference call site: the power-function averages of Karras
 * et al. 2024 (post-hoc EMA), whose weights pw_k = 1 - (1 - 1/t)^(gamma_k + 1) come from the host every step (an extension, off by default,
 * DG.ema_sigma_rel).  pema_stride >= n; columns >= n of a row are never touched; rows take 16-byte accesses when pema is 16-byte aligned and
 * pema_stride % 4 == 0, scalar ones otherwise.  Everything is read once and written once: 28 + 8 (averages) B / parameter.  Any n.  No row of
 * GMK_KERNEL_TABLE. */
int gmk_adam_pema_step(float* p, const float* g, float* m, float* v, float* ema, float* pema, int64_t pema_stride, int n_pema, int64_t n,
                       float lr, float beta1, float beta2, float eps, int step, float grad_scale, float ema_w, float pw0, float pw1, float pw2,
                       const float* state, void* stream);
/* out[i] = fp32(sum_k coef[k] src[k][i]), i < n: src fp32 [K][src_stride] (src_stride >= n), coef K doubles on the device, 1 <= K <= 64.  In
 * double: acc = coef[0] row_0, then acc = acc + coef[k] row_k for k = 1 .. K - 1 in index order, every product and every sum rounded on its
 * own (no contraction), acc rounded once to fp32 - a function of the inputs alone, which a float64 loop on the host reproduces bit for bit.
 * out must not overlap src.  16-byte loads when src and out are 16-byte aligned and src_stride % 4 == 0, scalar ones otherwise and for the
 * n & 3 tail.  4 K + 4 B / element.  No reference call site: the reconstruction step of post-hoc EMA (posthoc_ema.py).  No row of
 * GMK_KERNEL_TABLE. */
int gmk_arena_combine(const float* src, int64_t src_stride, const double* coef, int K, float* out, int64_t n, void* stream);
/* 64-bit digest of a device buffer of n_words 4-byte words (no reference call site: checkpoint.py ties model.pt to train_state.pt with it,
 * compares data-parallel replicas and arenas without a host copy).  In uint64 arithmetic mod 2^64, w_i the raw bits of word i (from 0):
 *   digest = sum_i mix(w_i + (i + 1) 0x9E3779B97F4A7C15),   mix = splitmix64's finaliser (x ^= x >> 30; x *= 0xBF58476D1CE4E5B9;
 *                                                           x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31)
 * The sum is exact and commutative: the value does not depend on the launch shape (a function of n_words alone, not of gmk_set_cu_limit).
 * data: 4-byte aligned (16-byte loads from the first 16-byte boundary on); out: one uint64 on the device, zeroed by this entry on `stream`
 * and then added to by one 64-bit atomic per workgroup. */
int gmk_arena_digest(const void* data, int64_t n_words, uint64_t* out, void* stream);

/* ---- exact nearest neighbours of byte rows (no reference call site: neighbours.py's report of samples beside their nearest training images) ----
 * d2(q, j) = sum_i (queries[q][i] - database[j][i])^2, an exact integer.  Row q of dist2_out / index_out holds the k smallest pairs (d2, j) in
 * lexicographic order: the smaller distance first and, among equal distances, the smaller index (identical database rows come lowest index
 * first).  A function of the inputs alone - integer arithmetic, no atomics, no merge that depends on an order of arrival: two calls give the
 * same bytes.
 *   queries [Q][D] uint8, database [N][D] uint8, row-contiguous, any alignment (D % 16 == 0 on 16-byte aligned bases takes 16-byte loads,
 *   everything else a per-byte staging path);  db_sqnorm [N] int32 = gmk_u8_sqnorm(database), so that a caller can keep it per dataset;
 *   dist2_out, index_out [Q][k] int32;  workspace: gmk_nn_search_workspace(Q, N, k) bytes, 16-byte aligned (-1 for arguments out of range)
 *   1 <= k <= GMK_NN_MAX_K and k <= N;  1 <= Q, N < 2^31;  1 <= D <= GMK_NN_MAX_D - there d2 <= 32768 * 255^2 = 2 130 739 200 < 2^31.
 * Bytes are taken as b ^ 0x80 = b - 128 (the differences do not change) and d2 = |q'|^2 + |x'|^2 - 2 q'.x' with the dot product on
 * v_mfma_i32_32x32x32_i8 (int32 accumulation, |q'.x'| <= 2^29: exact).  Three launches: the queries' norms, one workgroup per GMK_NN_SLAB
 * database rows that loops over the query tiles and leaves two lists of k keys (d2 << 32 | j) per query and slab in the workspace, and a
 * merge of those lists per query (csrc/nn_search.hip).  The database is read from HBM once per call.
 * gmk_u8_sqnorm: out[j] = sum_i (rows[j][i] - 128)^2 as int32 (<= 2^29), the same ranges of N and D.  No rows of GMK_KERNEL_TABLE. */
#define GMK_NN_SLAB 128
#define GMK_NN_MAX_K 8
#define GMK_NN_MAX_D 32768
int gmk_u8_sqnorm(const uint8_t* rows, int64_t N, int D, int* out, void* stream);
int64_t gmk_nn_search_workspace(int64_t Q, int64_t N, int k);
int gmk_nn_search_u8(const uint8_t* queries, int64_t Q, const uint8_t* database, int64_t N, int D, const int* db_sqnorm, int k,
                     void* workspace, int64_t workspace_bytes, int* dist2_out, int* index_out, void* stream);

/* ---- k-NN radii and ball counts of fp32 rows (no reference call site: metrics.manifold_metrics, the heavy evaluation at a sample count
 * where the reference's two N x N cdist matrices no longer fit) ----
 * Both entries use one squared distance of two rows a, b of D floats:  acc = 0;  for i = 0 .. D - 1: t = a[i] - b[i]; acc = fmaf(t, t, acc)
 * - one fp32 chain in ascending i, a function of the two rows alone (not of the launch shape, gmk_set_cu_limit, or which row is the query):
 * d2(a, b) == d2(b, a) bit for bit, d2(a, a) == 0, and both kernels give the same bits for the same pair.
 *   gmk_knn_radius_f32   r2_out[i] = the (k + 1)-th smallest VALUE of the multiset {d2(pts[i], pts[j]) : j = 0 .. N - 1} (j = i, value 0,
 *                        included): topk(cdist(a, a), k + 1, largest=False)[..., -1] squared.  1 <= k <= GMK_NN_MAX_K, k + 1 <= N < 2^31,
 *                        1 <= D <= GMK_KNN_MAX_D.  workspace: gmk_knn_radius_workspace(N, k) bytes (-1 for arguments out of range), 4-byte
 *                        aligned.  One workgroup per (row tile of GMK_KNN_TILE, slab of GMK_KNN_SLAB columns) leaves the k + 1 smallest
 *                        values per row and slab in the workspace ([slab][k + 1][N] floats), one thread per row merges them.  No atomics:
 *                        two calls give the same bytes.
 *   gmk_ball_counts_f32  q_count[q] = #{j : d2(queries[q], balls[j]) < r2[j]} (strict), m_count[j] = #{q : the same predicate}; either
 *                        may be null.  Both are zeroed by this entry on `stream`, then filled with int32 atomic adds (exact, commutative:
 *                        a function of the inputs).  1 <= M, Q < 2^31.
 * Rows are contiguous, 4-byte aligned (16-byte loads when every base is 16-byte aligned and D % 4 == 0).  csrc/knn_f32.hip.  No rows of
 * GMK_KERNEL_TABLE. */
#define GMK_KNN_TILE 64
#define GMK_KNN_SLAB 1024
#define GMK_KNN_MAX_D 4096
int64_t gmk_knn_radius_workspace(int64_t N, int k);
int gmk_knn_radius_f32(const float* pts, int64_t N, int D, int k, void* workspace, int64_t workspace_bytes, float* r2_out, void* stream);
int gmk_ball_counts_f32(const float* balls, const float* r2, int64_t M, const float* queries, int64_t Q, int D,
                        int* q_count, int* m_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GMK_H */
