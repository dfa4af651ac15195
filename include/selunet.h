/*
 * selunet.h — C-ABI of the MI355X (gfx950) SelectiveUNet_B training path.
 *
 * The reference has no FFI: its boundary is the Python API of `model.UNet_B`
 * (model.py:18-103), `selective_loss.calc_selective_risk_image_b`
 * (selective_loss.py:58-85), `torch.nn.BCEWithLogitsLoss` (train.py:78,195) and
 * `torch.optim.Adam` (train.py:90,209). Every ATen op those dispatch to on the
 * hot path is replaced by one of the entry points below; the Python host layer
 * (selectivenet_for_semantic_segmentation_binary_amd/) binds them with ctypes and
 * keeps the reference's module/function signatures. Each entry point notes the
 * reference call it replaces.
 *
 * Conventions
 *  - Plain device pointers, sizes and a `hipStream_t` passed as `void*` (the
 *    caller's current stream). No allocation, no synchronisation, no host copies
 *    inside any call: all workspaces are caller-owned, so every call is graph-
 *    capturable.
 *  - Activations are NHWC (channels contiguous), element type `dtype`
 *    (SELUNET_F32 or SELUNET_BF16); statistics, losses, weight gradients and
 *    optimizer state are fp32 (reductions fp64 where noted).
 *  - Return 0 on success, otherwise a nonzero code; `selunet_last_error()` gives
 *    the message of the last failing call on this thread.
 */
#ifndef SELUNET_H
#define SELUNET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SELUNET_F32 = 0, SELUNET_BF16 = 1 };

enum {
  SELUNET_OK = 0,
  SELUNET_EINVAL = 1,  /* bad argument (null pointer, size, alignment, unsupported shape) */
  SELUNET_ELAUNCH = 2, /* HIP launch error */
};

/* Kernel-selection and tuning options (selunet_set_option). The library reads no environment
 * variables; every value < 0 selects the built-in default. Selection options take 0/1. */
enum {
  SELUNET_OPT_HALO = 0,           /* 3x3 convolutions on the LDS halo kernels (1) or the gather GEMM (0) */
  SELUNET_OPT_HALO_PERSIST,       /* persistent halo kernel for multi-chunk layers: 0 off, 1 on (1) */
  SELUNET_OPT_WINO,               /* exact-fp32 3x3 fwd/dgrad as 1-D Winograd F(2,3) (1) or direct (0) */
  SELUNET_OPT_WINO_WGRAD,         /* exact-fp32 3x3 weight gradient as the Winograd transpose (1) */
  SELUNET_OPT_WINO_WGRAD_TW,      /* its tile width: 16 (default) or 8 pixels */
  SELUNET_OPT_WINO_WGRAD_WAVES,   /* its waves per workgroup: 12 (default) or 8 */
  SELUNET_OPT_WGRAD_WGS,          /* workgroup target of the halo / Winograd weight gradients (256) */
  SELUNET_OPT_X2_WGRAD_WGS,       /* workgroup target of the split-fp16 3x3 weight gradient (256) */
  SELUNET_OPT_GEMM_WGRAD_WGS,     /* workgroup target of the generic weight gradient (512) */
  SELUNET_OPT_GATHER_WGS,         /* resident gather-GEMM workgroups (512; 0 = one tile each) */
  SELUNET_OPT_RF_SINGLE,          /* slab rows reduced in one launch by the fused reductions (1024) */
  SELUNET_OPT_APPLY_U8,           /* BN-backward apply form: 0 8 ch x 4 px, 1 8 ch x 8 px, 2/3 4 contiguous ch x 8/16 px (0) */
  SELUNET_OPT_APPLY_GRID,         /* BN-backward apply: grid cap (1024) */
  SELUNET_OPT_X2D,                /* 64-column split-fp16 3x3 layers on the two-workgroups-per-CU kernel: 0 never,
                                   * 1 every eligible layer, 2 inputs of at most 64 channels, 3 (default) those of
                                   * them whose source carries a BN+ReLU transform (the forwards) */
  SELUNET_OPT_TILE_QUEUE,         /* bit mask (robustness to a concurrent all-reduce), 0 = static walks
                                   * (default). Bit 0: the split-fp16 persistent 3x3 kernel takes its pixel tiles from
                                   * a ticket counter and writes statistics per tile (selunet_conv3x3_x2_stats_rows
                                   * follows it). Bit 1: so do the split-fp16 weight gradients' (co tile, ci chunk)
                                   * groups (each partial then sums the tiles its workgroup took: the weight gradient
                                   * is not bit-reproducible run to run) */
  SELUNET_OPT_X2P,                /* 128-column split-fp16 3x3 layers (multi-chunk inputs) on the kernel with two
                                   * 256-thread workgroups per CU and LDS-DMA weights (1) or on the
                                   * one-workgroup-per-CU persistent kernel (0, default: measured faster);
                                   * selunet_conv3x3_x2_stats_rows follows it */
  SELUNET_OPT_CONVT_RING,         /* ConvTranspose2d forward / data gradient on 256-column blocks (fp32: K >= 256;
                                   * bf16: K >= 512): the LDS-DMA ring kernels with the forward on 8 x 1 waves (2,
                                   * default) or, fp32, 4 x 2 waves (1), or the resident-weight / staged kernels (0);
                                   * selunet_gemm_gather_x2_stats_rows / selunet_gemm_stats_rows follow it */
  SELUNET_OPT_IO_GRID,            /* grid-stride I/O, metrics and prediction launches: upper bound on the workgroup
                                   * count; default each launcher's own cap. For tests and small inputs: the kernels'
                                   * per-workgroup 32-bit partial counts are sized for the default grids (a small grid
                                   * on more than 2^30 pixels can overflow them), and a value above a launcher's own cap
                                   * raises that cap */
  SELUNET_OPT_COUNT
};
/* Sets option `key` to `value` (< 0: default); returns the previous setting, or INT64_MIN for an
 * unknown key. Changes apply to later calls (the stats-slab row counts of selunet_gemm_stats_rows
 * follow SELUNET_OPT_HALO_PERSIST / GATHER_WGS). Not thread-safe; set before enqueuing work. */
int64_t selunet_set_option(int32_t key, int64_t value);

/* Rows of the GEMM output tile (pixels per workgroup); stats slabs have ceil(M/128) rows. */
#define SELUNET_GEMM_BM 128

/* One source tensor of an implicit-GEMM operand. The transform
 * v -> relu?(v*scale[c] + shift[c]) is the folded BatchNorm of the producing
 * CBR block (model.py:12-13), applied on load; padded positions read 0 after it. */
typedef struct selunet_source {
  const void* data;    /* NHWC [n][hs][ws][channels] (layout 0) or NCHW fp32 (layout 1) */
  const float* scale;  /* per-channel, NULL = identity */
  const float* shift;
  int32_t channels;
  int32_t relu;        /* clamp at 0 after the affine */
  int32_t layout;      /* 0 NHWC, 1 NCHW (network input only, fp32) */
  int32_t reserved;
} selunet_source;

/* A gathered ("im2col without materialisation") matrix G[M][K]:
 *   row m = (img*h + y)*w + x over an n x h x w pixel grid,
 *   column k = tap*(C0+C1) + c, c < C0 from src[0] else src[1] (torch.cat((up, skip), 1),
 *   model.py:83,87,91). taps: 1 = the pixel itself; 9 = 3x3 neighbourhood, zero padded
 *   (conv 3x3 pad 1, model.py:11); 4 = the 2x2 block (2y+a, 2x+b) of a (2h)x(2w) source grid
 *   (ConvTranspose2d k2 s2 backward, model.py:44,51,57). */
typedef struct selunet_gather {
  int32_t n, h, w;
  int32_t taps;
  int32_t nsrc;
  int32_t reserved;
  selunet_source src[2];
} selunet_gather;

enum { SELUNET_EP_PLAIN = 0, SELUNET_EP_SPLIT = 1, SELUNET_EP_SCATTER2X = 2 };

/* Epilogue of selunet_gemm_gather. PLAIN: out0[M][N]; SPLIT: columns < split go to
 * out0[M][split], the rest to out1[M][N-split] (backward of torch.cat); SCATTER2X:
 * column (a*2+b)*Cq + c of row (img,y,x) goes to out0[img][2y+a][2x+b][c], Cq = N/4
 * (ConvTranspose2d k2 s2 forward). bias (fp32, per output channel) is added when
 * non-NULL. stats (fp32 [selunet_gemm_stats_rows(a, N, dtype)][2][N]): per-workgroup column
 * sum and sum of squares of the fp32 accumulators (BatchNorm batch statistics, model.py:12). */
/* BatchNorm-backward partial sums of a freshly written data gradient dA of a CBR block (fused into
 * the kernel that produces dA instead of re-reading it): per workgroup and channel,
 * sum(da), sum(da*xhat), sum(xhat) with da = dA*[y*scale+shift > 0], xhat = (y-mean)*invstd,
 * dA rounded to the activation dtype first (as stored). slab = NULL disables it. */
typedef struct selunet_bn_bwd_stats {
  const void* y;       /* the block's pre-BN conv output, same [M][C] layout as dA */
  const float* scale;  /* folded BN + ReLU of the forward pass */
  const float* shift;
  const float* mean;   /* batch statistics of the forward pass */
  const float* invstd;
  float* slab;         /* [rows][3][C] */
  float* amax;         /* nullable: atomic max of |dA| as stored (float bits; zeroed by the caller) — read by
                        * selunet_maxpool2_bwd and selunet_heads_bwd only, whose sums-only mode never stores
                        * dA: the range word selunet_bn_bwd_stats_finalize_bound needs for a fused apply */
} selunet_bn_bwd_stats;

typedef struct selunet_epilogue {
  void* out0;
  void* out1;
  const float* bias;
  float* stats;
  int32_t mode;
  int32_t split;
  /* SPLIT only (nullable): [stats_rows][split] per-workgroup column sums of the out0 part (the
   * ConvTranspose2d bias gradient of the up-sampled half of a torch.cat, model.py:44,51,57). */
  float* colsum;
  /* PLAIN only: BatchNorm-backward sums of the written tile, slab [stats_rows][3][N]. */
  selunet_bn_bwd_stats bnb;
  /* nullable: max |stored value| folded into *amax with an atomic max (float bits; the caller zeroes
   * it): the range word of a split-fp16 operand (selunet_conv3x3_x2) read by the next layer. */
  float* amax;
  /* nullable, with stats: per-column shift c (the previous step's batch mean): stats then hold the sums
   * of (v - c) and (v - c)^2, which selunet_bn_stats_finalize_shifted turns into the mean and a
   * one-pass variance that loses ~eps * (mean - c)^2 / var instead of ~eps * mean^2 / var. */
  const float* stats_center;
} selunet_epilogue;

const char* selunet_last_error(void);
int32_t selunet_version(void);
/* Fingerprint (SHA-256 prefix) of the kernel sources, headers and flags this library was built from. */
const char* selunet_build_id(void);

/* ---- weight repacking (fp32 master weights -> GEMM operands, dtype) ---------------- */
/* conv3x3 weight [co][ci][3][3] -> fwd [co][k_pad] (k = tap*ci + c, zero pad to k_pad) and,
 * if dgrad != NULL, dgrad [ci][9*co] with the taps flipped (k = tap*co + o). */
int selunet_pack_conv3x3(const float* w, int32_t co, int32_t ci, int32_t k_pad, void* fwd,
                         void* dgrad, int32_t dtype, void* stream);
/* ConvTranspose2d weight [ci][co][2][2] -> fwd [4*co][ci] (row (a*2+b)*co+o) and
 * dgrad [ci][4*co]. */
int selunet_pack_convT(const float* w, int32_t ci, int32_t co, void* fwd, void* dgrad,
                       int32_t dtype, void* stream);
/* packed fp32 grads -> reference layouts (accumulated into out when accumulate != 0) */
int selunet_unpack_conv3x3_grad(const float* packed, int32_t co, int32_t ci, int32_t k_pad,
                                float* out, void* stream);
int selunet_unpack_convT_grad(const float* packed, int32_t ci, int32_t co, float* out, void* stream);

/* ---- implicit GEMMs (MFMA) ------------------------------------------------------------ */
/* out = G_a[M][K] * B^T, B = [n_cols][k_pad] in dtype. Replaces conv2d 3x3 forward and
 * data-gradient, conv_transpose2d forward and data-gradient (model.py:11,44,51,57). */
int selunet_gemm_gather(const selunet_gather* a, const void* b, int32_t n_cols, int32_t k_pad,
                        const selunet_epilogue* ep, int32_t dtype, void* stream);
/* fp32 3x3 conv forward / data gradient (model.py:11; the reference's conv2d and its input
 * gradient) as a 1-D Winograd F(2,3) along x: per output pair and kernel row, four fp32 MFMA passes
 * over transformed operands (V = d0-d2, d1+d2, d2-d1, d1-d3; U = g0, (g0+g1+g2)/2, (g0-g1+g2)/2,
 * g2) instead of six direct ones. u = [n_cols][12*C] (k = (dy*4 + xi)*C + c), written by
 * selunet_pack_weights with kind SELUNET_PACK_CONV3X3_WINO. Same operands, epilogues and
 * statistics slab rows (selunet_gemm_stats_rows) as selunet_gemm_gather on the same 3x3 gather;
 * selunet_conv3x3_wino_ok tells from the shapes whether a layer can take it (fp32 multi-chunk
 * halo layers: h, w >= 16, w even, C a multiple of 32 and > 32, n_cols a multiple of 64). */
int32_t selunet_conv3x3_wino_ok(int32_t h, int32_t w, int32_t c_in, int32_t c_src0, int32_t n_cols);
int selunet_conv3x3_wino(const selunet_gather* a, const float* u, int32_t n_cols,
                         const selunet_epilogue* ep, void* stream);
const char* selunet_conv3x3_wino_kernel_name(int32_t n_cols, int32_t mode, int32_t split);
/* fp32 3x3 conv forward / data gradient (model.py:11 and its input gradient) on the fp16 matrix
 * cores: each fp32 operand is split into two fp16 parts, v*2^e = h + l (22 significant bits,
 * 2^e a power of two that keeps the operand below 2^14), and every product is summed as
 * h_a*h_b + h_a*l_b + l_a*h_b in fp32 accumulators (three v_mfma_f32_32x32x16_f16 per 16-channel
 * step; the dropped l_a*l_b is below 2^-22 of the product). Measured relative RMS error against
 * fp64 at K = 576..4608 is at or below the exact fp32 MFMA's (tools/split_probe.hip). Operand
 * ranges: amax0 / amax1 (device words, amax1 only for a two-source gather) bound |source value
 * after its BN+ReLU transform|. A BN+ReLU source has two producers: selunet_act_bound (or its fold
 * into selunet_bn_stats_finalize_centered_bound) when scale / shift come from this batch's statistics
 * (training: the Samuelson bound, a function of gamma, beta and the count alone), and selunet_act_amax,
 * the exact maximum taken from the data, when they do not (eval mode, running statistics: nothing
 * bounds the normalized value a priori). Any other source: the producing kernel's atomic max
 * (selunet_epilogue.amax, selunet_bn_bwd_apply). w: a
 * SELUNET_PACK_CONV3X3_X2 pack ([n_cols][9*C] + n_cols row unscale factors). Same gathers,
 * epilogues and statistics slab rows as selunet_gemm_gather; selunet_conv3x3_x2_ok tells whether a
 * layer can take it (h, w >= 16, C and c_src0 multiples of 32, C > 32, n_cols a multiple of 64). */
/* selunet_gemm_gather on split-fp16 operands (ConvTranspose2d forward / data gradient in fp32 training,
 * model.py:44,51,57): w a split-fp16 pack (SELUNET_PACK_CONVT_X2 rows, k_pad == K, K a multiple of 32),
 * amax0 / amax1 the sources' range words; any gather taps and epilogue of selunet_gemm_gather. Its
 * statistics slabs have selunet_gemm_gather_x2_stats_rows rows (256-row persistent tiles). */
int selunet_gemm_gather_x2(const selunet_gather* a, const float* w, int32_t n_cols, int32_t k_pad,
                           const selunet_epilogue* ep, const float* amax0, const float* amax1, void* stream);
int64_t selunet_gemm_gather_x2_stats_rows(const selunet_gather* a, int32_t n_cols);
/* selunet_gemm_wgrad_ws_to on split-fp16 operands (the ConvTranspose2d weight gradient in fp32 training,
 * layout SELUNET WG_CONVT = 2, or a Conv2d one, layout 1): vector gathers, K_p and K_q multiples of 64;
 * amax_p0/p1, amax_q0/q1 the sources' range words (p1 / q1 only for two-source gathers). Partials in
 * ws (>= selunet_gemm_wgrad_x2_ws_bytes), summed in a fixed order into out. */
int64_t selunet_gemm_wgrad_x2_ws_bytes(const selunet_gather* p, const selunet_gather* q);
int selunet_gemm_wgrad_x2(const selunet_gather* p, const selunet_gather* q, float* ws, int64_t ws_bytes, int32_t layout,
                          float* out, const float* amax_p0, const float* amax_p1, const float* amax_q0,
                          const float* amax_q1, void* stream);
int32_t selunet_conv3x3_x2_ok(int32_t h, int32_t w, int32_t c_in, int32_t c_src0, int32_t n_cols);
/* fp32 3x3 weight gradient (autograd of model.py:11's weight) on split-fp16 operands, the same
 * arithmetic as selunet_conv3x3_x2: p = dY (1 tap, [M][co]), q = the layer input (3x3 gather, BN+ReLU
 * transforms of its sources); amax_p / amax_q0 / amax_q1 their range words. Pixel-split partials in
 * ws (>= selunet_conv3x3_wgrad_x2_ws_bytes) are summed in a fixed order straight into out, the
 * Conv2d weight layout [co][ci][3][3] (deterministic). -1 bytes: operands not eligible (q: h >= 8,
 * w >= 16, channels multiples of 64; co a multiple of 64). */
int64_t selunet_conv3x3_wgrad_x2_ws_bytes(const selunet_gather* p, const selunet_gather* q);
int selunet_conv3x3_wgrad_x2(const selunet_gather* p, const selunet_gather* q, float* ws, int64_t ws_bytes,
                             float* out, const float* amax_p, const float* amax_q0, const float* amax_q1,
                             void* stream);
/* selunet_conv3x3_wgrad_x2 with the layer's BN-backward apply fused into its dY staging (replaces
 * selunet_bn_bwd_apply_amax + selunet_conv3x3_wgrad_x2; model.py:12-13's backward): p gathers dA (one
 * source, no transform), bnb the forward's y / scale / shift / mean / invstd (slab unused), coef the
 * [3][C] coefficients of selunet_bn_bwd_stats_finalize; the kernel forms
 * dy = (y*scale+shift > 0 ? k0*dA : 0) - k1 - k2*invstd*(y - mean) exactly as selunet_bn_bwd_apply,
 * stages it split-fp16 with the range word amax_p (an upper bound of |dy|:
 * selunet_bn_bwd_stats_finalize_bound), and writes dy [M][C] (fp32, nullable) with its exact max |dy|
 * into *dy_amax (atomic max; zeroed by the caller) for the layer's data gradient. */
int selunet_conv3x3_wgrad_x2_bn(const selunet_gather* p, const selunet_gather* q, float* ws, int64_t ws_bytes,
                                float* out, const float* amax_p, const float* amax_q0, const float* amax_q1,
                                const selunet_bn_bwd_stats* bnb, const float* coef, float* dy, float* dy_amax,
                                void* stream);
/* Where selunet_conv3x3_wgrad_x2_bn_src's dY staging takes dA from. TENSOR: p's source (as
 * selunet_conv3x3_wgrad_x2_bn). POOL: the layer feeds a 2x2 max-pool (model.py:30,60-61's encoder
 * blocks): dA = route(pooled) + skip, pooled [n][h/2][w/2][C] the pool output's gradient routed to
 * the first maximum of relu(y*scale+shift) in row-major window order, skip [M][C] (nullable) added to
 * every pixel — selunet_bn_bwd_apply_pool's dA. HEADS: the layer feeds the 1x1 heads (model.py:62-66):
 * dA[m][c] = sum_h head_w[h][c] * g[h][m] over nh = 1 or 3 heads, C = 64 — selunet_bn_bwd_apply_heads's
 * dA. For POOL / HEADS p only gives the grid and C (its data is not read) and C must be 64. */
enum { SELUNET_DA_TENSOR = 0, SELUNET_DA_POOL = 1, SELUNET_DA_HEADS = 2 };
typedef struct selunet_da_source {
  int32_t kind;
  int32_t nh;
  const float* pooled;
  const float* skip;
  const float* head_w;
  const float* g[3];
} selunet_da_source;
/* selunet_conv3x3_wgrad_x2_bn with dA formed from `src` (NULL: TENSOR): the fused pool / heads applies
 * (selunet_bn_bwd_apply_pool / _heads) move into the weight gradient's staging like the plain one. */
int selunet_conv3x3_wgrad_x2_bn_src(const selunet_gather* p, const selunet_gather* q, float* ws, int64_t ws_bytes,
                                    float* out, const float* amax_p, const float* amax_q0, const float* amax_q1,
                                    const selunet_bn_bwd_stats* bnb, const float* coef, const selunet_da_source* src,
                                    float* dy, float* dy_amax, void* stream);
int selunet_conv3x3_x2(const selunet_gather* a, const float* w, int32_t n_cols, const selunet_epilogue* ep,
                       const float* amax0, const float* amax1, void* stream);
const char* selunet_conv3x3_x2_kernel_name(const selunet_gather* a, int32_t n_cols, int32_t mode, int32_t split);
/* Statistics slab rows (stats / colsum / BN-backward sums of the epilogue) selunet_conv3x3_x2
 * writes for this operand: the layers SELUNET_OPT_X2D sends to the 64-column kernel
 * with two 256-thread workgroups per CU have min(16x16 tiles, 512) rows; the 128-column layers
 * under SELUNET_OPT_X2P min(16x16 tiles, 512 / column tiles); under SELUNET_OPT_TILE_QUEUE bit 0
 * the others have one row per 16x16 tile, else as selunet_gemm_stats_rows.
 * selunet_conv3x3_x2_kernel_name names the kernel a call would run. */
int64_t selunet_conv3x3_x2_stats_rows(const selunet_gather* a, int32_t n_cols);
/* Range word of a training-mode BatchNorm+ReLU output relu(gamma*xhat + beta) over `count` values
 * per channel: |xhat| <= sqrt(count - 1) for batch statistics (Samuelson's inequality), so
 * *out = max_c |gamma_c| * sqrt(count) + max_c |beta_c| bounds every element (max-pooled copies
 * included). One block; c <= 4096. */
int selunet_act_bound(const float* gamma, const float* beta, int32_t c, int64_t count, float* out, void* stream);
/* Exact range word of a BN+ReLU source whose (scale, shift) do not come from batch statistics (eval mode):
 * atomic max (float bits; zeroed by the caller) over [m][c] of relu(y*scale_c + shift_c), the value the
 * consumers' loaders stage. fp32 y, c a multiple of 4. One pass over y (m*c*4 bytes), no workspace. */
int selunet_act_amax(const float* y, int64_t m, int32_t c, const float* scale, const float* shift,
                     float* amax, void* stream);
/* Rows of the stats slab selunet_gemm_gather writes for this operand (workgroup rows of the
 * kernel it dispatches to: 16x16 halo tiles for single-chunk 3x3 operands, the persistent
 * workgroups of the multi-chunk halo kernel, else 128-row tiles); -1 on error. */
int64_t selunet_gemm_stats_rows(const selunet_gather* a, int32_t n_cols, int32_t dtype);
/* Tuning/testing knob: workgroups the persistent multi-chunk 3x3 kernel targets (default 256, one
 * per MI355X CU; wgs <= 0 restores the default). Returns the previous value. The stats-slab row
 * count depends on it: query selunet_gemm_stats_rows after changing it. Not thread-safe. */
int32_t selunet_set_halo_workgroups(int32_t wgs);
/* Tuning/testing knob: workgroups the persistent generic gather GEMM (ConvTranspose2d forward and
 * data gradient, 3x3 layers the halo kernels do not take) targets: default 512 (two per CU), 0 = one
 * output tile per workgroup, < 0 restores the default. Returns the previous value. Changes the
 * stats-slab row count like selunet_set_halo_workgroups. Not thread-safe. */
int32_t selunet_set_gather_workgroups(int32_t wgs);
/* Name of the kernel a selunet_gemm_gather (q == NULL; mode = epilogue mode) or
 * selunet_gemm_wgrad (q = the Q operand) call with these operands dispatches to. */
const char* selunet_gemm_kernel_name(const selunet_gather* a, const selunet_gather* q, int32_t n_cols,
                                     int32_t mode, int32_t dtype);
/* out[ni][nj] += sum_m G_p[m][i] * G_q[m][j] (fp32 atomics; out zeroed by the caller).
 * Replaces the weight-gradient of conv2d / conv_transpose2d (train.py:208 backward). */
int selunet_gemm_wgrad(const selunet_gather* p, const selunet_gather* q, float* out,
                       int32_t dtype, void* stream);
/* Deterministic variant: the pixel splits write their partial sums to the workspace `ws`
 * (selunet_gemm_wgrad_ws_bytes bytes; fp32 [splits][ni][ld]) and a reduction kernel sums them in
 * a fixed order into out, which is overwritten (no zeroing needed; pad columns become 0). Operands
 * without a split-partials path (fp32) report 0 bytes; out is then zeroed and accumulated with
 * atomics inside the call. Removes the fp32 atomic traffic (~150 MB per 3x3 layer) of
 * selunet_gemm_wgrad. */
int64_t selunet_gemm_wgrad_ws_bytes(const selunet_gather* p, const selunet_gather* q, int32_t dtype);
int selunet_gemm_wgrad_ws(const selunet_gather* p, const selunet_gather* q, float* out, float* ws,
                          int64_t ws_bytes, int32_t dtype, void* stream);
/* selunet_gemm_wgrad_ws with the result written in the reference parameter layout by the split
 * reduction itself: layout 1 = Conv2d weight [co][ci][3][3] (P = dY, Q = the 3x3 input taps),
 * layout 2 = ConvTranspose2d weight [ci][co][2][2] (P = the input, Q = the 4 output taps) — the
 * .grad of model.py:11 / model.py:44,51,57 weights. `packed` ([ni][selunet_wgrad_ld] fp32) is
 * scratch used only by operands without a split-partials path (may be NULL otherwise). */
int selunet_gemm_wgrad_ws_to(const selunet_gather* p, const selunet_gather* q, float* packed,
                             float* ws, int64_t ws_bytes, int32_t layout, float* out, int32_t dtype,
                             void* stream);
/* Row stride of the packed wgrad output for a Q operand with kq columns (kq rounded up to
 * the column tile); `out` must be [ni][selunet_wgrad_ld(kq)], the pad columns are garbage-free
 * zeros when out was zeroed. */
int32_t selunet_wgrad_ld(int32_t kq);

/* Every weight pack of a step in one launch: conv3x3 entries as selunet_pack_conv3x3 (fwd
 * required, dgrad optional), ConvTranspose2d entries as selunet_pack_convT (w [ci][co][2][2]).
 * `offset` is computed by the call. Replaces the per-tensor loop over model.py's conv/unpool
 * parameters (model.py:11,44,51,57) that casting fp32 masters to the compute operands needs. */
#define SELUNET_PACK_MAX 32
/* SELUNET_PACK_CONV3X3_WINO (fp32): fwd = [co][12*ci] and dgrad = [ci][12*co] Winograd weight
 * operands of selunet_conv3x3_wino (k_pad = 12*ci; dgrad from the flipped/transposed kernel). */
/* SELUNET_PACK_CONV3X3_X2 (fp32): split-fp16 operands of selunet_conv3x3_x2, k_pad = 9*ci; fwd =
 * [co][9*ci] and dgrad = [ci][9*co] 32-bit words (taps flipped), each row scaled by 2^e_row
 * (max|w_row| * 2^e_row < 2^14) and every 32-k group (one tap, 32 channels) stored as 32 fp16 high
 * parts h = fp16(v) then 32 low parts l = fp16(v - h); the row unscale factors 2^-e_row follow the
 * matrix: fwd + co*9*ci (co floats), dgrad + ci*9*co (ci floats). ci, co multiples of 32. */
/* SELUNET_PACK_CONVT_X2 (fp32): the same split-fp16 format for a ConvTranspose2d weight [ci][co][2][2]:
 * fwd = [4*co][ci] (row (a*2+b)*co + o, k_pad = ci) + 4*co unscale factors, dgrad = [ci][4*co] + ci. */
/* SELUNET_PACK_COPY (any dtype): co*ci fp32 values w -> fwd unchanged (dgrad unused) — the heads'
 * current weights and biases (model.py:62,65,66) gathered into the contiguous [heads][64] / [heads]
 * operands of selunet_heads_fwd in the same launch. */
enum {
  SELUNET_PACK_CONV3X3 = 0,
  SELUNET_PACK_CONVT = 1,
  SELUNET_PACK_CONV3X3_WINO = 2,
  SELUNET_PACK_CONV3X3_X2 = 3,
  SELUNET_PACK_CONVT_X2 = 4,
  SELUNET_PACK_COPY = 5
};
typedef struct selunet_pack_desc {
  const float* w;
  void* fwd;
  void* dgrad;
  int32_t kind, co, ci, k_pad;
  int64_t offset;
} selunet_pack_desc;
typedef struct selunet_pack_list {
  int32_t n, _pad;
  selunet_pack_desc d[SELUNET_PACK_MAX];
} selunet_pack_list;
int selunet_pack_weights(const selunet_pack_list* list, int32_t dtype, void* stream);

/* ---- reductions ----------------------------------------------------------------------- */
/* out[c] = sum_r slab[r][c] in fp64, deterministic order, written as fp64 (out) and/or fp32
 * (out32), either may be NULL; ws: >= selunet_reduce_ws_bytes(cols). */
int64_t selunet_reduce_ws_bytes(int32_t cols);
int selunet_reduce_rows(const float* slab, int64_t rows, int32_t cols, double* ws, double* out,
                        float* out32, void* stream);
/* per-channel sums of an NHWC tensor: slab [selunet_channel_slab_rows(M)][C] */
int64_t selunet_channel_slab_rows(int64_t m);
int selunet_channel_sum(const void* x, int64_t m, int32_t c, float* slab, int32_t dtype, void* stream);

/* ---- BatchNorm2d (model.py:12; eps 1e-5, momentum 0.1) ------------------------------- */
/* From fp64 sums [2][C] (sum, sumsq of conv output without bias) over `count` pixels:
 * training: mean/invstd of the batch, running stats updated (unbiased var), *num_batches += 1;
 * eval (training == 0): running stats. Writes mean (of conv output w/o bias), invstd, and the
 * folded scale = gamma*invstd, shift = beta - mean*scale used by consumers' loaders. */
int selunet_bn_finalize(const double* sums, int64_t count, int32_t c, const float* conv_bias,
                        const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int64_t* num_batches, float momentum, float eps,
                        int32_t training, float* mean, float* invstd, float* scale, float* shift,
                        void* stream);
/* slab [selunet_channel_slab_rows(M)][3][C]: sum(dA), sum(dA*xhat), sum(xhat), dA = dz*[z>0],
 * z = relu(y*scale+shift), xhat = (y-mean)*invstd. */
int selunet_bn_bwd_reduce(const void* dz, const void* y, int64_t m, int32_t c, const float* scale,
                          const float* shift, const float* mean, const float* invstd, float* slab,
                          int32_t dtype, void* stream);
/* From fp64 sums [3][C]: dgamma, dbeta, dbias (pre-BN conv bias), coef [3][C]. */
int selunet_bn_bwd_finalize(const double* sums, int64_t count, int32_t c, const float* gamma,
                            const float* invstd, float* dgamma, float* dbeta, float* dbias,
                            float* coef, void* stream);
/* Fused forms used by the training step: the column sums of the statistics slab the producer
 * wrote ([rows][2][C] sum/sumsq for the forward, [rows][3][C] for the backward) reduced in fp64
 * (fixed order) and finalized in one launch (two above SELUNET_RF_SINGLE rows, default 1024).
 * Same results as selunet_reduce_rows + selunet_bn_finalize(training = 1) /
 * selunet_bn_bwd_finalize up to the fp64 summation order. ws: >= selunet_reduce_ws_bytes(2*C or
 * 3*C); sums (fp64 [2|3][C]) may be NULL. Replace BatchNorm2d's batch-statistics pass
 * (model.py:12) and its backward (autograd of model.py:12). */
int selunet_bn_stats_finalize(const float* slab, int64_t rows, double* ws, double* sums, int64_t count,
                              int32_t c, const float* conv_bias, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, int64_t* num_batches,
                              float momentum, float eps, float* mean, float* invstd, float* scale,
                              float* shift, void* stream);
/* Second (centered) pass of the batch statistics, fp32 parity configuration: slab [rows][2][c] of
 * per-channel sums of (y - center) and (y - center)^2 over y [m][c] (center = the first pass's
 * batch mean; rows = selunet_bn_centered_rows(m)); then selunet_bn_stats_finalize_centered
 * reduces it like selunet_bn_stats_finalize (mean = center + E[y - center], var = E[(y - center)^2]
 * - E[y - center]^2) and writes the same outputs — `mean` may alias `center`. Same role as
 * selunet_bn_stats_finalize (model.py:12 BatchNorm2d batch statistics), numerically two-pass. */
int64_t selunet_bn_centered_rows(int64_t m);
int selunet_bn_centered_partials(const void* y, int64_t m, int32_t c, const float* center, float* slab,
                                 int32_t dtype, void* stream);
/* Adaptive second pass: uvar[c] = the first pass's unbiased variance (selunet_bn_stats_finalize with
 * running_var = a zeroed scratch, running_mean = NULL, momentum 1). A group of 4 channels is re-read
 * (as selunet_bn_centered_partials) only if one of them has center^2 > ratio * uvar — where
 * E[y^2] - mean^2 loses digits; the others write the sums that make the centered finalize return
 * the first pass's variance. Same slab layout and finalize. */
int selunet_bn_centered_partials_adaptive(const void* y, int64_t m, int32_t c, const float* center,
                                          const float* uvar, float ratio, float* slab, int32_t dtype,
                                          void* stream);
/* First pass of the fp32 batch statistics from a slab of SHIFTED sums (selunet_epilogue.stats_center =
 * center, the previous step's batch mean): mean = center + E[y - center]; uvar_flag[c] = the unbiased
 * one-pass variance, or -1 where (mean - center)^2 > ratio * var (there it loses digits); center is
 * then overwritten with mean (the next step's center). invstd / scale / shift are provisional (eps
 * 1e-5, no running-statistic update). Followed by selunet_bn_centered_partials_adaptive(center = mean,
 * uvar = uvar_flag, ratio = +inf: re-reads exactly the flagged channel groups) and
 * selunet_bn_stats_finalize_centered, whose outputs are final. In training the previous batch mean
 * differs from the current one by a small fraction of the standard deviation, so after the first
 * step almost no channel group is re-read. */
int selunet_bn_stats_finalize_shifted(const float* slab, int64_t rows, double* ws, int64_t count, int32_t c,
                                      float* center, const float* conv_bias, const float* gamma,
                                      const float* beta, float ratio, float* mean, float* uvar_flag,
                                      float* invstd, float* scale, float* shift, void* stream);
int selunet_bn_stats_finalize_centered(const float* slab, int64_t rows, double* ws, double* sums,
                                       int64_t count, int32_t c, const float* center,
                                       const float* conv_bias, const float* gamma, const float* beta,
                                       float* running_mean, float* running_var, int64_t* num_batches,
                                       float momentum, float eps, float* mean, float* invstd,
                                       float* scale, float* shift, void* stream);
/* selunet_bn_stats_finalize_centered that also folds the split-fp16 range word of relu(bn(y)) into
 * *bound (zeroed by the caller before the step): atomic max over the channels of
 * (|gamma_c| * sqrt(count) + |beta_c|) * 1.0001 — the per-channel form of selunet_act_bound's
 * Samuelson bound (never larger), without its separate launch. bound may be NULL. */
int selunet_bn_stats_finalize_centered_bound(const float* slab, int64_t rows, double* ws, double* sums,
                                             int64_t count, int32_t c, const float* center,
                                             const float* conv_bias, const float* gamma, const float* beta,
                                             float* running_mean, float* running_var, int64_t* num_batches,
                                             float momentum, float eps, float* mean, float* invstd,
                                             float* scale, float* shift, float* bound, void* stream);
int selunet_bn_bwd_stats_finalize(const float* slab, int64_t rows, double* ws, double* sums,
                                  int64_t count, int32_t c, const float* gamma, const float* invstd,
                                  float* dgamma, float* dbeta, float* dbias, float* coef,
                                  void* stream);
/* selunet_bn_bwd_stats_finalize that also folds an upper bound of |dy| into *bound (zeroed by the
 * caller; atomic max over the channels of 1.25 * (|k0| amax_da + |k1| + |k2| sqrt(count)), amax_da the
 * exact max |dA| its producer recorded): the range word selunet_conv3x3_wgrad_x2_bn stages dy with
 * before dy exists. */
int selunet_bn_bwd_stats_finalize_bound(const float* slab, int64_t rows, double* ws, double* sums,
                                        int64_t count, int32_t c, const float* gamma, const float* invstd,
                                        float* dgamma, float* dbeta, float* dbias, float* coef,
                                        const float* amax_da, float* bound, void* stream);
/* dy = coef0*dA - coef1 - coef2*xhat (the conv-output gradient). */
int selunet_bn_bwd_apply(const void* dz, const void* y, int64_t m, int32_t c, const float* scale,
                         const float* shift, const float* mean, const float* invstd,
                         const float* coef, void* dy, int32_t dtype, void* stream);
/* The same with max|dy| folded into *amax (atomic max on the float bits; zeroed by the caller):
 * the range word of dy as a split-fp16 operand (selunet_conv3x3_x2, split-fp16 weight gradient). */
int selunet_bn_bwd_apply_amax(const void* dz, const void* y, int64_t m, int32_t c, const float* scale,
                              const float* shift, const float* mean, const float* invstd,
                              const float* coef, void* dy, float* amax, int32_t dtype, void* stream);

/* Stream-ordered device memset / device-to-device copy (hipMemsetAsync / hipMemcpyAsync):
 * zeroing atomic-accumulation targets and gathering small parameter vectors inside a recorded
 * launch plan, without host synchronisation. */
int selunet_memset(void* dst, int32_t value, int64_t bytes, void* stream);
int selunet_memcpy(void* dst, const void* src, int64_t bytes, void* stream);

/* ---- HIP graphs of recorded launch plans ---------------------------------------------------
 * A replayed launch plan (a whole forward or backward pass, ~100 launches) is captured once into
 * a hipGraph and afterwards issued with one selunet_graph_launch instead of one host call per
 * kernel. Capture runs on a private non-blocking stream (the default stream cannot capture);
 * the instantiated graph is then launched on the caller's stream. */
int selunet_stream_create(void** out);
int selunet_stream_destroy(void* stream);
int selunet_graph_capture_begin(void* stream);
int selunet_graph_capture_end(void* stream, void** exec);
int selunet_graph_launch(void* exec, void* stream);
int selunet_graph_destroy(void* exec);

/* ---- first layer (C_in = 3 or 2, model.py:24-29) --------------------------------------- */
/* x NCHW fp32 -> out [n*h*w][k_pad] in dtype: column tap*c + ci of the 3x3 pad-1 window, zero
 * for columns >= 9c. The first conv then runs as selunet_gemm_gather with taps = 1. */
int selunet_im2col3x3(const float* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t k_pad, void* out,
                      int32_t dtype, void* stream);
/* encoder_layer_1_1's conv (model.py:29) straight from the NCHW fp32 input x [n][cin][h][w]
 * (cin <= 3) to y [n*h*w][64] in dtype, no bias (it cancels in training-mode BN), with the BN
 * column statistics of selunet_gemm_gather (stats [selunet_first_conv_rows][2][64], nullable).
 * wpack: the conv weight from selunet_pack_conv3x3 with k_pad = 32. */
int64_t selunet_first_conv_rows(int32_t n, int32_t h, int32_t w);
/* selunet_first_conv_fwd with its statistics shifted by center (selunet_epilogue.stats_center). */
int selunet_first_conv_fwd_centered(const float* x, int32_t n, int32_t cin, int32_t h, int32_t w,
                                    const void* wpack, void* y, float* stats, const float* center,
                                    int32_t dtype, void* stream);
int selunet_first_conv_fwd(const float* x, int32_t n, int32_t cin, int32_t h, int32_t w, const void* wpack,
                           void* y, float* stats, int32_t dtype, void* stream);
/* Its weight gradient: slab [selunet_first_conv_wgrad_rows][64][32] of per-workgroup partial sums
 * of dY^T im2col(x) (column k = tap*cin + c); reduce the rows (selunet_reduce_rows) to the packed
 * [64][32] gradient, then selunet_unpack_conv3x3_grad(.., ld = 32). */
int64_t selunet_first_conv_wgrad_rows(int32_t n, int32_t h, int32_t w);
int selunet_first_conv_wgrad(const float* x, int32_t n, int32_t cin, int32_t h, int32_t w, const void* dy,
                             float* slab, int32_t dtype, void* stream);
/* The same weight gradient with encoder_layer_1_1's BatchNorm+ReLU backward fused into the staging:
 * dz = dA of the layer, y its conv output, scale/shift/mean/invstd its BN, coef [3][64] from
 * selunet_bn_bwd_stats_finalize; dy = (y*scale+shift > 0 ? k0*dz : 0) - b - a*y exactly as
 * selunet_bn_bwd_apply forms it, never written (replaces selunet_bn_bwd_apply + selunet_first_conv_wgrad,
 * whose dy has no other reader: the input needs no gradient, model.py:29 / train.py:207). */
int selunet_first_conv_wgrad_bn(const float* x, int32_t n, int32_t cin, int32_t h, int32_t w, const void* dz,
                                const void* y, const float* scale, const float* shift, const float* mean,
                                const float* invstd, const float* coef, float* slab, int32_t dtype, void* stream);

/* ---- MaxPool2d(2) on relu(bn(y)) (model.py:31,35,39) ---------------------------------- */
int selunet_maxpool2_fwd(const void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                         const float* scale, const float* shift, void* out, int32_t dtype,
                         void* stream);
/* dz = route(dpool to the first max of each window, row-major, strict >) + dskip (nullable).
 * bnb (nullable; bnb->y must be y): BatchNorm-backward sums of dz, slab
 * [selunet_maxpool2_bwd_slab_rows(n, h, w, c)][3][c]. dz may be NULL when bnb is given: the sums only
 * (selunet_bn_bwd_apply_pool then forms dz itself). */
int selunet_maxpool2_bwd(const void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                         const float* scale, const float* shift, const void* dpool,
                         const void* dskip, void* dz, const selunet_bn_bwd_stats* bnb, int32_t dtype,
                         void* stream);
int64_t selunet_maxpool2_bwd_slab_rows(int32_t n, int32_t h, int32_t w, int32_t c);

/* ---- 1x1 heads conv1x1 / conv_select / conv_aux on relu(bn(y)), C = 64 (model.py:62-66) */
int selunet_heads_fwd(const void* y, int64_t m, const float* scale, const float* shift,
                      const float* w, const float* b, int32_t nh, float* out0, float* out1,
                      float* out2, int32_t dtype, void* stream);
/* dz[m][c] = sum_h g_h[m] w_h[c]; slab [selunet_channel_slab_rows(M)][nh][65]: per head
 * sum g*z (weight grad, 64) and sum g (bias grad). bnb (nullable; bnb->y must be y):
 * BatchNorm-backward sums of dz, slab [selunet_channel_slab_rows(M)][3][64]. */
int selunet_heads_bwd(const void* y, int64_t m, const float* scale, const float* shift,
                      const float* w, int32_t nh, const float* g0, const float* g1,
                      const float* g2, void* dz, float* slab, const selunet_bn_bwd_stats* bnb,
                      int32_t dtype, void* stream);
/* BatchNorm-backward apply (as selunet_bn_bwd_apply_amax; amax nullable) with dA formed on the fly
 * instead of read, for the two producers whose dA is cheap to recompute — their kernels then run in
 * sums-only mode (dz = NULL), so dA is never written:
 *  _heads: dA[m][c] = sum_h g_h[m] w_h[c] (C = 64; the arguments of selunet_heads_bwd);
 *  _pool:  dA = route(dpool) + dskip (the arguments of selunet_maxpool2_bwd).
 * dA is rounded to dtype before use, as the stored tensor of the unfused path. Replaces the
 * selunet_heads_bwd / selunet_maxpool2_bwd write + selunet_bn_bwd_apply read of dA for decoder_layer_1_1
 * and encoder_layer_{1,2,3}_2 (model.py:62-66, 31/35/39, the backward of CBR_2D model.py:12-13). */
int selunet_bn_bwd_apply_heads(const void* y, int64_t m, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* coef,
                               const float* w, int32_t nh, const float* g0, const float* g1,
                               const float* g2, void* dy, float* amax, int32_t dtype, void* stream);
int selunet_bn_bwd_apply_pool(const void* y, int32_t n, int32_t h, int32_t w, int32_t c,
                              const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* coef, const void* dpool,
                              const void* dskip, void* dy, float* amax, int32_t dtype, void* stream);

/* ---- N-output 1x1 heads (the CE `UNet`, model.py:106-191: conv1x1 64->n_cls, conv_select
 * 64->2, conv_aux 64->n_cls) on relu(bn(y)), C = 64. Output k (k < n <= 8) is an fp32 plane
 * set: pixel q of image i at plane[k][i * img_stride[k] + q] (q < hw), so the channels of
 * NCHW [N, C, H, W] logits are planes base + c*hw with img_stride C*hw. */
typedef struct selunet_head_planes {
  int32_t n;               /* outputs (<= 8) */
  int32_t hw;              /* pixels per image */
  float* plane[8];         /* fwd: written; bwd: the incoming gradients (read) */
  int64_t img_stride[8];
  int32_t w_off[8];        /* bwd: slab column of output k's 64 weight grads */
  int32_t b_off[8];        /*      and of its bias grad */
  int32_t row_len;         /*      slab row length (the heads' segment of the gradient buffer) */
} selunet_head_planes;
/* w fp32 [n][64], b fp32 [n] */
int selunet_heads_fwd_planes(const void* y, int64_t m, const float* scale, const float* shift,
                             const float* w, const float* b, const selunet_head_planes* out,
                             int32_t dtype, void* stream);
/* dz[m][c] = sum_k g_k[m] w_k[c]; slab [selunet_channel_slab_rows(M)][row_len]: per output the
 * sums g*z (64, at w_off) and g (at b_off); bnb as selunet_heads_bwd. */
int selunet_heads_bwd_planes(const void* y, int64_t m, const float* scale, const float* shift,
                             const float* w, const selunet_head_planes* grads, void* dz, float* slab,
                             const selunet_bn_bwd_stats* bnb, int32_t dtype, void* stream);
/* selunet_bn_bwd_apply_heads for the N-output heads: dA[m][c] = sum_k g_k[m] w_k[c] from the gradient
 * planes of selunet_heads_bwd_planes (which then runs with dz = NULL: the sums only). */
int selunet_bn_bwd_apply_heads_planes(const void* y, int64_t m, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, const float* coef,
                                      const float* w, const selunet_head_planes* grads, void* dy,
                                      float* amax, int32_t dtype, void* stream);

/* ---- losses ----------------------------------------------------------------------------- */
/* calc_selective_risk_image_b (selective_loss.py:58-85), numerically stable form.
 * partials slab [selunet_loss_slab_rows(P)][2]: sum sigmoid(g), sum ell*sigmoid(g). */
int64_t selunet_loss_slab_rows(int64_t p);
int selunet_selective_partials(const float* out, const float* sel, const float* target,
                               int64_t p, float* slab, void* stream);
/* sums[2] global (after any cross-rank all-reduce), p_global pixels -> loss, coverage,
 * and state[4] = {S0, R, d, P} for the backward. */
int selunet_selective_finalize(const double* sums, double p_global, float lamb,
                               float target_coverage, float* loss, float* coverage,
                               float* state, void* stream);
int selunet_selective_bwd(const float* out, const float* sel, const float* target, int64_t p,
                          const float* state, float lamb, const float* g_loss,
                          const float* g_coverage, float* d_out, float* d_sel, void* stream);
/* hard_selection=True (selective_loss.py:74-77): the risk numerator weights pixels by the detached
 * hard selection [sigmoid(g) > 0.5] (slab column 1 = sum ell*[sigmoid(g) > 0.5]; column 0 stays
 * sum sigmoid(g), the coverage); finalized by selunet_selective_finalize. Selection and coverage are
 * detached in the reference, so the backward writes d_sel = 0 and
 * d_out = g_loss * [sigmoid(g) > 0.5] * (sigmoid(x) - t) / sum sigmoid(g). */
int selunet_selective_partials_hard(const float* out, const float* sel, const float* target,
                                    int64_t p, float* slab, void* stream);
int selunet_selective_bwd_hard(const float* out, const float* sel, const float* target, int64_t p,
                               const float* state, const float* g_loss, float* d_out, float* d_sel,
                               void* stream);
/* BCEWithLogitsLoss() mean (train.py:78): slab [selunet_loss_slab_rows(P)][1]. */
int selunet_bce_partials(const float* logit, const float* target, int64_t p, float* slab,
                         void* stream);
int selunet_bce_finalize(const double* sums, double p_global, float* loss, void* stream);
int selunet_bce_bwd(const float* logit, const float* target, int64_t p, double p_global,
                    const float* g_loss, float* d_logit, void* stream);
/* Cross-entropy forms (CE `UNet`, n_cls = C <= 8): logits NCHW fp32 [N][C][hw], selection NCHW
 * [N][2][hw], target int64 class indices [N][hw] (a value outside [0, C) makes that pixel's loss
 * term and gradients NaN, as torch rejects it).
 * calc_selective_risk_image (selective_loss.py:24-56): s = softmax(selection)[:, 1],
 * ell = -log_softmax(output)[target]; partials slab [selunet_loss_slab_rows(N*hw)][2] = sum s,
 * sum ell*s — finalized by selunet_selective_finalize exactly as the BCE form. */
int selunet_ce_selective_partials(const float* out, const float* sel, const int64_t* target, int64_t n,
                                  int32_t c, int64_t hw, float* slab, void* stream);
int selunet_ce_selective_bwd(const float* out, const float* sel, const int64_t* target, int64_t n, int32_t c,
                             int64_t hw, const float* state, float lamb, const float* g_loss,
                             const float* g_coverage, float* d_out, float* d_sel, void* stream);
/* hard_selection=True of the CE form (selective_loss.py:43-48), as the _hard BCE entry points. */
int selunet_ce_selective_partials_hard(const float* out, const float* sel, const int64_t* target, int64_t n,
                                       int32_t c, int64_t hw, float* slab, void* stream);
int selunet_ce_selective_bwd_hard(const float* out, const float* sel, const int64_t* target, int64_t n,
                                  int32_t c, int64_t hw, const float* state, const float* g_loss,
                                  float* d_out, float* d_sel, void* stream);
/* torch.nn.CrossEntropyLoss() mean (train.py:80): slab [selunet_loss_slab_rows(N*hw)][1] = sum ell,
 * finalized by selunet_bce_finalize (sum / P). */
int selunet_ce_partials(const float* logit, const int64_t* target, int64_t n, int32_t c, int64_t hw,
                        float* slab, void* stream);
int selunet_ce_bwd(const float* logit, const int64_t* target, int64_t n, int32_t c, int64_t hw, double p_global,
                   const float* g_loss, float* d_logit, void* stream);

/* ---- torch.optim.Adam (train.py:90,209), multi-tensor ---------------------------------- */
typedef struct selunet_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  int64_t chunk_begin; /* prefix sum of ceil(numel / SELUNET_ADAM_CHUNK) */
} selunet_adam_tensor;
#define SELUNET_ADAM_CHUNK 4096
/* list: device array of n entries. step: the 1-based step count after increment. */
int selunet_adam_step(const selunet_adam_tensor* list, int32_t n, int64_t total_chunks, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int64_t step,
                      void* stream);

/* ---- training-loop I/O ------------------------------------- */
/* Pre-decoded patches -> network input and BCE target, replacing PatchDataset.__getitem__'s
 * numpy transforms (utils/data_utils.py:94-125,160-168,220-221; train.py:189-191).
 * img: uint8 NHWC [n][h][w][cin] (cin = 3, RGB); lab: uint8 [n][h][w] raw mask values (only 255
 * maps to 1); flips: uint8 [n] (bit 0 = np.fliplr, bit 1 = np.flipud; NULL = none).
 * x: fp32 NCHW [n][3][h][w] = (float32(v/255.0) - 0.5)/0.5; target: fp32 [n][h][w] in {0,1}.
 * cin = 2: input_type 'GH' (utils/data_utils.py:13-27): x [n][2][h][w] = normalised (cv2 gray,
 * skimage hematoxylin stain min-max scaled with the reference's constants). */
int selunet_prep_batch(const uint8_t* img, const uint8_t* lab, const uint8_t* flips, int32_t n,
                       int32_t h, int32_t w, int32_t cin, float* x, float* target, void* stream);
/* The same by input_type: mode 0 'RGB', 1 'GH', 2 'H_RGB' (utils/data_utils.py:29-41: the
 * hematoxylin stain recombined alone by skimage.color.combine_stains; x [n][3][h][w]). */
int selunet_prep_batch_mode(const uint8_t* img, const uint8_t* lab, const uint8_t* flips, int32_t n,
                            int32_t h, int32_t w, int32_t mode, float* x, float* target, void* stream);
/* selunet_prep_batch_mode with the training augmentation deciding which three bytes and
 * which label byte of the uint8 batch enter the same per-pixel conversion. All arrays are DEVICE arrays.
 * For output pixel (y, x) of image b:
 *   glass: uint8 [n] or NULL; 0 = none, 1..4 = a quadrant of the OUTPUT (hh = h / 2, hw = w / 2; 1: y < hh,
 *     x < hw; 2: y < hh, x >= hw; 3: y >= hh, x < hw; 4: y >= hh, x >= hw). A pixel of that quadrant gets
 *     byte_c = table[u(key[b], (y w + x) 3 + c) >> 20] and label byte 0. table: uint8 [4096], the glass model
 *     0.96 + 0.005 N(0,1) quantised to bytes; key: uint32 [n];
 *     u(k, i) = mix(mix(k) + i * 0x9E3779B9) in uint32 arithmetic,
 *     mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16.
 *   geom: uint8 [n] or NULL (0); every other pixel is the source pixel img[b][xs][ys] when geom[b] & 4, else
 *     img[b][ys][xs], with ys = h-1-y when geom[b] & 2 and xs = w-1-x when geom[b] & 1 (the `flips` of
 *     selunet_prep_batch when bit 2 is clear); its label byte comes from the same place.
 *   transposed: nonzero iff some geom[b] has bit 2 set (the caller knows its own draws: the call reads no
 *     device memory). Then h == w is required; when zero, bit 2 of geom is ignored.
 *   lut: uint8 [n][3][256] or NULL; byte_c = lut[b][c][byte_c] for pixels that are not glass.
 * x / target as selunet_prep_batch_mode. EINVAL for a mode outside 0..2, w % 4 != 0, outputs not 16-B
 * aligned, transposed with h != w or without geom, glass without table or key. */
int selunet_prep_batch_aug(const uint8_t* img, const uint8_t* lab, const uint8_t* geom,
                           const uint8_t* glass, const uint32_t* key, const uint8_t* lut,
                           const uint8_t* table, int32_t transposed, int32_t n, int32_t h, int32_t w,
                           int32_t mode, float* x, float* target, void* stream);
/* Per-batch metrics of train.py:211-238 / eval.py:218-246 accumulated on the device:
 * counts[6] (uint64, caller-zeroed, accumulated across calls) = {cm[0][0], cm[0][1], cm[1][0],
 * cm[1][1], selected, total} with cm[label][pred] = Evaluator.confusion_matrix
 * (utils/compute_metric.py:10-26) over pixels whose selection logit >= t_sel (all pixels when
 * sel is NULL); pred = out >= t_out. t_out / t_sel: the smallest fp32 logit the reference's
 * host rule (sigmoid in fp64 or fp32, then > cut_off) maps to 1. */
int selunet_seg_metrics(const float* out, const float* sel, const float* target, int64_t p,
                        float t_out, float t_sel, unsigned long long* counts, void* stream);

/* Risk-coverage sweep: the counts of selunet_seg_metrics at k selection thresholds in one pass.
 * bins: uint64 [(k+1)][5], caller-zeroed, accumulated across calls.
 * bin b of a pixel = number of j in [0,k) with sel >= t_sel[j]
 *   (t_sel: DEVICE array, ascending — the caller's duty —, duplicates and +-inf allowed;
 *    NaN sel -> bin 0).
 * bins[b] = {cm[0][0], cm[0][1], cm[1][0], cm[1][1], pixels}
 *   cm[label][pred], pred = out >= t_out, label = (uint8)target, counted only when label < 2
 *   (the rule of selunet_seg_metrics); `pixels` counts every pixel of the bin whatever its label.
 * For every j the sum of bins[b] over b > j equals counts[0..4] of selunet_seg_metrics at
 * t_sel[j], and the sum of `pixels` over all bins its counts[5]. Integer atomics only: the result
 * does not depend on scheduling. EINVAL for a null pointer, p <= 0 or p > 2^40 (a 32-bit
 * on-chip counter could overflow beyond), k outside [1, SELUNET_SWEEP_MAX], out / sel / target
 * not 16-B aligned. */
#define SELUNET_SWEEP_MAX 256
int selunet_seg_metrics_sweep(const float* out, const float* sel, const float* target, int64_t p,
                              float t_out, const float* t_sel, int32_t k,
                              unsigned long long* bins, void* stream);

/* Per-patch report (the reference's get_performance, utils/compute_metric.py:93-148, per image of a
 * batch of n images of hw pixels each; out / sel / target [n][hw] fp32, sel nullable).
 * Both calls: EINVAL for a null pointer (sel may be null), n < 1, hw < 1, hw % 4 != 0 or hw > 2^20
 * (the 32-bit on-chip partial counts are sized for it), out / sel / target not 16-B aligned, rows
 * not 8-B aligned. Integer atomics only: the result does not depend on scheduling. */
/* Row i (i < n) += the six counts of selunet_seg_metrics over image i alone
 * (pixels [i*hw, (i+1)*hw)): rows [n][6], uint64, caller-zeroed. */
int selunet_seg_metrics_rows(const float* out, const float* sel, const float* target,
                             int32_t n, int64_t hw, float t_out, float t_sel,
                             unsigned long long* rows, void* stream);
/* Exact per-image Mann-Whitney statistic of the prediction logit.
 * rows [n][4] uint64, caller-zeroed, += {two_u, n_pos, n_neg, n_nan}.
 * A pixel is considered when label = (int)(uint8_t)target < 2 (the rule of selunet_seg_metrics), it
 * is selected (sel == NULL or sel >= t_sel) and out is not NaN; considered pixels of label 1 form P,
 * of label 0 form N; selected pixels of label < 2 with a NaN out are counted in n_nan only.
 *   two_u = sum over p in P of ( 2 * #{q in N: out_q < out_p} + #{q in N: out_q == out_p} ),
 *   n_pos = |P|, n_neg = |N|,
 * in the numeric fp32 order (-0 == +0; +-inf and denormals are ordinary values). The ROC AUC of the
 * image, ties at one half (sklearn's roc_auc_score), is two_u / (2 * n_pos * n_neg).
 * The statistic is taken on the logit, not on its sigmoid: the fp32 sigmoid is monotone but merges
 * neighbouring and saturated logits into ties, so the logit is the finer ranking.
 * No workspace: the negatives are sorted on chip in chunks of SELUNET_AUC_CHUNK pixels. */
#define SELUNET_AUC_CHUNK 4096
int selunet_patch_auc(const float* out, const float* sel, const float* target,
                      int32_t n, int64_t hw, float t_sel,
                      unsigned long long* rows, void* stream);

/* ---- boundary-distance metrics -------------------------------------------------
 * Where a selective network abstains and how far its errors lie from the annotation: an exact
 * Euclidean distance transform of a thresholded plane, and the counts of selunet_seg_metrics by
 * distance band and per image. Integer arithmetic and integer atomics only: every result is the same
 * bit for bit on every run. */
/* The value of selunet_edt_sq for every pixel of an image that holds one class only. */
#define SELUNET_EDT_NONE INT32_MAX
#define SELUNET_EDT_MAX_SIDE 4096
/* Squared Euclidean distance to the other class. x: fp32 [n][h][w]; a pixel is foreground iff
 * x >= t (a NaN is background). d2: int32 [n][h][w] = the smallest (y - y')^2 + (x - x')^2 over the
 * pixels (y', x') of the same image whose class differs from the pixel's own, hence >= 1;
 * SELUNET_EDT_NONE throughout an image of one class. Exact for 1 <= h, w <= SELUNET_EDT_MAX_SIDE
 * (2 * 4095^2 < 2^31). Two launches (columns, then rows in place in d2), no workspace.
 * EINVAL: a null pointer; n < 1; h or w outside [1, SELUNET_EDT_MAX_SIDE]; n * max(h, w) >= 2^31;
 * x or d2 not 4-B aligned. */
int selunet_edt_sq(const float* x, float t, int32_t n, int32_t h, int32_t w, int32_t* d2, void* stream);
/* The six words of selunet_seg_metrics by distance band. out / sel / target: fp32 [n][hw] (sel
 * nullable) with selunet_seg_metrics' rules for thresholds, NaNs, labels and a null sel; d2_target:
 * int32 [n][hw], selunet_edt_sq of the target. r2: HOST array of k squared radii, strictly increasing,
 * r2[0] >= 1, 1 <= k <= SELUNET_BAND_MAX (read during the call only). bins: uint64 [k + 2][6],
 * caller-zeroed, accumulated across calls; row b += the six counts over the pixels of band b:
 *   band 0: d2 <= r2[0]; band j (0 < j < k): r2[j-1] < d2 <= r2[j]; band k: r2[k-1] < d2, finite;
 *   band k + 1: d2 == SELUNET_EDT_NONE (images without a contour).
 * The sum of the rows is what selunet_seg_metrics counts over the same pixels.
 * EINVAL: a null pointer (sel may be null); n < 1, hw < 1 or n * hw > 2^40; a bad k or r2; out, sel,
 * target or d2_target not 16-B aligned; bins not 8-B aligned. */
#define SELUNET_BAND_MAX 15
int selunet_boundary_bands(const float* out, const float* sel, const float* target, const int32_t* d2_target,
                           int32_t n, int64_t hw, float t_out, float t_sel, const int32_t* r2, int32_t k,
                           unsigned long long* bins, void* stream);
/* Per-image error distances. d2_pred: selunet_edt_sq of out at t_out (always of the full prediction
 * mask, whatever sel). With label = (int)(uint8_t)target and pred = out >= t_out as selunet_seg_metrics,
 * over the pixels that are selected (sel == NULL or sel >= t_sel): a false positive has label 0 and
 * pred 1, a false negative label 1 and pred 0. rows: uint64 [n][6], caller-zeroed; row i becomes
 *   word 0 = max(word 0, max of d2_target over the false positives)   (0 when there are none),
 *   word 1 = max(word 1, max of d2_pred over the false negatives),
 *   words 2, 3 += false positives with d2_target <= tol_sq, false negatives with d2_pred <= tol_sq,
 *   words 4, 5 += false positives, false negatives.
 * Word 0 is the squared directed Hausdorff distance from the predicted region to the label region
 * (SELUNET_EDT_NONE: the label region is empty), word 1 the converse.
 * EINVAL: a null pointer (sel may be null); n < 1; hw outside [1, 2^24]; tol_sq < 0; a pointer not
 * 4-B aligned, or not 16-B aligned when hw % 4 == 0 (the vector path); rows not 8-B aligned. */
int selunet_boundary_rows(const float* out, const float* sel, const float* target, const int32_t* d2_target,
                          const int32_t* d2_pred, int32_t n, int64_t hw, float t_out, float t_sel,
                          int32_t tol_sq, unsigned long long* rows, void* stream);

/* ---- calibration report ---------------------------------------------------------
 * Can a score be read as a probability: the reliability histogram of sigmoid(score / T) against an
 * event, with the sums behind the Brier score and the NLL, and a fine histogram of the raw score for a
 * temperature fit. Integer counts, fixed-point integer sums and integer atomics only: every result is
 * the same bit for bit on every run.
 * score / out / sel / target: fp32 [p] (out nullable with event 0, sel nullable; they may alias).
 * With label = (int)(uint8_t)target, a pixel is considered when label < 2, it is selected (sel == NULL
 * or sel >= t_sel) and score is not NaN (the rules of selunet_seg_metrics and selunet_patch_auc);
 * selected pixels with label < 2 and a NaN score are counted in misc[0] only, selected pixels with
 * label >= 2 in misc[1] only (misc: uint64 [2], caller-zeroed, accumulated).
 * The event e of a considered pixel: event 0: e = label; event 1: e = ((out >= t_out) == (label == 1)),
 * "the prediction is right".
 * Its reliability bin b = #{j < m : score >= edges[j]} on the raw score (edges: DEVICE array, ascending
 * — the caller's duty —, duplicates and +-inf allowed, 1 <= m <= SELUNET_CALIB_MAX_EDGES; the caller
 * folds any temperature into the edges).
 * Its values, in fp64: x = (double)score * inv_temperature,
 *   s = x >= 0 ? 1 / (1 + exp(-x)) : exp(x) / (1 + exp(x)),
 *   P = llrint(s * 2^FRAC_BITS), B = llrint((s - e)^2 * 2^FRAC_BITS),
 *   L = llrint(min(softplus(e ? -x : x), NLL_MAX) * 2^NLL_BITS), softplus(v) = max(v, 0) + log1p(exp(-|v|));
 * +-inf scores are ordinary values (s is exactly 0 or 1, a wrong one costs the capped NLL_MAX nats).
 * bins: uint64 [(m + 1)][5], caller-zeroed, accumulated across calls: bins[b] += {1 - e, e, P, B, L}.
 * fine (nullable): uint64 [SELUNET_CALIB_FINE_CELLS][2], caller-zeroed, accumulated: fine[cell][e] += 1 with
 *   cell 0 for score < -32, cell 4097 for score >= 32, else 2049 + (int)floorf(score * 64.0f) (the fp32
 *   product is exact).
 * The sums are sized for 2^33 accumulated pixels (2^33 * 2^30 < 2^64): keeping the accumulated total below
 * it is the caller's duty. Per launch a workgroup counts about p / 256 <= 2^25 pixels into a 32-bit
 * on-chip counter of `fine`; the on-chip sums of `bins` are 64 bits wide.
 * EINVAL (before any device call): a null pointer where one is required; p < 1 or p > 2^33; event outside
 * {0, 1}; m out of range; inv_temperature not finite or not > 0; score / out / sel / target not 16-B
 * aligned, edges not 4-B aligned, bins / fine / misc not 8-B aligned. */
#define SELUNET_CALIB_MAX_EDGES 255
#define SELUNET_CALIB_FRAC_BITS 30
#define SELUNET_CALIB_NLL_BITS 20
#define SELUNET_CALIB_NLL_MAX 1024
#define SELUNET_CALIB_FINE_CELLS 4098
int selunet_calibration_bins(const float* score, const float* out, const float* sel, const float* target,
                             int64_t p, int32_t event, float t_out, float t_sel,
                             const float* edges, int32_t m, double inv_temperature,
                             unsigned long long* bins, unsigned long long* fine,
                             unsigned long long* misc, void* stream);

/* ---- whole-image prediction I/O --------------------------------------------
 * A trained network applied to an image of any size: overlapping tiles are gathered from the image, run
 * through the eval-mode forward, and the tiles' cores (tile minus a halo on every side) stitched into
 * canvases. origins: DEVICE int32 [n][2] = (y0, x0) of each tile in image coordinates; it is never read on
 * the host. Both calls: EINVAL for a null pointer, n < 1, H or W outside [1, 65535], th or tw < 8 or not a
 * multiple of 8. */
/* img: uint8 [H][W][3] RGB on the device. x: fp32 [n][C][th][tw], C = 3 (mode 0 'RGB', 2 'H_RGB') or 2
 * (mode 1 'GH'). Element (i, c, y, x) is what selunet_prep_batch_mode gives, without flip, for the source
 * pixel (refl(y0 + y, H), refl(x0 + x, W)); refl is numpy's 'reflect' padding as an index map: the edge is
 * not repeated, period 2 (n - 1), folded as often as needed, 0 for n = 1. Origins may be negative or past
 * the edge. Also EINVAL: a bad mode, x not 16-B aligned. */
int selunet_tile_gather(const uint8_t* img, int32_t H, int32_t W, const int32_t* origins, int32_t n,
                        int32_t th, int32_t tw, int32_t mode, float* x, void* stream);
/* out, sel: fp32 [n][th][tw] logits (sel nullable; sel_plane is null exactly when sel is). The core of
 * tile i, rows and columns [halo, th - halo) x [halo, tw - halo), goes to canvas position
 * (y0 + halo, x0 + halo) of the canvases [Hc][Wc] (Hc >= H, Wc >= W, Wc % 8 == 0; the image is their
 * [:H, :W] corner):
 *   logit_plane, sel_plane (fp32) = out, sel unchanged;
 *   mask (uint8) = 127 if sel != NULL and not (sel >= t_sel), else 255 if out >= t_out, else 0
 *     (a NaN selection abstains, a NaN output is background: the rule of selunet_seg_metrics);
 *   prob8 (uint8, nullable) = floor(255 sigmoid(out) + 0.5), 0 for a NaN.
 * counts: uint64 [4], caller-zeroed, += {background, tumor, abstained, pixels} over the canvas pixels with
 * y < H and x < W. Integer atomics only: the result does not depend on scheduling. Canvas pixels outside
 * every core of the call are left untouched.
 * The caller's duty (the origins live on the device): every core lies inside the canvas at a column that
 * is a multiple of 8. An 8-pixel group that does not is skipped, neither stored nor counted.
 * Also EINVAL: halo < 0, halo % 8 != 0 or 2 * halo >= min(th, tw); Hc < H, Wc < W or Wc % 8 != 0; out, sel
 * or a plane not 16-B aligned; counts not 8-B aligned; 2^32 or more core pixels in one call. */
int selunet_tile_stitch(const float* out, const float* sel, const int32_t* origins, int32_t n, int32_t th,
                        int32_t tw, int32_t halo, int32_t H, int32_t W, int32_t Hc, int32_t Wc,
                        float t_out, float t_sel, float* logit_plane, float* sel_plane, uint8_t* mask,
                        uint8_t* prob8, unsigned long long* counts, void* stream);

/* ---- flip / D4 test-time augmentation of whole-image prediction --------------
 * Member k = 0..7 of the ensemble is the prediction of T_k(image) mapped back by T_k^-1: bit 2 of k
 * transposes the image, then bit 1 flips its rows, then bit 0 its columns. The image is transposed once
 * (selunet_image_transpose), so the per-tile calls take a flip code 0..3 (k & 3) and the image of the
 * member's orientation class: the image itself (k < 4) or its transpose. */
/* selunet_tile_gather of the flipped image without forming it: element (i, c, y, x) comes from source row
 * fy(refl(y0 + y, H)) and column fx(refl(x0 + x, W)), fy(r) = H - 1 - r if flip & 2 else r, fx(c) = W - 1 - c if
 * flip & 1 else c. Arguments and EINVALs as selunet_tile_gather's; also EINVAL: flip outside [0, 3]. */
int selunet_tile_gather_flip(const uint8_t* img, int32_t H, int32_t W, const int32_t* origins, int32_t n,
                             int32_t th, int32_t tw, int32_t mode, int32_t flip, float* x, void* stream);
/* src: uint8 [H][W][3] -> dst: uint8 [W][H][3], dst[x][y] = src[y][x]; not in place. EINVAL: a null
 * pointer, src == dst, H or W outside [1, 65535]. */
int selunet_image_transpose(const uint8_t* src, int32_t H, int32_t W, uint8_t* dst, void* stream);
/* One batch of one member's output tiles into the running sums of its orientation class. out, sel: fp32
 * [n][th][tw] as selunet_tile_stitch's (sel, sum_sel and sel_votes all null or all given); H x W: the
 * member's image (the transposed size for k >= 4). Canvas pixel (cy, cx) of a core with cy < H and cx < W goes
 * to (fy(cy), fx(cx)) of the planes [H][ws] (ws >= W, ws % 8 == 0):
 *   sum_out, sum_sel (fp32) += out, sel       (first = 1: = out, sel; the class's first member);
 *   votes, sel_votes (uint8) += out >= t_out, sel >= t_sel   (first = 1: =; a NaN casts no vote).
 * Everything else in the planes is left untouched. Each pixel is read and written by one thread, without
 * atomics: with one call after another on one stream the order of the additions is the order of the calls.
 * The caller's duty: the cores of one call do not overlap, and a member's calls cover every image pixel once.
 * Also EINVAL: the halo rule of selunet_tile_stitch; flip outside [0, 3]; first not 0 or 1; ws < W or
 * ws % 8 != 0; tiles or planes not 16-B aligned. */
int selunet_tta_accumulate(const float* out, const float* sel, const int32_t* origins, int32_t n, int32_t th,
                           int32_t tw, int32_t halo, int32_t flip, int32_t first, int32_t H, int32_t W,
                           int32_t ws, float t_out, float t_sel, float* sum_out, float* sum_sel,
                           uint8_t* votes, uint8_t* sel_votes, void* stream);
/* The mean of the members and what follows from it. a_*: the sums and votes of members 0..3, [H][wa]; b_*:
 * those of members 4..7 in the transposed orientation, [W][hb] (all null for members = 4). For y < H, x < wa
 * (outputs [H][wa]; wa >= W, hb >= H, both multiples of 8):
 *   logit_plane, sel_plane = a * 0.25 (members = 4) or (a + b^T) * 0.125 (members = 8), in fp32;
 *   mask, prob8 (nullable): selunet_tile_stitch's rules applied to those means;
 *   votes, sel_votes = a_votes (+ b_votes^T), a_sel_votes (+ b_sel_votes^T).
 * counts: uint64 [4], caller-zeroed, += {background, tumor, abstained, pixels} over x < W, integer atomics.
 * The selection arguments (a_sel, a_sel_votes, sel_plane, sel_votes, and b_sel, b_sel_votes for members = 8)
 * are all given or all null. EINVAL: members not 4 or 8; a missing or a superfluous pointer; H or W outside
 * [1, 65535]; wa < W, hb < H or either not a multiple of 8; a plane not 16-B aligned; counts not 8-B aligned. */
int selunet_tta_finalize(const float* a_out, const float* a_sel, const uint8_t* a_votes,
                         const uint8_t* a_sel_votes, const float* b_out, const float* b_sel,
                         const uint8_t* b_votes, const uint8_t* b_sel_votes, int32_t members, int32_t H,
                         int32_t W, int32_t wa, int32_t hb, float t_out, float t_sel, float* logit_plane,
                         float* sel_plane, uint8_t* mask, uint8_t* prob8, uint8_t* votes, uint8_t* sel_votes,
                         unsigned long long* counts, void* stream);

/* ---- connected regions of a prediction mask ----------------------------------
 * A region of value v of a uint8 mask [H][W] is a maximal set of pixels equal to v connected under
 * connectivity 4 or 8; its label is 1 + y W + x of its first pixel in raster order. mask is a view: row y
 * starts mask_pitch bytes after row y - 1, at any alignment. All three calls: EINVAL for H or W < 1,
 * H * W >= 2^31 - 1, a pitch below W. Integer arithmetic and integer atomics only: every result is the
 * same bit for bit on every run. */
/* Labels the regions of `value`: local union-find per 64 x 64 tile, unions across the tile borders by
 * agent-scope atomic minima, then every pixel replaced by its root (three launches on `stream`).
 *   parent: uint32 [H][lp] scratch, lp = W rounded up to a multiple of 4; holds no result afterwards;
 *   labels: int32 [H][lp] = the label of the pixel's region, 0 where the pixel is not `value` and in the
 *     padding columns x >= W;
 *   roots: uint8 [H][lp] = 1 where the pixel is the first of its region, else 0;
 *   err: uint32 [1], caller-zeroed, |= 1 / 2 / 4 if a loop of the local / seam / flatten pass reached its
 *     iteration cap (never on an intact plane: the words of a chain strictly decrease);
 *   passes: 7 for a labelling; a subset of 1 local, 2 seam, 4 flatten launches only those (to time a pass:
 *     the passes of one labelling must then be issued in that order on one stream, with the same arguments).
 * Also EINVAL: passes outside [1, 7]; a null pointer; value outside [0, 255]; connectivity not 4 or 8; lp not W rounded up to 4;
 * H * lp >= 2^32 - 1; parent or labels not 16-B aligned, roots or err not 4-B aligned. */
int selunet_regions_label(const uint8_t* mask, int64_t mask_pitch, int32_t H, int32_t W, int32_t value,
                          int32_t connectivity, uint32_t* parent, int32_t* labels, uint8_t* roots,
                          int32_t lp, uint32_t* err, int32_t passes, void* stream);
/* The region table. labels: int32 rows of lp words as selunet_regions_label's; rowidx: int32 rows of rp
 * words holding, at the position (y, x) of every region's first pixel, the region's row in [0, n_rows).
 * table: uint64 [9][n_rows], columns {area, y_min, x_min, y_max, x_max, sum_y, sum_x, prob_sum,
 * abstain_contacts}; the caller sets the minima to a value >= H, W and the rest to 0. prob_sum sums prob8
 * (uint8 rows of prob_pitch bytes, nullable: the column is then left alone); abstain_contacts counts the
 * ordered pairs (pixel of the region, 4-neighbour inside the image) whose neighbour is 127 in `mask`.
 * A label outside [1, H W] or a row outside [0, n_rows) is skipped. Also EINVAL: null labels, mask, rowidx
 * or table; n_rows outside [1, H W]; labels or rowidx not 4-B aligned, table not 8-B aligned. */
int selunet_regions_stats(const int32_t* labels, int32_t lp, const uint8_t* mask, int64_t mask_pitch,
                          const uint8_t* prob8, int64_t prob_pitch, int32_t H, int32_t W,
                          const int32_t* rowidx, int32_t rp, int64_t n_rows, unsigned long long* table,
                          void* stream);
/* Rewrites the mask in place: a pixel of a region whose action[row] (uint8 [n_rows]) is 1 becomes 0, 2
 * becomes 255, 0 stays; pixels without a label stay. counts: uint64 [4], caller-zeroed, += {pixels equal
 * to 0, to 255, to 127, their sum} of the resulting mask. labels, rowidx and action all null: the mask is
 * only counted. Bytes outside the [H][W] view are neither read nor written. Also EINVAL: null mask or
 * counts; only some of labels, rowidx, action given; n_rows outside [1, H W]; labels or rowidx not 4-B
 * aligned; counts not 8-B aligned. */
int selunet_regions_apply(uint8_t* mask, int64_t mask_pitch, int32_t H, int32_t W, const int32_t* labels,
                          int32_t lp, const int32_t* rowidx, int32_t rp, const uint8_t* action,
                          int64_t n_rows, unsigned long long* counts, void* stream);

/* ---- tissue mask of whole-image prediction -------------------------------------
 * Bare glass is told from tissue per pixel by an exact integer rule, so that tiles whose whole input window
 * is glass need not be forwarded. A tissue plane is uint8, 0 for glass and anything else (255 as written
 * here) for tissue. Integer arithmetic only: every result is the same bit for bit on every run. */
/* img: uint8 [H][W][3] RGB on the device -> plane: uint8 [H][pitch]. A pixel is glass iff
 * min(r,g,b) >= bright and max(r,g,b) - min(r,g,b) <= spread; plane = 0 for glass, 255 for every other
 * pixel, 0 in the bytes x >= W of a row. EINVAL: a null pointer; H or W outside [1, 65535]; bright or spread
 * outside [0, 255]; pitch < W or pitch % 4 != 0; plane not 4-B aligned. */
int selunet_tissue_plane(const uint8_t* img, int32_t H, int32_t W, int32_t bright, int32_t spread,
                         uint8_t* plane, int32_t pitch, void* stream);
/* counts: int32 [n], caller-zeroed, counts[i] += the number of positions (y, x) of tile i's th x tw window
 * whose source pixel is tissue; the source pixel is selunet_tile_gather_flip's for `flip`: row
 * fy(refl(y0 + y, H)), column fx(refl(x0 + x, W)) of plane (rows of `pitch` bytes), so a reflected copy of a
 * pixel counts again. origins: DEVICE int32 [n][2] as selunet_tile_gather's. Integer atomics only.
 * EINVAL: a null pointer; the size and tile rules of selunet_tile_gather; pitch < W; flip outside [0, 3];
 * th * tw >= 2^31; counts not 4-B aligned. */
int selunet_tile_tissue_counts(const uint8_t* plane, int64_t pitch, int32_t H, int32_t W,
                               const int32_t* origins, int32_t n, int32_t th, int32_t tw, int32_t flip,
                               int32_t* counts, void* stream);
/* counts: uint64 [4], caller-zeroed, += {pixels equal to 0, to 255, to 127, their sum} of mask (uint8 rows of
 * mask_pitch bytes, at any alignment) over the pixels y < H, x < W that are tissue in plane (rows of `pitch`
 * bytes). Integer atomics only. EINVAL: a null pointer; H or W outside [1, 65535]; a pitch below W; counts
 * not 8-B aligned. */
int selunet_tissue_class_counts(const uint8_t* mask, int64_t mask_pitch, const uint8_t* plane, int64_t pitch,
                                int32_t H, int32_t W, unsigned long long* counts, void* stream);

/* ---- Macenko stain normalisation of whole-image prediction ----------------------
 * Four per-pixel passes over img, uint8 [H][W][3] RGB on the device; the caller does the linear algebra
 * between them. Integer arithmetic and integer atomics only: every result is the same bit for bit on every
 * run. Common to all four:
 *   od_q: DEVICE int32 [256], the optical density of a byte in Q12, round(4096 * -ln(max(v, 1) / 255));
 *     every entry must lie in [0, 2^15) (the overflow bounds below rest on it).
 *   A pixel is stained iff od_q of all three of its bytes is >= beta_q.
 *   B, P_q, T_q: HOST int32 arrays, row-major, read before the launch.
 *   Outputs of the first three are caller-zeroed and accumulated (+=), so several images can share them.
 * Common EINVAL: a null pointer; H or W outside [1, 65535]; od_q or dirs not 4-B aligned; a uint64 output
 * not 8-B aligned. */
#define SELUNET_STAIN_ANGLE_BINS 1024
#define SELUNET_STAIN_CONC_BINS 1024
#define SELUNET_STAIN_EXP_MAX 8192
/* out: uint64 [10] += {n, sum r, sum g, sum b, sum rr, sum rg, sum rb, sum gg, sum gb, sum bb} of the
 * optical densities (r, g, b) of the stained pixels. A product is < 2^30 and H W < 2^32: no overflow. */
int selunet_stain_moments(const uint8_t* img, int32_t H, int32_t W, const int32_t* od_q, int32_t beta_q,
                          unsigned long long* out, void* stream);
/* out: uint64 [SELUNET_STAIN_ANGLE_BINS + 1]. Per stained pixel x = B[0] . od and y = B[1] . od (B: int32
 * [2][3], two unit vectors in Q14); x <= 0 adds one to the last word ("skipped"), otherwise one to the bin
 * #{k in 1 .. K-1 : dirs[k-1][0] y - dirs[k-1][1] x >= 0}. dirs: DEVICE int32 [K-1][2] = round(2^14 (cos,
 * sin)) of theta_k = -pi/2 + k pi / K, which makes the predicate monotone in k (the kernel searches by
 * halving and relies on it); entries in [-2^14, 2^14]. Also EINVAL: a row of B whose sum of |B| reaches 2^16
 * (x and y are kept in 32 bits). */
int selunet_stain_angle_hist(const uint8_t* img, int32_t H, int32_t W, const int32_t* od_q, int32_t beta_q,
                             const int32_t* B, const int32_t* dirs, unsigned long long* out, void* stream);
/* out: uint64 [2][SELUNET_STAIN_CONC_BINS]. Per stained pixel and stain s, c = P_q[s] . od (P_q: int32
 * [2][3] in Q12, so c is Q24) adds one to bin clamp(c >> 17, 0, bins - 1) of row s: bins of 1/128. */
int selunet_stain_conc_hist(const uint8_t* img, int32_t H, int32_t W, const int32_t* od_q, int32_t beta_q,
                            const int32_t* P_q, unsigned long long* out, void* stream);
/* out: uint8 [H][W][3]. Every pixel, stained or not: out_c = exp_q[clamp((T_q[c] . od + 2^15) >> 16, 0,
 * n_exp - 1)] (T_q: int32 [3][3] in Q14; exp_q: DEVICE uint8 [n_exp], round(255 exp(-i / 1024))). Also
 * EINVAL: n_exp outside [1, SELUNET_STAIN_EXP_MAX]; an entry of T_q with |T_q| >= 2^20; out overlapping img. */
int selunet_stain_apply(const uint8_t* img, int32_t H, int32_t W, const int32_t* od_q, const int32_t* T_q,
                        const uint8_t* exp_q, int32_t n_exp, uint8_t* out, void* stream);

/* ---- multi-GPU overlap probe (bench/tools only, not on the training path) ------
 * Stand-in for one bucketed RCCL all-reduce kernel on a single GPU: n_wg workgroups of 256 threads
 * reduce-copy dst[i] += src[i] over their slices of [0, n) (n % 4 == 0, 16-B aligned), repeatedly,
 * until `us` microseconds of GPU wall clock have passed since each workgroup started — holding
 * n_wg CUs' worth of waves the way a ring all-reduce holds its channels. Issued on a side stream at
 * GradBucketer's bucket points by tools/overlap_emulation.py. */
int selunet_cu_hold(const float* src, float* dst, int64_t n, int32_t n_wg, float us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SELUNET_H */
