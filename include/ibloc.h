/*
 * ibloc.h -- C-ABI of libibloc_hip.so, the MI355X (gfx950) native implementation of the
 * embed -> match -> assign -> register hot path of instance-based-loc
 * (ObjectMemory.localise(), /root/reference/object_memory/object_memory.py:852-1169).
 *
 * The reference is pure Python and has no FFI of its own; every entry point below names the
 * reference interface (file:line under /root/reference) whose arithmetic it replaces.  The Python
 * host layer (instance-based-loc_amd/) binds these with ctypes and mirrors the reference's module
 * surface (utils.embeddings, utils.similarity_volume, utils.fpfh_register, object_memory).
 *
 * Conventions
 *   - every function returns an int32 status: 0 = OK, < 0 = error (ibl_last_error() has the text,
 *     thread-local).  No exception crosses the boundary.
 *   - the CALLER owns all memory.  Pointers marked [dev] are device (HBM) pointers, e.g.
 *     torch.Tensor.data_ptr(); pointers marked [host] are host pointers.  Workspace sizes come
 *     from the *_workspace_bytes() queries.  The library's own device memory is explicit: the arena of a registration context
 *     (scratch: every call releases what it took) and the arrays of a memory grid (ibl_memgrid_build .. ibl_memgrid_destroy).
 *   - all launches are asynchronous on the hipStream_t passed as `void* stream`
 *     (torch.cuda.current_stream().cuda_stream).  Functions whose results are DEVICE arrays (embed, match, candidate selection)
 *     never synchronise.  Functions that return HOST results synchronise the stream -- how often is stated per function:
 *     ibl_radius_outlier_batch 1 (grid table size), ibl_instance_features_batch 2 (bounding boxes; end),
 *     ibl_register_jobs 2-4 (one per group of RANSAC rounds -- most calls need one -- plus the results; one more when
 *     instances of a job lie within the influence radius of each other), ibl_evaluate_batch 1, ibl_evaluate_information 1, ibl_memgrid_overlap 1, ibl_memgrid_build / _append / _remove / _replace 2
 *     (cell count; end; one more when the call has to reallocate the other point buffer).  Plan tables are staged through pinned host memory of the registration context, so uploads never wait.
 *   - plain C types only; no torch types in any signature.
 */
#ifndef IBLOC_H
#define IBLOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* library                                                                                     */
/* ------------------------------------------------------------------------------------------ */
int ibl_version(void);
const char* ibl_last_error(void);

/* In-process kernel timer for the roofline line of bench.py: when enabled, selected kernel families are
 * bracketed by HIP events ON THEIR LAUNCH STREAM.  ibl_prof_read synchronises those events and returns the
 * accumulated device time, the accumulated algorithmic units (FLOPs or bytes, see csrc/ibl_common.h) and the
 * number of launches of family `id` (1 = fp16 GEMM, 3 = SPFH k-NN, ...). */
int ibl_prof_enable(int on);
int ibl_prof_read(int id, double* ms, double* units, int64_t* launches);

/* ------------------------------------------------------------------------------------------ */
/* embed: crop preprocessing + ViT encoder forward                       */
/* ------------------------------------------------------------------------------------------ */

#define IBL_VIT_MAX_LAYERS 32
#define IBL_VIT_LAYERSCALE 1      /* DINOv2 LayerScale (per-layer ls1/ls2 non-NULL)                */
#define IBL_VIT_PRE_LN 2          /* CLIP ln_pre on the embedded tokens                            */
#define IBL_VIT_FINAL_LN 4        /* final LayerNorm (DINOv2 / ViT layernorm, CLIP ln_post)        */
#define IBL_VIT_QUICK_GELU 8      /* fc1 activation x*sigmoid(1.702x) (OpenAI CLIP, open_clip *-quickgelu, transformers' default
                                     CLIPVisionConfig) in place of erf GELU (laion2b ViT-B-32)     */
#define IBL_VIT_PROJ 16           /* CLS -> out_dim projection (CLIP visual.proj)                  */
#define IBL_VIT_OUT_ALL_TOKENS 32 /* return every token (DATOR/TransReID local_feature=True)       */
#define IBL_VIT_ACT_TERMS2 64     /* some block has o_terms / fc2_terms = 2: attention output / hidden layer as rows of 2 terms  */
#define IBL_VIT_ACT_TERMS3 128    /* ... = 3: rows of 3 terms (sizes the workspace)                                             */
#define IBL_VIT_NO_CLS 256        /* no class token (SigLIP): n_tokens is the patch count, `patches` is [batch*n_tokens][patch_k_pad], patch p of crop b
                                     goes to row b*n_tokens + p, pos_patch has n_tokens rows and cls_pos is not read (may be NULL).  Needs
                                     IBL_VIT_OUT_ALL_TOKENS -- there is no row to return otherwise: refused with IBL_ERR_UNSUPPORTED before any launch */
#define IBL_VIT_TANH_GELU 512     /* fc1 activation 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) (gelu_pytorch_tanh: SigLIP) in place of erf GELU;
                                     together with IBL_VIT_QUICK_GELU it is refused                  */
#define IBL_VIT_SPLIT_SCALE 64.0f /* S of the two-term operands below                              */

typedef struct {
    int32_t dim, depth, heads, mlp_dim;
    int32_t patch, img_h, img_w;   /* model input size after preprocessing                          */
    int32_t n_tokens;              /* 1 + n_registers + (img_h/patch)*(img_w/patch); the patches alone with IBL_VIT_NO_CLS */
    int32_t patch_k_pad;           /* 3*patch*patch rounded up to a multiple of 64 (zero padded)    */
    int32_t flags;                 /* IBL_VIT_*                                                     */
    int32_t n_blocks_run;          /* blocks actually executed (DATOR runs depth-1)                 */
    int32_t out_dim;               /* dim, or the projection width                                  */
    float ln_eps;
    int32_t n_registers;           /* register tokens between the class row and the patch rows (DINOv2-reg, DINOv3: 4): a crop's rows are
                                      [cls, reg_0 .. reg_{R-1}, patch_0 ..].  0 = none, the forward of before the field existed bit for bit.
                                      Negative, or non-zero with IBL_VIT_NO_CLS, is refused before any launch */
} ibl_vit_desc;

typedef struct {                   /* all [dev]; weights fp16 [N][K] row-major (nn.Linear layout)   */
    const float* ln1_g; const float* ln1_b;
    const void* w_qkv;  const float* b_qkv;     /* [3*dim][dim] = [Wq; Wk; Wv], [3*dim]              */
    const void* w_o;    const float* b_o;       /* [dim][dim]                                         */
    const float* ls1;                            /* [dim] or NULL.  NULL is accepted (no LayerScale in the model, or ls1 multiplied into the
                                                  * rows of w_o and into b_o by the host, as ibloc_amd.vit can do) and runs the same
                                                  * read-modify-write residual GEMM with a scale of 1.  The form with the residual tile
                                                  * preloaded into the accumulators is opt-in ($IBL_GEMM_RESID_PRE=1) and measured ~2 %
                                                  * slower                                                                 */
    const float* ln2_g; const float* ln2_b;
    const void* w_fc1;  const float* b_fc1;     /* [mlp_dim][dim]                                     */
    const void* w_fc2;  const float* b_fc2;     /* [dim][mlp_dim]                                     */
    const float* ls2;
    /* Optional two-term fp16 operands (round 3; all NULL / 0 = plain fp16 operands, what rounds 1-2 ran).  With random-init
     * weights the first blocks carry most of the encoder's fp16 rounding error (the residual stream is still small there), so
     * the host may hand those blocks their weights as W = W_hi + W_lo (both fp16, W_lo stored times IBL_VIT_SPLIT_SCALE so it
     * stays a normal number) and ask for the LayerNorm output as a_hi + a_lo as well.  K-extended operand rows:
     *   terms 2: A' = [a_hi | a_hi / S],             W' = [W_hi | W_lo * S]              (weights exact to ~2^-22)
     *   terms 3: A' = [a_hi | a_lo * S | a_hi / S],  W' = [W_hi | W_hi / S | W_lo * S]   (+ the activation's second term)
     * one accumulation, same kernel, K' = terms * dim.  The two residual GEMMs (linear epilogue) take the second weight term
     * as a second launch that accumulates scale_lo[n] * (a W_lo'^T) into the residual (scale_lo = LayerScale / S, or 1 / S). */
    const void* w_qkv_x;                         /* fp16 [3*dim][qkv_terms*dim] or NULL                */
    const void* w_o_lo;  const float* ls1_lo;   /* fp16 [dim][dim] = W_lo * S; fp32 [dim] = ls1 / S, or NULL: the term is added with the
                                                  * factor 1 / S (no LayerScale, or LayerScale folded into W_o by the host)            */
    const void* w_fc1_x;                         /* fp16 [mlp_dim][fc1_terms*dim] or NULL              */
    const void* w_fc2_lo; const float* ls2_lo;  /* fp16 [dim][mlp_dim]; fp32 [dim]                    */
    int32_t qkv_terms, fc1_terms;                /* 1 (or 0), 2 or 3                                   */
    /* round 4: the two residual GEMMs with K-extended operands as well -- ONE launch of K' = terms * K instead of one read-modify-write pass
     * over the residual per term: the attention kernel / the fc1 epilogue write the rows [a_hi | a_hi / S] (terms 2) or
     * [a_hi | a_lo * S | a_hi / S] (terms 3: + the second fp16 term of the attention output / of the GELU hidden layer); w_o_x / w_fc2_x are laid
     * out like w_qkv_x.  Needs IBL_VIT_ACT_TERMS2 / 3 in the descriptor's flags.  With w_o_x / w_fc2_x NULL the older w_o_lo / w_fc2_lo launches run.
     * The terms of every block to run are checked before the first launch: a count above 3, or o_terms / fc2_terms above what the flags allow,
     * in ANY layer is refused (IBL_ERR_ARG) with the workspace and `out` untouched. */
    int32_t o_terms, fc2_terms;
    const void* w_o_x;                           /* fp16 [dim][o_terms*dim] or NULL                     */
    const void* w_fc2_x;                         /* fp16 [dim][fc2_terms*mlp_dim] or NULL               */
} ibl_vit_layer;

typedef struct {
    const void* w_patch;           /* fp16 [dim][patch_k_pad]: conv weight flattened (c, kh, kw)     */
    const float* b_patch;          /* [dim] or NULL                                                  */
    const float* cls_pos;          /* [dim]: cls_token + position_embedding[0]; not read with IBL_VIT_NO_CLS */
    const float* pos_patch;        /* [P][dim], P = n_tokens - 1 - n_registers patch tokens (n_tokens with IBL_VIT_NO_CLS): their position
                                      embeddings, already interpolated to the (img_h/patch, img_w/patch) grid.  Registers get none */
    const float* ln_pre_g; const float* ln_pre_b;
    const float* ln_f_g;   const float* ln_f_b;
    const void* w_proj;            /* fp16 [out_dim][dim] or NULL                                    */
    const void* w_patch_lo;        /* optional fp16 [dim][patch_k_pad] = (W - fp16(W)) * S: second term of the patch weights  */
    const void* w_proj_x;          /* optional fp16 [out_dim][3*dim] = [W_hi | W_hi / S | W_lo * S]: the projection with three-term
                                      operands (round 4: the final LayerNorm row is written as [a_hi | a_lo * S | a_hi / S]); the
                                      projection is the last arithmetic before the output, so its fp16 roundings are not attenuated
                                      by anything downstream (4e-4 of the embedding with plain operands) and it costs nothing     */
    ibl_vit_layer layers[IBL_VIT_MAX_LAYERS];
    const float* reg_tokens;       /* fp32 [n_registers][dim]: rows 1 .. n_registers of every crop; not read with n_registers = 0 */
    const float* rope_table;       /* fp32 [P][64] = [cos(32) | sin(32)] per patch, 16-byte aligned, or NULL: no rotation.  With a table
                                      every block rotates q and k of the patch rows in place between its QKV projection and its
                                      attention (ibl_rope_f16 below; DINOv3) */
} ibl_vit_weights;

/* One crop of a preprocessing batch.  The separable resample coefficient tables are the
 * fixed-point (22-bit) tables of Pillow's 8-bit resampler, computed on the host in float64
 * (instance-based-loc_amd/preprocess.py) so that the device arithmetic is pure integer and
 * bit-identical to PIL.Image.resize -- the resize every reference embedding function applies
 * through its HF / open_clip processor (utils/embeddings.py:41-42, 64-65, 86-89).
 * Table layout per pass: out_size records of (2 + ksize) int32 = [first_tap, n_taps, k0 .. ]. */
typedef struct {
    int64_t src_offset;            /* byte offset of the crop (HWC u8, 3 channels) in `src`          */
    int32_t in_h, in_w;
    int32_t h_table, h_ksize;      /* int32 index into `tables` of the horizontal pass, taps/record  */
    int32_t v_table, v_ksize;      /* vertical pass (NULL pass = identity: ksize 0)                  */
    int64_t tmp_offset;            /* byte offset of this crop's [in_h][out_w][3] scratch in `tmp`   */
} ibl_crop_desc;

/* One pass of Pillow's 8-bit resampler as a fixed-point table (host function; libImaging/Resample.c precompute_coeffs +
 * normalize_coeffs_8bpc restated): output samples [win0, win0 + win_n) of a resize in_size -> out_size.  rec: [HOST] win_n records of
 * (2 + ksize) int32 = [first tap, tap count, 22-bit weights ...]; ksize = ibl_resample_ksize(...).  Returns ksize (> 0) or a negative
 * status.  What the reference's HF / open_clip processors compute per crop on the CPU (utils/embeddings.py:41-42, 64-65, 86-89). */
#define IBL_FILTER_BILINEAR 0
#define IBL_FILTER_BICUBIC 1
int ibl_resample_ksize(int in_size, int out_size, int filter);
int ibl_resample_table(int in_size, int out_size, int filter, int win0, int win_n, int32_t* rec);

/* u8 crops -> (optional R<->B swap, utils/embeddings.py:41,64,86) -> PIL-exact resize ->
 * window (centre crop) -> ((u8/255) - mean) / std -> fp16 im2col patch matrix
 * [n_crops * (out_h/patch)*(out_w/patch)][patch_k_pad], k = c*patch*patch + kh*patch + kw.
 *   max_in_h: tallest crop of the batch (sizes the launch);
 *   src, tables, descs, tmp: [dev];  mean/stdv: 3 floats each (host), indexed by MODEL channel
 *   out_u8: optional [dev] n_crops x out_h x out_w x 3 resized+cropped u8 image (for parity tests) */
int ibl_preprocess_crops(const uint8_t* src, const ibl_crop_desc* descs, int n_crops, int max_in_h,
                         const int32_t* tables,
                         uint8_t* tmp, int out_h, int out_w, int patch, int patch_k_pad, int swap_rb,
                         const float* mean, const float* stdv, void* patches, uint8_t* out_u8, void* stream);

/* Native-aspect crops: the same preprocessing with a target size and a destination per crop.  Crop b (descs[b]: its tables are those of
 * an exact resize in_w -> out_w, in_h -> out_h, its scratch [in_h][out_w][3]) is resized to out_h x out_w, normalised and written as
 * (out_h / patch) * (out_w / patch) rows of the patch matrix from row row0 on -- for ibl_vit_forward_ragged row0 = seq_off[b] +
 * 1 + n_registers.  The whole matrix, fp16 [patch_rows][patch_k_pad], is cleared first: rows no crop writes (the prefix rows) and the K
 * padding are zero.  out_u8 (optional): crop b's out_h x out_w x 3 image at byte u8_offset.  The arithmetic per pixel is that of
 * ibl_preprocess_crops.  rdescs is given twice, [dev] for the kernels and [HOST] for the checks; the caller keeps them equal.
 * Enqueues on `stream` and synchronises nothing.  Refused (IBL_ERR_ARG) before anything is launched or cleared: null pointers (out_u8
 * may be NULL), sizes that are not positive multiples of `patch`, row0 (or, with out_u8, u8_offset) that does not ascend past the
 * previous crop's rows, rows beyond patch_rows, n_crops outside 1..65535. */
typedef struct {
    int32_t out_h, out_w;          /* target size in pixels: multiples of the patch size                */
    int64_t row0;                  /* first row of this crop's patches in the patch matrix              */
    int64_t u8_offset;             /* byte offset of this crop's image in out_u8                        */
} ibl_crop_ragged_desc;
int ibl_preprocess_crops_ragged(const uint8_t* src, const ibl_crop_desc* descs, const ibl_crop_ragged_desc* rdescs_dev,
                                const ibl_crop_ragged_desc* rdescs_host, int n_crops, int max_in_h, const int32_t* tables,
                                uint8_t* tmp, int patch, int patch_k_pad, int swap_rb, const float* mean, const float* stdv,
                                void* patches, int64_t patch_rows, uint8_t* out_u8, void* stream);

/* ViT forward over a batch of crops.  Replaces the batch-1 torch forward of
 * utils/embeddings.py:46,69,93 and dator/model/backbones/vit_pytorch.py:422-443.
 *   patches [dev] fp16 [batch*P][patch_k_pad], P = n_tokens - 1 - n_registers (from ibl_preprocess_crops; P = n_tokens with IBL_VIT_NO_CLS)
 *   out     [dev] fp32 [batch][out_dim]  (CLS embedding; un-normalised, like the reference), or
 *           fp32 [batch][n_tokens][dim] with IBL_VIT_OUT_ALL_TOKENS */
int64_t ibl_vit_workspace_bytes(const ibl_vit_desc* desc, int batch);
/* Where ibl_vit_forward keeps its intermediates in the caller's workspace (no device call): offsets [host] [n], n <= IBL_VIT_WS_COUNT,
 * byte offsets of the first n buffers below relative to the workspace pointer rounded up to 256 bytes; each on a 256-byte boundary, none
 * overlapping, the last one ending inside ibl_vit_workspace_bytes.  Refused (IBL_ERR_ARG): batch <= 0, a null pointer, n outside
 * 0..IBL_VIT_WS_COUNT.  With Rn = batch * n_tokens rows, D = dim, and k = n_blocks_run - 1 the last block run, a forward leaves:
 *   X    fp32 [Rn][D]           the residual stream after block k (after the patch embedding / ln_pre with n_blocks_run = 0)
 *   XN   fp16 [Rn][ft * D]      block k's second LayerNorm output in ft = fc1_terms column blocks [a | a / S] or [a | a_lo * S | a / S]
 *   QKV  fp16 [Rn][3 * D]       block k's [q | k | v]; with a rope_table q and k of the patch rows are the ROTATED ones the attention read
 *   ATT  fp16 [Rn][ot * D]      block k's attention output in ot = o_terms column blocks
 *   HID  fp16 [Rn][f2t * mlp]   block k's hidden layer after the activation in f2t = fc2_terms column blocks
 *   FIN  fp16 [batch][D]        not written by an all-token run
 * Where block k runs on the class rows alone (no IBL_VIT_OUT_ALL_TOKENS; one term everywhere, whatever the layer's *_terms say): XN
 * is the block's FIRST LayerNorm output [Rn][D]; QKV holds k and v of every row but q of the class rows (row b * n_tokens) only; ATT
 * [Rn][D] is written in the class rows only, in place; FIN is the second LayerNorm of the class rows, the MLP input; HID is
 * [batch][mlp], its first `batch` rows.  The projection then overwrites the head of a buffer: with w_proj_x XN becomes [batch][3 * D],
 * the final LayerNorm of the class rows in three terms; without it FIN becomes that LayerNorm in one term. */
enum { IBL_VIT_WS_X = 0, IBL_VIT_WS_XN, IBL_VIT_WS_QKV, IBL_VIT_WS_ATT, IBL_VIT_WS_HID, IBL_VIT_WS_FIN, IBL_VIT_WS_COUNT };
int ibl_vit_workspace_layout(const ibl_vit_desc* desc, int batch, int64_t* offsets, int n);
int ibl_vit_forward(const ibl_vit_desc* desc, const ibl_vit_weights* weights, const void* patches, int batch,
                    float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The forward over crops with different patch grids (native-aspect crops).  Crop b owns rows seq_off[b] .. seq_off[b + 1] - 1 of every
 * per-token buffer: 1 + n_registers prefix rows, then its gh * gw patches in row-major order; seq_off int32 [batch + 1] from 0, given
 * [dev] and [HOST] (kept equal by the caller), total = seq_off[batch].  desc->n_tokens, img_h and img_w are not read.
 *   patches  [dev] fp16 [total][patch_k_pad]: one row per TOKEN, the prefix rows zero (ibl_preprocess_crops_ragged)
 *   pos_rows [dev] fp32 [total][dim]: the position row of every token (a crop's table resampled to its grid; the prefix rows are not used)
 *   out      [dev] fp32 [batch][dim] (class rows), or fp32 [total][dim], packed like the input, with IBL_VIT_OUT_ALL_TOKENS
 * The launches are those of ibl_vit_forward with Rn = total and the attention of ibl_attention_ragged_f16; the class rows of the last
 * block are gathered to compact buffers.  A crop's result does not depend on the batch it runs in; a batch of equal grids gives
 * ibl_vit_forward's bits where that runs the streaming attention (n_tokens > 272).  Enqueues on `stream`, synchronises nothing.
 * Refused before anything is launched: IBL_ERR_UNSUPPORTED for weights->rope_table (DINOv3), IBL_VIT_NO_CLS (SigLIP), IBL_VIT_PROJ /
 * IBL_VIT_PRE_LN (CLIP) and the shapes ibl_vit_forward refuses; IBL_ERR_ARG for null or misaligned pointers, batch <= 0 or > 65535,
 * seq_off[0] != 0, a segment that is descending, has no patch row or exceeds IBL_ATT_STREAM_MAX_TOKENS, term counts the descriptor has
 * no room for, a workspace below ibl_vit_ragged_workspace_bytes(desc, total, batch) (-1 for arguments it cannot size). */
int64_t ibl_vit_ragged_workspace_bytes(const ibl_vit_desc* desc, int64_t total_tokens, int batch);
int ibl_vit_forward_ragged(const ibl_vit_desc* desc, const ibl_vit_weights* weights, const void* patches, const float* pos_rows,
                           const int32_t* seq_off_dev, const int32_t* seq_off_host, int batch, float* out, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* One linear layer of the encoder on its own: out = epilogue(x W^T + bias).  The nn.Linear of the reference's
 * encoders (transformers' ViTSelfAttention / ViTIntermediate / ViTOutput called from utils/embeddings.py:46,69,93).
 *   x [dev] fp16 [rows][ldx], W [dev] fp16 [n_out][ldw] (nn.Linear layout), bias [dev] fp32 [n_out] or NULL
 *   epilogue: IBL_LINEAR_F16 -> out fp16; IBL_LINEAR_GELU_F16 -> out = gelu(.) fp16 (erf form);
 *             IBL_LINEAR_RESID_F32 -> out fp32 += scale[n] * (.) (scale NULL = 1); IBL_LINEAR_F32 -> out fp32
 *   n_out % 128 == 0, n_in % 64 == 0, ldx / ldw / ldo in elements with 16-byte aligned rows */
enum { IBL_LINEAR_F16 = 0, IBL_LINEAR_GELU_F16 = 1, IBL_LINEAR_RESID_F32 = 2, IBL_LINEAR_PATCH_F32 = 3, IBL_LINEAR_F32 = 4,
       IBL_LINEAR_RESID_PRE_F32 = 5, IBL_LINEAR_GELU_F16_X2 = 6, IBL_LINEAR_GELU_F16_X3 = 7 };
int ibl_linear_f16(const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias, const float* scale,
                    int64_t rows, int n_out, int n_in, int epilogue, void* out, int64_t ldo, void* stream);

/* The same GEMM with every epilogue ibl_vit_forward runs (ibl_linear_f16 forwards here with its four).  y = x W^T, fp32 accumulation
 * of the fp16 operands; the kernel, the tile shape (256 x 256 persistent where n_out % 256 == 0 and rows >= 4096, else 128 x 128) and
 * the launch are those of the encoder.
 *   x, W, bias, ldx / ldw / ldo as for ibl_linear_f16; rows of x at and beyond `rows`, and columns beyond n_in, are never read
 *   epilogue IBL_LINEAR_F16 / _GELU_F16 / _RESID_F32 / _F32: as above
 *            IBL_LINEAR_PATCH_F32: the patch-embedding scatter.  Row r = b * patches_per_crop + p of x goes to row
 *                b * tokens_per_crop + 1 + p of out (fp32): out = y + bias + pos[p] (pos [dev] fp32 [patches_per_crop][n_out]), or, with
 *                accumulate = 1, out += alpha * (y + bias) (the second weight term; pos is not read).  Row 0 of every crop (the CLS
 *                token) and rows beyond patches_per_crop are not touched.  rows must be whole crops: a multiple of patches_per_crop
 *            IBL_LINEAR_RESID_PRE_F32: out fp32 = out + bias + alpha * y, with the tile of out preloaded into the accumulators as
 *                (out + bias) / alpha; selected here and nowhere else ($IBL_GEMM_RESID_PRE concerns ibl_vit_forward and ibl_linear_f16)
 *            IBL_LINEAR_GELU_F16_X2 / _X3: out fp16 [rows][ldo] of 2 / 3 column blocks of n_out: [h | h / S], [h | (value - h) * S | h / S]
 *                with h = gelu(y + bias) rounded to fp16 from the fp32 `value` (S = IBL_VIT_SPLIT_SCALE): ldo >= 2 / 3 * n_out
 *   activation is read by IBL_LINEAR_GELU_F16 / _X2 / _X3 only: IBL_ACT_GELU_ERF (0, what a zeroed descriptor asks for) is the erf form
 *   above, IBL_ACT_QUICK_GELU gelu(v) = v * sigmoid(1.702 v) (what IBL_VIT_QUICK_GELU runs in the encoder); the rest of the epilogue is the same
 *   scale is read by IBL_LINEAR_RESID_F32 only; alpha by IBL_LINEAR_RESID_PRE_F32 and by the accumulate form of the patch scatter, where it
 *   must be a positive power of two (the kernel divides and multiplies by it and both must be exact)
 *   rows 0 returns IBL_OK without a launch.  A null x / W / out, n_out % 128, n_in % 64, a stride shorter than its row or not a
 *   multiple of 8 elements, an alpha that is no positive power of two where it is read, patches_per_crop <= 0, tokens_per_crop <=
 *   patches_per_crop, part of a crop, pos NULL without accumulate, an unknown epilogue, an activation other than 0 / 1 and a non-zero
 *   activation with an epilogue that has none are refused with a status before any launch.  The field lies in what was the tail padding
 *   of the struct (its size stays 112): zero the descriptor before filling it, a garbage tail is refused, not obeyed. */
/* IBL_ACT_GELU_TANH (0.5 v (1 + tanh(sqrt(2/pi) (v + 0.044715 v^3))), what IBL_VIT_TANH_GELU runs in the encoder) is NOT taken by
 * ibl_linear_f16_ex, whose contract -- every activation other than 0 / 1 is refused -- stays as it was; it is an argument of
 * ibl_linear_f16_act below. */
enum { IBL_ACT_GELU_ERF = 0, IBL_ACT_QUICK_GELU = 1, IBL_ACT_GELU_TANH = 2 };
typedef struct {
    const void* x;  int64_t ldx;       /* fp16 [rows][ldx]                                              */
    const void* W;  int64_t ldw;       /* fp16 [n_out][ldw]                                             */
    const float* bias;                 /* [n_out] or NULL                                               */
    const float* scale;                /* [n_out] or NULL (IBL_LINEAR_RESID_F32)                        */
    const float* pos;                  /* [patches_per_crop][n_out] (IBL_LINEAR_PATCH_F32)              */
    void* out;      int64_t ldo;
    int64_t rows;
    int32_t n_out, n_in, epilogue;
    int32_t accumulate;                /* IBL_LINEAR_PATCH_F32: 0 or 1                                  */
    int32_t tokens_per_crop, patches_per_crop;
    float alpha;
    int32_t activation;                /* IBL_ACT_* (IBL_LINEAR_GELU_F16 / _X2 / _X3), 0 elsewhere       */
} ibl_linear_desc;
int ibl_linear_f16_ex(const ibl_linear_desc* desc, void* stream);

/* ibl_linear_f16_ex with the activation as an argument: IBL_ACT_GELU_ERF, IBL_ACT_QUICK_GELU or IBL_ACT_GELU_TANH.  Validation, kernel
 * and launch are those of ibl_linear_f16_ex; with activation 0 or 1 the result is that entry's bit for bit.  desc->activation must be 0
 * (the argument is the activation); a non-zero `activation` is accepted with IBL_LINEAR_GELU_F16 / _X2 / _X3 only; any other value, and
 * everything ibl_linear_f16_ex refuses, is refused with a status before any launch. */
int ibl_linear_f16_act(const ibl_linear_desc* desc, int activation, void* stream);

/* The encoder's attention on its own: out = softmax(q k^T / 8) v per (crop, head), head_dim 64 -- what transformers'
 * ViTSelfAttention / Dinov2SelfAttention and open_clip's nn.MultiheadAttention compute inside the encoders of
 * utils/embeddings.py:46,69,93.  The kernel and the key-tile tier (4 / 9 / 13 / 17 tiles of 16 keys) are those ibl_vit_forward runs.
 *   qkv [dev] fp16 [batch*n_tokens][3*dim] = [q | k | v], each [heads][64]; 16-byte aligned
 *   out [dev] fp16 [batch*n_tokens][terms*dim]; 8-byte aligned.  terms 1: the row a; 2: [a | a / S]; 3: [a | (value - a) * S | a / S]
 *       (S = IBL_VIT_SPLIT_SCALE, value = the fp32 result a was rounded from: the K-extended operand rows of the output projection)
 *   cls_only 1: only token 0 of every crop is a query (the encoder's last block); the other rows of out are not written
 *   dim == 64 * heads, 0 <= n_tokens <= 272, terms 1..3; batch or n_tokens 0 returns IBL_OK without a launch.  Everything else is
 *   refused with a status before anything is launched.  Longer rows run through ibl_attention_stream_f16 below. */
int ibl_attention_f16(const void* qkv, void* out, int batch, int n_tokens, int dim, int heads, int cls_only, int terms, void* stream);

/* Rotary position embedding of the encoder on its own (transformers' DINOv3 apply_rotary_pos_emb: rotate_half with the table tiled
 * twice), in place on the QKV buffer.  For every crop b, patch p (row b * n_tokens + n_prefix + p), head h, i in 0..31 and x in {q, k}:
 *     x'[i] = x[i] cos[p][i] - x[i + 32] sin[p][i]        x'[i + 32] = x[i + 32] cos[p][i] + x[i] sin[p][i]
 * in fp32 (one product rounded, then one fma), rounded once to fp16 and clamped to +-65504 like every other conversion here.
 *   qkv   [dev] fp16 [batch*n_tokens][3*dim] = [q | k | v], each [heads][64]; 16-byte aligned
 *   table [dev] fp32 [n_tokens - n_prefix][64] = [cos(32) | sin(32)] per patch; 16-byte aligned
 *   k_only 1: the q columns are left alone (the encoder's class-rows-only last block has q of the class rows only)
 * The n_prefix first rows of every crop, the v columns and everything past row batch * n_tokens are neither read nor written.  A crop's
 * result does not depend on the batch it runs in.  batch 0 or n_prefix == n_tokens returns IBL_OK without a launch.  Refused with a
 * status before any launch: dim != 64 * heads, n_prefix outside 0..n_tokens, negative sizes, k_only other than 0 / 1, null or
 * misaligned pointers, more work than one grid holds. */
int ibl_rope_f16(void* qkv, const float* table, int batch, int n_tokens, int n_prefix, int dim, int heads, int k_only, void* stream);

/* The same product for rows of any length up to IBL_ATT_STREAM_MAX_TOKENS: keys and values pass through LDS in chunks of 128 under an fp32
 * online softmax, one workgroup per (crop, head, block of 64 queries) -- the kernel ibl_vit_forward runs where n_tokens > 272 (CLIP
 * ViT-L/14@336: 577 tokens, DINOv2 at 448 / 518 px: 1025 / 1370).  Arguments, layouts, alignment and refusals as for
 * ibl_attention_f16, except 0 <= n_tokens <= IBL_ATT_STREAM_MAX_TOKENS; short rows are accepted too (the two entries agree within the
 * rounding of either, not bit for bit).  No atomics: a crop's rows do not depend on the batch it runs in, and cls_only row 0 is the
 * row 0 of the full run bit for bit. */
#define IBL_ATT_STREAM_MAX_TOKENS 8192
int ibl_attention_stream_f16(const void* qkv, void* out, int batch, int n_tokens, int dim, int heads, int cls_only, int terms,
                             void* stream);

/* The streaming attention over crops of different lengths, packed back to back: crop b owns rows seq_off[b] .. seq_off[b + 1] - 1 of
 * qkv fp16 [total][3 * dim] and out fp16 [total][terms * dim] (seq_off int32 [batch + 1], given twice: [dev] for the kernel, [HOST] for
 * the checks and the launch size; the caller keeps them equal).  The arithmetic per crop is ibl_attention_stream_f16's in its order, so
 * a crop's rows are those of that entry run on the crop alone, bit for bit, whatever its neighbours hold; cls_only 1 writes row
 * seq_off[b] of every crop only.  Rows outside every segment are neither read nor written.  Enqueues on `stream`, synchronises nothing.
 * batch 0 returns IBL_OK without a launch.  Refused with a status, nothing launched and out untouched: null or misaligned pointers
 * (qkv 16, out 8, seq_off 4 bytes), dim != 64 * heads, terms outside 1..3, cls_only outside 0 / 1, batch < 0 or > 65535, seq_off[0] < 0,
 * an empty or descending segment, a segment longer than IBL_ATT_STREAM_MAX_TOKENS. */
int ibl_attention_ragged_f16(const void* qkv, void* out, const int32_t* seq_off_dev, const int32_t* seq_off_host, int batch, int dim,
                             int heads, int cls_only, int terms, void* stream);

/* The encoder's LayerNorm on its own: out[r] = (x[r] - mean) / sqrt(var + eps) * gamma + beta over `dim` columns, biased variance
 * from a second pass over the centred row (torch.nn.LayerNorm as the reference's encoders call it).  The kernel and the launch are
 * those of ibl_vit_forward.
 *   x [dev] fp32 [n_rows][ld_x], gamma / beta [dev] fp32 [dim]; all 16-byte aligned
 *   out_kind IBL_LN_OUT_F32: out fp32 [n_rows][ld_out], 16-byte aligned; out == x (with ld_out == ld_x) normalises in place
 *            IBL_LN_OUT_F16 / _X2 / _X3: out fp16 [n_rows][ld_out] of 1 / 2 / 3 terms per row -- [a], [a | a / S],
 *            [a | (value - a) * S | a / S] as for ibl_attention_f16; 8-byte aligned, ld_out >= terms * dim
 *   dim a multiple of 4, <= 1024; ld_x >= dim; ld_x, ld_out multiples of 4 elements; eps >= 0; n_rows 0 returns IBL_OK without a
 *   launch.  Rows between the strides are neither read nor written.  x and out must not overlap except in the in-place form. */
enum { IBL_LN_OUT_F32 = 0, IBL_LN_OUT_F16 = 1, IBL_LN_OUT_F16_X2 = 2, IBL_LN_OUT_F16_X3 = 3 };
int ibl_layernorm_f32(const float* x, int64_t ld_x, int64_t n_rows, int dim, const float* gamma, const float* beta, float eps,
                      void* out, int64_t ld_out, int out_kind, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* DATOR RGB-D encoder                                                       */
/* ------------------------------------------------------------------------------------------ */

/* Fusion-head weights of build_FourDNet (dator/model/make_model.py:484-591), all [dev] fp32.  Linear weights are
 * [out][in] row-major; hyper-network convolution weights are repacked to [9 taps][in][out]. */
typedef struct {
    const float *proj_local_rgb_w, *proj_local_rgb_b, *proj_global_rgb_w, *proj_global_rgb_b, *merge_rgb_w, *merge_rgb_b;
    const float *proj_local_depth_w, *proj_local_depth_b, *proj_global_depth_w, *proj_global_depth_b, *merge_depth_w, *merge_depth_b;
    const float *Q_r_w, *Q_r_b, *V_r_w, *V_r_b, *Q_d_w, *Q_d_b, *V_d_w, *V_d_b;
    const float *r2r_sel_w, *r2r_sel_b, *r2r_aw_w, *r2r_aw_b, *r2r_ffn_w, *r2r_ffn_b, *r2r_norm_g, *r2r_norm_b;
    const float *d2d_sel_w, *d2d_sel_b, *d2d_aw_w, *d2d_aw_b, *d2d_ffn_w, *d2d_ffn_b, *d2d_norm_g, *d2d_norm_b;
    const float *d2r_sel_w, *d2r_sel_b, *d2r_aw_w, *d2r_aw_b, *d2r_ffn_w, *d2r_ffn_b, *d2r_norm_g, *d2r_norm_b;
    const float *r2d_sel_w, *r2d_sel_b, *r2d_aw_w, *r2d_aw_b, *r2d_ffn_w, *r2d_ffn_b, *r2d_norm_g, *r2d_norm_b;
    const float *hyper0_w, *hyper0_b, *hyper1_w, *hyper1_b, *hyper2_w, *hyper2_b, *hyper3_w, *hyper3_b;
} ibl_dator_head_weights;

/* build_FourDNet.forward after the two backbones (dator/model/make_model.py:676-843, eval mode):
 * rgb_tokens / depth_tokens [dev] fp32 [batch][129][768] (ibl_vit_forward with IBL_VIT_OUT_ALL_TOKENS on the TransReID
 * streams, 11 of 12 blocks, no final norm) -> out [dev] fp32 [batch][128].  Replaces get_dator_embeddings
 * (utils/embeddings.py:105-121) together with ibl_preprocess_crops / ibl_preprocess_depth. */
int64_t ibl_dator_head_workspace_bytes(int batch);
int ibl_dator_head_forward(const ibl_dator_head_weights* w, const float* rgb_tokens, const float* depth_tokens, int batch,
                           float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The fp32 buffers ibl_dator_head_forward carves out of its workspace, in carving order, and what each holds once a forward
 * pass has finished (R = batch * 128 token rows, row-major; the pass reads its offsets from the same table this query returns):
 *   FR, FD          [R][128]  the final RGB / depth features, after all four attentions
 *   GL              [batch][128], LP [R][128]  global (CLS) and local projections of the DEPTH side (the RGB side's are overwritten)
 *   CAT             [R][256]  [fd | fr]: the merged features of both sides before any attention (the hyper-network's input)
 *   H1 H2 H3 H4     [R][128], [R][32], [R][8], [R][2]  hyper-network activations (ReLU after the first three)
 *   RGB_F, DEPTH_F  [R]       the two gates (softmax over H4)
 *   Q_R V_R Q_D V_D [R][128]  queries / values, projected from the merged (un-updated) features
 *   SEL [R][48], AW [R][24], SAMP [R][128], FEAT [R][128]  of the LAST attention, R2D (queries Q_R, values V_D): selectors after
 *                   the sigmoid (x = first 24, y = last 24), attention LOGITS (the softmax is taken inside the sampler), the
 *                   sampled and weighted values, and the ffn output that is gated into FD */
enum {
    IBL_DATOR_WS_FR = 0, IBL_DATOR_WS_FD, IBL_DATOR_WS_GL, IBL_DATOR_WS_LP, IBL_DATOR_WS_CAT,
    IBL_DATOR_WS_H1, IBL_DATOR_WS_H2, IBL_DATOR_WS_H3, IBL_DATOR_WS_H4, IBL_DATOR_WS_RGB_F, IBL_DATOR_WS_DEPTH_F,
    IBL_DATOR_WS_Q_R, IBL_DATOR_WS_V_R, IBL_DATOR_WS_Q_D, IBL_DATOR_WS_V_D,
    IBL_DATOR_WS_SEL, IBL_DATOR_WS_AW, IBL_DATOR_WS_SAMP, IBL_DATOR_WS_FEAT, IBL_DATOR_WS_COUNT
};
/* offsets [host] [n], n <= IBL_DATOR_WS_COUNT: byte offsets of the first n buffers above, relative to the workspace pointer
 * rounded up to 256 bytes.  No device call. */
int ibl_dator_head_workspace_layout(int batch, int64_t* offsets, int n);

/* ------------------------------------------------------------------------------------------ */
/* SigLIP attention-pooling head (transformers' SiglipMultiheadAttentionPoolingHead)            */
/* ------------------------------------------------------------------------------------------ */

/* One learned probe attends over a crop's tokens.  The query is a constant, so the key and value projections over all tokens fold away:
 *   score[b][h][t] = x[b][t] . u[h],  u[h] = W_k,h^T q_h / sqrt(head_dim)   (host, float64; q_h . b_k,h is constant over t and cancels)
 *   p = softmax_t(score),  pooled[b][h] = sum_t p[b][h][t] x[b][t]           (then W_v,h pooled[b][h] + b_v,h per head)
 * ibl_probe_pool_f32 is that kernel alone, fp32 throughout: one workgroup per crop, u and the probabilities in LDS, every reduction in a
 * fixed order without floating-point atomics -- a crop's result does not depend on the batch it runs in, bit for bit.
 *   x      [dev] fp32 [batch][n_tokens][dim], 16-byte aligned       u [dev] fp32 [heads][dim], 16-byte aligned
 *   pooled [dev] fp32 [batch][heads][dim], 16-byte aligned          probs [dev] fp32 [batch][heads][n_tokens] or NULL (same pooled either way)
 * batch >= 1, n_tokens >= 1, heads in 1..16, dim % 4 == 0, dim <= 1024, dim % heads == 0, heads * (dim + n_tokens) * 4 bytes within the
 * 160 KiB of LDS; null pointers and everything else are refused with a status before any launch and leave the outputs untouched. */
int ibl_probe_pool_f32(const float* x, int batch, int n_tokens, int dim, int heads, const float* u, float* pooled, float* probs, void* stream);

typedef struct {
    int32_t dim, heads, mlp_dim, n_tokens;
    float ln_eps;
} ibl_probe_head_desc;

typedef struct {                   /* all [dev] fp32; linear weights [out][in] row-major (nn.Linear layout) */
    const float* u;                /* [heads][dim], see above                                        */
    const float* w_v; const float* b_v;       /* [dim][dim], [dim]: rows h*head_dim .. of in_proj_weight's value part (head h reads pooled[b][h]) */
    const float* w_o; const float* b_o;       /* [dim][dim], [dim]: attention.out_proj                */
    const float* ln_g; const float* ln_b;     /* [dim]: head.layernorm                                */
    const float* w_fc1; const float* b_fc1;   /* [mlp_dim][dim], [mlp_dim]: head.mlp.fc1 (tanh GELU behind it) */
    const float* w_fc2; const float* b_fc2;   /* [dim][mlp_dim], [dim]: head.mlp.fc2                  */
} ibl_probe_head_weights;

/* The whole head: tokens [dev] fp32 [batch][n_tokens][dim] (ibl_vit_forward with IBL_VIT_OUT_ALL_TOKENS | IBL_VIT_FINAL_LN) ->
 * out [dev] fp32 [batch][dim] = a + fc2(gelu_tanh(fc1(LayerNorm(a)))), a = out_proj(concat_h(W_v,h pooled_h + b_v,h)): the model's
 * pooler_output, un-normalised.  fp32 throughout (the head is the last arithmetic before the output).  A row's result does not depend on
 * batch.  The limits of ibl_probe_pool_f32 apply; mlp_dim a positive multiple of 4; tokens, u and the four weight matrices 16-byte aligned; a
 * workspace smaller than ibl_probe_head_workspace_bytes is refused. */
int64_t ibl_probe_head_workspace_bytes(const ibl_probe_head_desc* desc, int batch);
int ibl_probe_head_forward(const ibl_probe_head_desc* desc, const ibl_probe_head_weights* weights, const float* tokens, int batch,
                           float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* The fp32 buffers ibl_probe_head_forward carves out of its workspace, in carving order, and what each holds after a forward pass:
 *   PROBS [batch][heads][n_tokens], POOLED [batch][heads][dim], VCAT [batch][dim] (per-head value projections, concatenated),
 *   ATT [batch][dim] (out_proj: the residual), LN [batch][dim], HID [batch][mlp_dim] (after the activation)
 * offsets [host] [n], n <= IBL_PROBE_WS_COUNT: byte offsets relative to the workspace pointer rounded up to 256 bytes.  No device call. */
enum { IBL_PROBE_WS_PROBS = 0, IBL_PROBE_WS_POOLED, IBL_PROBE_WS_VCAT, IBL_PROBE_WS_ATT, IBL_PROBE_WS_LN, IBL_PROBE_WS_HID, IBL_PROBE_WS_COUNT };
int ibl_probe_head_workspace_layout(const ibl_probe_head_desc* desc, int batch, int64_t* offsets, int n);

/* Depth crops (float, [dev], crop i = sizes[2i] x sizes[2i+1] floats at src + offsets[i]) -> fp16 patch matrix of the
 * depth stream: bilinear resize to out_h x out_w (cv2.INTER_LINEAR convention), clip [dmin, dmax], (d - dmin)/(dmax - dmin),
 * (x - 0.5)/0.5, three identical channels (dator/get_embeds.py:129-136; the reference's dator_wrapper is missing). */
int ibl_preprocess_depth(const float* src, const int64_t* offsets, const int32_t* sizes, int n_crops, int out_h, int out_w,
                         int patch, int patch_k_pad, float dmin, float dmax, void* patches, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* match: L2 normalisation + closest-similarity matrix                 */
/* ------------------------------------------------------------------------------------------ */

/* Row-wise L2 normalisation, fp32.  Replaces `e/np.linalg.norm(e)` and
 * `detected_embs /= np.linalg.norm(detected_embs, axis=-1, keepdims=True)`
 * (object_memory/object_memory.py:922,924).  Summation order is fixed (64 strided partial sums
 * with fmaf, xor-butterfly 32..1, IEEE sqrt and divide) so that oracle/ reproduces it bit-exactly.
 * in/out: [dev] n_rows x dim (row stride = dim), may alias. */
int ibl_normalize_rows(const float* in, float* out, int64_t n_rows, int dim, void* stream);

/* Closest-similarity matrix: S[q][j] = max_e <mem[e], det[q]> over the stored embeddings
 * e in [emb_offsets[j], emb_offsets[j+1]) of instance j.  Replaces the Python double loop
 * object_memory/object_memory.py:933-936.  Inputs must already be L2-normalised.
 *   det         [dev] n_query x dim fp32
 *   mem         [dev] n_mem_rows x dim fp32       (all stored embeddings, instance-major)
 *   emb_offsets [dev] (n_inst + 1) int32, emb_offsets[0] = 0, emb_offsets[n_inst] = n_mem_rows
 *   out_sims    [dev] n_query x n_inst fp32 or NULL
 *   out_aug     [dev] n_query x (n_inst + 1) IEEE binary16 bits or NULL: the reference's
 *               `aug = [sims | 1]` cast to float16 (utils/similarity_volume.py:13-18)
 *   workspace   [dev] ibl_closest_similarity_workspace_bytes() bytes
 * The dot product is computed on the fp32-input MFMA (v_mfma_f32_32x32x2_f32), which is a
 * k-ordered fmaf chain; the k order is the fixed permutation documented in DESIGN.md and
 * restated by oracle/, so the result is bit-exact against the oracle. dim % 8 == 0 required. */
int64_t ibl_closest_similarity_workspace_bytes(int64_t n_query, int64_t n_mem_rows);
int ibl_closest_similarity(const float* det, int64_t n_query, const float* mem, int64_t n_mem_rows,
                           const int32_t* emb_offsets, int64_t n_inst, int dim, float* out_sims,
                           uint16_t* out_aug, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-row two-ended candidate selection on the fp16 rows `aug` ([sims | 1], ld >= n_cols + 1 halves per row): the k_hi largest and
 * the k_lo smallest of the first n_cols entries of every row under the total order (value, then lower column first) -- the order
 * np.argmax's tie rule induces in utils/similarity_volume.py:219-225 -- sorted, as
 *   out_val [dev] n_rows x (k_hi + k_lo) IEEE binary16 bits, out_idx [dev] n_rows x (k_hi + k_lo) int32 = index_base + column,
 *   out_cnt [dev] n_rows x 2 int32 = (entries of the high list, entries of the low list).
 * A row with n_cols <= k_hi + k_lo is returned whole in the high list (count n_cols, 0).  k_hi, k_lo <= 256.  Only these lists leave
 * the GPU (8 bytes per entry instead of the 2 (M + 1)-byte row) or cross xGMI when the memory is sharded by instance range
 * (index_base = first instance of the shard).  ibl_assign_candidates runs the assignment search on them. */
int ibl_topk_select(const uint16_t* aug, int64_t n_rows, int64_t ld, int n_cols, int k_hi, int k_lo, int index_base,
                    uint16_t* out_val, int32_t* out_idx, int32_t* out_cnt, void* stream);

/* ibl_closest_similarity + ibl_topk_select in one call (SURVEY §8b `ibl_match_topk`): query rows against this rank's memory rows,
 * the candidates of every row with GLOBAL instance indices.  out_aug [dev] n_query x (n_inst + 1) or NULL (kept in the workspace).
 * Replaces object_memory/object_memory.py:933-936 and the cast of utils/similarity_volume.py:13-18 for a memory shard. */
int64_t ibl_match_topk_workspace_bytes(int64_t n_query, int64_t n_mem_rows, int64_t n_inst);
int ibl_match_topk(const float* det, int64_t n_query, const float* mem, int64_t n_mem_rows, const int32_t* emb_offsets, int64_t n_inst,
                   int dim, int k_hi, int k_lo, int index_base, uint16_t* out_val, int32_t* out_idx, int32_t* out_cnt, uint16_t* out_aug,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* assign: exact similarity-volume search                                   */
/* ------------------------------------------------------------------------------------------ */

/* Replaces SimVolume(sims).fast_construct_volume(min(Q,3)) +
 * .get_top_indices_from_subvolumes(num_per_length)  (utils/similarity_volume.py:13-18,102-164,
 * 213-270; called at object_memory/object_memory.py:974-982).  Bit-exact assignment lists
 * without materialising the (M+1)^3 volumes.  Host function (integer / fp16 index logic).
 *   aug_half     [host] n_frames x q_stride x (M+1) IEEE binary16 bits ([sims | 1])
 *   q_per_frame  [host] n_frames, number of valid detection rows of each frame (<= q_stride)
 *   out_assn     [host] n_frames x max_assn x 3 x 2 int32: (detection idx, memory idx), -1 padded
 *   out_len      [host] n_frames x max_assn: pairs in each assignment (1..3)
 *   out_count    [host] n_frames: assignments of each frame (<= 6)
 *   max_assn     >= 6;  n_threads: host threads to spread frames over. */
int ibl_assign_batch(const uint16_t* aug_half, const int32_t* q_per_frame, int n_frames, int q_stride,
                     int M, int num_per_length, int32_t* out_assn, int32_t* out_len, int32_t* out_count,
                     int max_assn, int n_threads);

/* The same search on per-row candidate lists (ibl_topk_select / ibl_match_topk, possibly the union of the lists of several memory
 * shards after the all-gather): row r has cand_cnt[r] entries (value bits, global column) at cand_val / cand_idx + r * cand_stride,
 * in any order; frame f owns the rows row_first[f] .. row_first[f] + q_per_frame[f] - 1 (q <= 7).  M_total = instances of the whole
 * memory; k_hi / k_lo = the list sizes every producer used (they define what a producer may have dropped: entries between its
 * k_lo-th smallest and k_hi-th largest).  The search runs on the union of the rows' candidate columns and PROVES per frame that no
 * dropped entry could have reached the k-th best cell of any sub-volume (the chained fp16 product is monotone in every coordinate,
 * so its maximum over the dropped range is attained at a corner: csrc/assign.cpp).  out_exact[f] = 1: the list equals
 * ibl_assign_batch on the full rows; 0: the proof failed (ties at the candidate threshold) and the caller redoes the frame on
 * full rows.  All pointers [host]. */
int ibl_assign_candidates(const uint16_t* cand_val, const int32_t* cand_idx, const int32_t* cand_cnt, int64_t cand_stride,
                          const int32_t* row_first, const int32_t* q_per_frame, int n_frames, int M_total, int k_hi, int k_lo,
                          int num_per_length, int32_t* out_assn, int32_t* out_len, int32_t* out_count, uint8_t* out_exact,
                          int max_assn, int n_threads);

/* ------------------------------------------------------------------------------------------ */
/* exchange: the collectives of the sharded path on RCCL                      */
/* ------------------------------------------------------------------------------------------ */

/* The reference issues no collective on this path (one process); with the memory sharded by instance range over the GPUs of a node
 * two are needed: the all-gather of the per-shard candidate lists before the assignment search (north star) and the all-reduce(MIN)
 * of per-point nearest distances for evaluate_transform against sharded clouds.  One communicator per process / GPU:
 * ibl_comm_unique_id on rank 0 (returns the id size, 128 bytes), the id reaches the other ranks through the host's own channel,
 * ibl_comm_init on every rank (current HIP device), then the collectives on the caller's stream.  The Python layer can use
 * torch.distributed (the same RCCL) instead: ibloc_amd.parallel. */
typedef struct ibl_comm ibl_comm;
int ibl_comm_unique_id(void* out, int out_bytes);
int ibl_comm_init(ibl_comm** out, int rank, int world, const void* unique_id, int id_bytes);
int ibl_comm_destroy(ibl_comm* comm);
/* recv [dev] world x bytes_per_rank: the contribution of rank r at offset r * bytes_per_rank */
int ibl_allgather_topk(ibl_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
/* Equal-block all-to-all (ncclSend / ncclRecv pairs in one group): block r of `send` ([world][bytes_per_pair]) goes to rank r, block r
 * of `recv` comes from rank r.  The exchange of the per-shard candidate lists since round 3: the owner of a query row receives the
 * `world` lists of that row and nothing else (the all-gather above delivered every rank's lists to every rank). */
int ibl_alltoall(ibl_comm* comm, const void* send, void* recv, int64_t bytes_per_pair, void* stream);
/* in place, element-wise minimum over the ranks of n floats (the d2_out distances of ibl_evaluate_batch) */
int ibl_allreduce_min(ibl_comm* comm, float* buf, int64_t n, void* stream);
/* in place, element-wise maximum of n int32 (the "some rank needs the full rows" flag of a step) */
int ibl_allreduce_max_i32(ibl_comm* comm, int32_t* buf, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* register: grids, normals + FPFH, feature matching, RANSAC, coloured ICP (rows a9-a13)        */
/* ------------------------------------------------------------------------------------------ */

/* Registration context: one device arena (bump allocator) that the batched calls carve their
 * grids, neighbour lists and per-job state from, as scratch: every call releases what it took.
 * Created and destroyed explicitly.  Not thread-safe: one context per stream/thread. */
typedef struct ibl_reg_ctx ibl_reg_ctx;
int ibl_reg_ctx_create(ibl_reg_ctx** out, int64_t arena_bytes);
int ibl_reg_ctx_destroy(ibl_reg_ctx* ctx);
/* drop every allocation of the arena (between calls nothing is held; memory grids own their arrays and stay valid) */
int ibl_reg_ctx_reset(ibl_reg_ctx* ctx);
int64_t ibl_reg_ctx_high_water(const ibl_reg_ctx* ctx);
/* device status word (bit 0: grid table overflow, bit 1: a k-NN query took the re-scan slow path; bits 2-3 are internal to
 * ibl_register_jobs; bits 4 / 5, informational: a registration call since the last clear was redone with the VALU feature
 * search / with a full-size RANSAC survivor list after the fast path's list overflowed -- same results, more time); synchronises the
 * device */
int ibl_reg_ctx_status(ibl_reg_ctx* ctx, int clear);
/* Diagnostic switches of a context, by name.  All are numbers; a flag is on when it is not 0.
 *   name            default  meaning
 *   knn_safety      1.1      tile k-NN grids: a ball of knn_rho cells holds knn_safety x max_nn points at the cloud's mean density
 *   knn_rho         3        tile k-NN grids: cells a tile's staging cube reaches past the tile (clamped to 1..4)
 *   knn_noguess     0        flag: the two-pass histogram selection for every k-NN query instead of the guessed threshold
 *   knn_debug       0        flag: print how many queries of each tile search fell back to the grid walk (synchronises)
 *   feat_unfused    0        flag: normals and FPFH from two neighbour searches instead of one
 *   feat_valu       0        flag: the VALU feature search of the registration instead of the matrix-core one
 *   feat_cand_cap   0        entries of the matrix-core search's candidate list (>= 1), 0 = sized by the call; a small one forces the
 *                            overflow fallback
 *   feat_p1_stride  2        pass 1 of the matrix-core search visits one database chunk in feat_p1_stride (>= 1)
 *   spfh_f64        0        flag: every SPFH pair in fp64 instead of fp32 bins + fp64 for the undecided pairs
 *   spfh_qcap       0        entries per queue of undecided SPFH pairs (>= 1), 0 = sized by the call; a small one forces the overflow path
 *   spfh_stats      0        flag: print the undecided SPFH pairs of every batch (synchronises)
 *   eval_fullscan   0        flag: the evaluation reads every cell of a query's box instead of pruning by the best distance so far
 *   timing          0        level: 1 prints the host-synchronised phase times of a registration call, 2 also synchronises and checks
 *                            for errors after every launch group of its feature search
 * Every switch except knn_safety, knn_rho and feat_p1_stride must leave every output bit unchanged: each selects another path to the
 * same result, or only prints.  Those three dimension work and leave the results unchanged as well, but are for measurements, not
 * for comparisons.  ibl_reg_ctx_create sets every switch whose environment variable IBL_<NAME IN UPPER CASE> exists (IBL_TIMING=1,
 * IBL_KNN_RHO=2, ...) to its value; the environment is not read again.  After that the switches of a context are set by the thread
 * that owns the context, between calls.  Both functions return the argument error (-1) and change nothing for an unknown name, a null argument
 * or a value that is not finite; the setter clamps as listed. */
int ibl_reg_ctx_set_diag(ibl_reg_ctx* ctx, const char* name, double value);
int ibl_reg_ctx_get_diag(const ibl_reg_ctx* ctx, const char* name, double* value);

/* Clouds are passed as batches of segments: pts4 [dev] N x float4 (x, y, z, intensity =
 * (r+g+b)/3), seg_off [dev] and [host] copies of the (n_seg + 1) int32 segment boundaries.  The registration calls take such a batch
 * as one ibl_cloud_pool (below, after ibl_instance_features). */

/* Depth image + instance masks -> one coloured cloud per mask.  Replaces
 * get_mask_coloured_pointclouds_from_depth / get_coloured_pointcloud_from_depth (utils/depth_utils.py:176-206, 46-90)
 * before their outlier step (-> ibl_radius_outlier_batch): the reference's centred pixel grid
 *     x = linspace(-W/2, W/2, W)[col] * z / fx,   y = linspace(H/2, -H/2, H)[row] * z / fy,   z = depth / depth_factor
 * (float32 linspace values, utils/depth_utils.py:57-67, whose `w, h` names are swapped), pixels with z == 0 or outside the
 * mask dropped, row-major pixel order kept, intensity = mean of the float32 colours / 255.  The arithmetic type follows
 * numpy's promotion of the reference's expressions: a float32 depth image stays in float32 throughout, an integer or
 * float64 one promotes the products to float64 (then rounded to the float32 of the HBM layout).
 *   depth [dev] H x W; depth_type IBL_DEPTH_F32 / IBL_DEPTH_U16 / IBL_DEPTH_F64; rgb [dev] H x W x 3 u8; masks [dev] n_masks x H x W u8
 *   pts4 [dev] capacity x float4 (n_masks * H * W always suffices), seg_off_dev [dev] / seg_off_host [HOST] n_masks + 1
 * Additionally, on request, the clouds as the reference's Open3D containers hold them for the memory build (process_image,
 * object_memory/object_memory.py:163-256): pts3_f64 / colors3_f64 [dev] capacity x 3 doubles, each or NULL = the numpy values (float32
 * or float64 by the promotion rule above; colours = float32 rgb / 255) widened to double, same order as pts4.
 * The call synchronises (the cloud sizes are returned to the host). */
enum { IBL_DEPTH_F32 = 0, IBL_DEPTH_U16 = 1, IBL_DEPTH_F64 = 2 };
int ibl_unproject_masks(ibl_reg_ctx* ctx, const void* depth, int depth_type, const uint8_t* rgb, const uint8_t* masks, int n_masks,
                        int H, int W, double fx, double fy, double depth_factor, float* pts4, double* pts3_f64, double* colors3_f64,
                        int64_t capacity, int32_t* seg_off_dev, int32_t* seg_off_host, void* stream);

/* keep[i] = 1 iff the point has more than nb_points points (itself included) within `radius` of its
 * own cloud.  Replaces PointCloud.remove_radius_outlier (object_memory/object_memory.py:994-995,
 * utils/depth_utils.py:87-88).  keep: [dev] N bytes. */
int ibl_radius_outlier_batch(ibl_reg_ctx* ctx, const float* pts4, const int32_t* seg_off_dev, const int32_t* seg_off_host,
                             int n_seg, double radius, int nb_points, uint8_t* keep, void* stream);

/* Normals (hybrid radius_normal / max_nn_normal, Open3D fast 3x3 eigen solver, no orientation) and
 * FPFH (hybrid radius_feature / max_nn_feature) of every cloud of the batch.  Replaces
 * downsample_and_compute_fpfh (utils/fpfh_register.py:86-98).  normals4: [dev] N x float4,
 * fpfh: [dev] N x 33 fp32 (point-major) or NULL to skip the features.  When radius_normal <= radius_feature and max_nn_normal <=
 * min(max_nn_feature, 32) -- the reference's 2 / 5 voxel, 30 / 100 neighbours -- ONE neighbour search serves both (the normal's
 * neighbours are among the feature neighbours); the results are those of the two searches bit for bit (switch feat_unfused runs them). */
int ibl_normals_fpfh_batch(ibl_reg_ctx* ctx, const float* pts4, const int32_t* seg_off_dev, const int32_t* seg_off_host,
                           int n_seg, double radius_normal, int max_nn_normal, double radius_feature, int max_nn_feature,
                           float* normals4, float* fpfh, void* stream);

/* Per-instance registration features, computed ONCE per cloud and kept resident in HBM instead of once per
 * (frame, assignment) job: the reference re-runs estimate_normals / compute_fpfh_feature
 * (utils/fpfh_register.py:86-98) and the colour gradients inside registration_colored_icp
 * (utils/fpfh_register.py:125-133) on the concatenated clouds of every assignment (object_memory.py:1023-1034,
 * 1087-1089), although a memory instance never changes and a detected instance is shared by all assignments of its
 * frame.  Normals, FPFH and colour gradients only depend on point differences, so they are evaluated in the frame
 * the clouds are stored in (before the per-job centring) and the value at a point of instance A inside a
 * concatenation A+B+C equals its stand-alone value unless a point of B or C lies within the influence radius
 *     R = max(2 * 5 * voxel + 2 * voxel, grad_radius + 2 * voxel)
 * of A.  ibl_register_jobs uses the stored values for every instance none of whose points is within R (plus a
 * rounding margin) of a point of another instance of its job side -- bounding boxes first, then an exact point-set test
 * on the device for the box pairs that are close -- and recomputes the rest in the context of the job's concatenation,
 * which makes its results bit-identical to those with features == NULL.
 *   normals4 [dev] N x float4, fpfh [dev] N x 33 with every row in MATCHING ORDER (bin 11 b + c at position
 *   3 * rank(c) + {b=1: 0, b=2: 1, b=0: 2}, rank over c = 5,4,6,3,7,2,8,1,9,0,10: the three histograms from their centre
 *   bins outwards, interleaved -- the order in which the feature search sums its squared differences, so that its
 *   early-abandon chain reads contiguously), fpfh_split / fpfh_norm [dev]: every row once more, CENTRED (x = row - a constant table, FM_MU of
 *   csrc/reg_common.h), as 48 fp16 search operands
 *   [x_0 .. x_32 | 8 8 | |x|^2 / 8 as hi + lo | 1e-3 |x|^2 + 4e-3 rounded up | 0 ..] and its squared norm -- the operands of the
 *   matrix-core filter of the feature search, whose one MFMA chain yields the whole distance bound (csrc/reg_featnn.hip), grad4 [dev] N x float4 or NULL (grad_radius <= 0: targets'
 *   gradients are recomputed per job), bbox [HOST] n_seg x 6 = (min xyz, max xyz) -- all written by
 *   ibl_instance_features_batch (the call synchronises); voxel_size / grad_radius: the parameters they hold for
 *   (grad_radius = 2 * voxel_size * local_dist_factor in register_point_clouds). */
typedef struct {
    const float* normals4;
    const float* fpfh;
    const uint16_t* fpfh_split;   /* [dev] N x 48 fp16 search operands (layout above), or NULL: COMPACT features (168 instead of 264
                                   * bytes per point) -- the search builds the same operands from fpfh / fpfh_norm as it stages them */
    const float* fpfh_norm;       /* [dev] N: |centred row|^2 */
    const float* grad4;
    const float* bbox;
    double voxel_size;
    double grad_radius;
} ibl_instance_features;
int ibl_instance_features_batch(ibl_reg_ctx* ctx, const float* pts4, const int32_t* seg_off_dev, const int32_t* seg_off_host,
                                int n_seg, double voxel_size, double grad_radius, float* normals4, float* fpfh, uint16_t* fpfh_split,
                                float* fpfh_norm, float* grad4, float* bbox_host, void* stream);

/* The arguments of the registration calls, named once. */
typedef struct {                 /* a batch of clouds */
    const float* pts4;           /* [dev] N x float4 */
    const int32_t* off_dev;      /* [dev]  n_seg + 1 */
    const int32_t* off_host;     /* [HOST] n_seg + 1 */
    const ibl_instance_features* features;   /* or NULL: none, every instance is recomputed per job */
    int32_t n_seg;
} ibl_cloud_pool;

#define IBL_REG_HAVE_COLORS 1
#define IBL_REG_CENTER 2
#define IBL_REG_FIXED_BUDGET 4   /* RANSAC walks exactly ransac_max_iter hypotheses per job (confidence exit off): the fixed-budget
                                    hypotheses/s figure of the benchmark, never the product setting */
typedef struct {
    double voxel_size, global_dist_factor, local_dist_factor;
    uint64_t seed;
    int64_t ransac_max_iter;
    uint32_t job_id_base;        /* used when job_ids == NULL */
    int32_t flags;               /* IBL_REG_* */
} ibl_register_params;

typedef struct {                 /* HOST arrays, [n_jobs] rows each; which may be NULL is stated at ibl_register_jobs */
    double *T, *rmse, *fitness, *means, *T_ransac;
    int64_t *ransac_stats, *reuse_stats;
} ibl_register_out;

/* Batched register_point_clouds (utils/fpfh_register.py:100-143) over n_jobs (frame, assignment) jobs.
 * Job j registers the concatenation of up to three segments of the detected pool `det` (job_src_seg[3j..],
 * -1 padded) onto the concatenation of up to three segments of the memory pool `mem` (job_tgt_seg), exactly
 * like object_memory/object_memory.py:1023-1034,1087-1089:
 *   IBL_REG_CENTER      subtract each side's mean first (localise does; the stand-alone function does not)
 *   IBL_REG_HAVE_COLORS normals + FPFH + RANSAC + coloured ICP; without it the reference's exception path:
 *                       point-to-point ICP from the identity (fpfh_register.py:137-141)
 * Normals, FPFH and the targets' colour gradients are evaluated on the concatenations BEFORE centring (they are
 * translation invariant; see ibl_instance_features); RANSAC and ICP run between the centred clouds.  Either pool may carry its
 * instance features (features != NULL): the results do not depend on them, only the work does.  Features computed for another
 * voxel_size, or memory features whose gradient radius is not 2 * voxel_size * local_dist_factor, are refused (IBL_ERR_ARG).
 * RANSAC hypothesis i of job j is drawn from Philox4x32-10(counter = (i, id_j, 0, 0), key = seed) with id_j = job_ids[j], or
 * job_id_base + j when job_ids == NULL.  The result of a job is a function of its clouds, the seed and its id only, so a job routed
 * to another rank with its id (memory clouds sharded by instance range: the owner of its target instances runs it, SURVEY 8e /
 * routing.py; the loop being distributed: object_memory/object_memory.py:1020-1106) returns the bits it would have returned at home.
 * Outputs are HOST arrays (the call synchronises): out->T [n_jobs][16] row-major double (between the centred
 * clouds), rmse / fitness [n_jobs] (result_icp.inlier_rmse / .fitness), means [n_jobs][2][3]
 * (detected mean, memory mean; zeros without IBL_REG_CENTER) or NULL, T_ransac [n_jobs][16] or NULL,
 * ransac_stats [n_jobs][3] = (hypotheses walked, validated, best inlier count) or NULL, reuse_stats [6] or NULL: points served by
 * the instance features, points recomputed, recomputed groups, job sides, distinct (query instance, database instance)
 * feature-matching pairs searched, pair uses by the jobs.
 * A null ctx / pool / pool array / job table / params / out / T / rmse / fitness, n_jobs <= 0 and voxel_size <= 0 are refused before
 * anything is launched. */
int ibl_register_jobs(ibl_reg_ctx* ctx, const ibl_cloud_pool* det, const ibl_cloud_pool* mem, const int32_t* job_src_seg,
                      const int32_t* job_tgt_seg, const uint32_t* job_ids /* [HOST] n_jobs or NULL */, int n_jobs,
                      const ibl_register_params* params, const ibl_register_out* out, void* stream);

/* ---- memory build / consolidation; fp64 clouds, as the build side of the reference keeps them ---- */

/* Voxel down-sampling with colours of every object of a batch.  Replaces voxel_down_sample_with_colors
 * (utils/depth_utils.py:211-265) as applied per object by ObjectInfo.downsample (object_memory/object_info.py:95-97) <-
 * ObjectMemory.downsample_all_objects (object_memory/object_memory.py:258-263): voxel = floor(p / voxel_size) per axis, output
 * voxels in order of first occurrence, point / colour = running fp64 sum in input order / count (bit-identical to np.mean).
 *   points, colors [dev] N x 3 doubles (colors may be NULL); seg_off_host [HOST] n_seg + 1 object offsets (n_seg <= 65535, an
 *   object may span at most 65536 voxels per axis); out_points / out_colors [dev] N x 3 doubles (the first
 *   out_seg_off_host[n_seg] rows are written); out_counts [dev] N ints or NULL (points per voxel); out_seg_off_host [HOST]
 *   n_seg + 1.  The call synchronises. */
int ibl_voxel_downsample_batch(ibl_reg_ctx* ctx, const double* points, const double* colors, const int32_t* seg_off_host, int32_t n_seg,
                               double voxel_size, double* out_points, double* out_colors, int32_t* out_counts,
                               int32_t* out_seg_off_host, void* stream);

/* DBSCAN labels, one independent clustering per group of a batch of concatenated clouds.  Replaces
 * open3d.geometry.PointCloud.cluster_dbscan(eps, min_points) as called by recluster_objects_with_dbscan
 * (object_memory/object_memory.py:300-305) and per agglomerative cluster by recluster_via_clustering_and_IoU (:627-631):
 * neighbours are the points at squared distance < eps^2 (the point itself included), a core point has >= min_points of them,
 * clusters are numbered from 0 per group in the order a sequential scan meets their first core point, a border point takes the
 * lowest-numbered cluster among its core neighbours, every other point is -1.
 *   points [dev] N x 3 doubles; grp_off_host [HOST] n_grp + 1; labels [dev] N ints; n_clusters_host [HOST] n_grp or NULL. */
int ibl_dbscan_batch(ibl_reg_ctx* ctx, const double* points, const int32_t* grp_off_host, int32_t n_grp, double eps, int32_t min_points,
                     int32_t* labels, int32_t* n_clusters_host, void* stream);

/* Persistent spatial hash over ALL memory points (world frame), built once per memory upload.  Replaces the
 * KD-tree Open3D rebuilds over `all_memory_pcd` on every evaluate_registration call (utils/fpfh_register.py:146-148
 * <- object_memory/object_memory.py:1104).  cell >= 2 * threshold keeps a query to <= 8 cells.
 *   The grid owns its device arrays (hipMalloc: 16 bytes per point -- 20 in a live grid, see ibl_memgrid_remove --, 12 per occupied cell, 12 per table slot); ctx's arena is
 *   scratch only (40 bytes per point + the sort's, released on return).  live == 0: the grid is immutable and reserve_points must
 *   be 0 (else IBL_ERR_ARG); live != 0: a grid for a memory that grows while it is resident, see ibl_memgrid_append.  A failed
 *   build frees what it allocated; a cell table found full is IBL_ERR_OVERFLOW.
 * ibl_memgrid_destroy frees the grid and its device arrays (NULL is a no-op); nothing may still be using it on any stream. */
typedef struct ibl_memgrid ibl_memgrid;
int ibl_memgrid_build(ibl_reg_ctx* ctx, const float* mem_pts4, int64_t n, double cell, int live, int64_t reserve_points, ibl_memgrid** out,
                      void* stream);
int ibl_memgrid_destroy(ibl_memgrid* grid);

/* Live memory: a grid built with live != 0 has the same keys, the same hash and the same arrays as one built with live == 0 from the
 * same points (it is the same build) -- every evaluation entry point below takes either kind.
 *   It differs in two things: the point buffer holds n + reserve_points points (and the cell arrays min(reserve_points, cells / 2)
 *   further cells), and the grid accepts ibl_memgrid_append.
 *   ibl_memgrid_append merges n_new further points (new_pts4 [dev] n_new x 4 floats; they count as the points n .. n + n_new - 1)
 *   into the grid: afterwards it holds what ibl_memgrid_build returns for the old points followed by the new ones, array for array
 *   (the sort is stable and a cell keeps its points in index order, so the merge "old before new" is that sort).  One pass over
 *   the resident points into the second buffer of a ping-pong pair (allocated by the first append), cell arrays and table
 *   rebuilt; buffers that no longer fit grow by a factor of 1.5, the table keeps the rule of the build (smallest power of two
 *   >= 3 x cells, >= 1024).  Scratch: 16 bytes per point of the merged grid + 24 per new point from ctx's arena, released on return.
 *   n_new == 0 is a no-op (IBL_OK); n + n_new <= 0x7FFFFFF0; a grid built with live == 0 is refused with IBL_ERR_ARG and nothing
 *   is launched.  A failed append that returns IBL_ERR_ARG, the arena error or an allocation error leaves the grid as it was.
 *   Synchronisation: both calls synchronise `stream` before they return.  An append frees and replaces arrays of the grid: no
 *   evaluation that uses the grid may be in flight on ANY other stream during the call, and none may be issued until it returns.
 * ibl_memgrid_info: n, occupied cells, table slots, point capacity of the current buffer and ustart[n_cells] (any pointer may be
 * NULL; asking for ustart_end reads it from the device and synchronises `stream`). */
int ibl_memgrid_append(ibl_reg_ctx* ctx, ibl_memgrid* grid, const float* new_pts4, int64_t n_new, void* stream);
int ibl_memgrid_info(const ibl_memgrid* grid, int64_t* n, int32_t* n_cells, int64_t* table_slots, int64_t* point_capacity,
                     int32_t* ustart_end, void* stream);

/* Live memory, the other direction: ibl_memgrid_remove takes points out of a grid built with live != 0.
 *   range_begin / range_end [HOST] n_ranges entries: half-open ranges over the ORIGINAL point indices of the grid -- a point's position
 *   in the array the grid was built from, plus everything appended since (the indices a batch's segment offsets speak of).  The
 *   ranges must be ascending, disjoint (they may touch) and non-empty, and must leave at least one point.
 *   Afterwards the grid holds what ibl_memgrid_build returns for the kept points in their original order, array for array: sorted,
 *   ukeys, ustart, n, n_cells and the table dimension of the build's rule (smallest power of two >= 3 x cells, >= 1024 -- the table
 *   shrinks logically when cells disappear).  The kept points count as renumbered: original index i becomes i - #removed below i.
 *   Allocations and capacities do not shrink: the freed room is headroom for later appends, and ibl_memgrid_info reports the same
 *   point capacity before and after (the half of the ping-pong pair that becomes current is brought to the current half's size).
 *   A live grid keeps, for this call, the original index of the point in every sorted slot (4 bytes per point on top of the 16,
 *   in both halves of the ping-pong pair; an immutable grid has none; no evaluation reads it).  The removal is one stable compaction
 *   of the cell-ordered points into the other half of the pair -- no sort: slots are flagged by a binary search of their index in
 *   the ranges, the flags are scanned, kept points move with their keys and renumbered indices, and cell arrays and table are
 *   rebuilt as after an append.  A stable compaction of an array in (cell, index) order is in (cell, index) order: that is the
 *   build's order of the kept points.  Traffic ~36 B per point for points and indices + ~40 B for flags, keys and scans.  Scratch:
 *   8 bytes per resident point + 16 per kept point + 12 per range from ctx's arena, released on return; a grid that was never
 *   appended to allocates the second half of its pair here, and one whose last append grew reallocates the smaller half (both as
 *   large as the current one).
 *   n_ranges == 0 is a no-op (IBL_OK).  IBL_ERR_ARG, decided on the host before anything is launched and leaving the grid as it
 *   was: a grid built with live == 0; ranges that are unsorted, overlapping, empty or pass n; ranges that cover every point; null
 *   pointers with n_ranges > 0.  The arena error and an allocation error leave the grid as it was, too.
 *   Synchronisation: as ibl_memgrid_append -- the call synchronises `stream` before it returns, and no evaluation that uses the grid
 *   may be in flight on ANY other stream during the call.
 * ibl_memgrid_export copies the grid's current arrays, device to device and asynchronously on `stream`: the n points in cell order,
 * the n_cells unique cell keys and the n_cells + 1 cell starts (sizes from ibl_memgrid_info; any pointer may be NULL).  For tests
 * and diagnostics that compare grids array for array. */
int ibl_memgrid_remove(ibl_reg_ctx* ctx, ibl_memgrid* grid, const int64_t* range_begin, const int64_t* range_end, int n_ranges,
                       void* stream);
int ibl_memgrid_export(const ibl_memgrid* grid, float* sorted_out /* [dev] n x 4 */, uint64_t* ukeys_out /* [dev] n_cells */,
                       int32_t* ustart_out /* [dev] n_cells + 1 */, void* stream);

/* Live memory, in place: ibl_memgrid_replace changes points that stay where they are in the index space (an instance seen again,
 * two fragments joined, a cloud downsampled) in a grid built with live != 0.
 *   range_begin / range_end [HOST] n_ranges entries: half-open ranges over the ORIGINAL point indices, as for ibl_memgrid_remove:
 *   ascending and disjoint (they may touch).  Range r is replaced by the next new_count[r] rows of new_pts4 ([HOST] n_ranges counts;
 *   [dev] sum(new_count) x 4 floats).  A range may be empty (begin == end, begin == n allowed): a pure insertion in front of index
 *   `begin`, which needs new_count > 0.  new_count[r] may be 0: a pure removal.  Two ranges never begin at the same index, and at
 *   least one point must remain.
 *   Afterwards the grid holds what ibl_memgrid_build returns for the spliced point sequence, array for array: sorted, ukeys, ustart,
 *   n, n_cells and the table dimension of the build's rule; the per-slot original indices are renumbered to the spliced sequence.
 *   One empty range at n is ibl_memgrid_append, counts that are all 0 are ibl_memgrid_remove.
 *   The merge of an append relies on "old before new within a cell" -- appended points have the highest indices.  Points spliced
 *   into the middle interleave, inside a cell, with points of lower and of higher index, so both sides look their place up: a kept
 *   old point with index idx stands behind its kept predecessors (the scan of the removal's flags), the new points of lower cells
 *   and the new points of its own cell whose range begins at or below idx (a search in the stable sort's order of the new
 *   points, which ascends inside a cell); a sorted new point j of range r stands behind j new points and the kept old points in
 *   front of the first slot of its cell whose index is not below range_begin[r] (a search in the cell's indices, which ascend).
 *   No sort of resident points, no atomics, bounded binary searches only; cell arrays and table are rebuilt as after an append.
 *   Traffic: that of a removal per resident point, 56 B per new point.  Scratch from ctx's arena, released on return: 8 bytes per
 *   resident point + 16 per point of the result + 24 per new point + 16 per range + the sort's.
 *   Capacities never shrink: the other half of the ping-pong pair is brought to the current half's size, or grown by 1.5 when the
 *   result no longer fits.
 *   n_ranges == 0 is a no-op (IBL_OK).  IBL_ERR_ARG, decided on the host before anything is launched and leaving the grid as it
 *   was: a grid built with live == 0; ranges that are unsorted, overlapping, reversed or pass n; two ranges with the same begin; an
 *   empty range without new points; a negative count; nothing left; more than 0x7FFFFFF0 points; null pointers.  The arena error
 *   and an allocation error leave the grid as it was, too: nothing of it is overwritten before the new state is complete.
 *   Synchronisation: as ibl_memgrid_append and ibl_memgrid_remove. */
int ibl_memgrid_replace(ibl_reg_ctx* ctx, ibl_memgrid* grid, const int64_t* range_begin, const int64_t* range_end,
                        const int64_t* new_count, const float* new_pts4, int n_ranges, void* stream);

/* Live memory, association: which resident instances does each detection cloud overlap -- the geometric half of deciding whether a
 * detection is an instance seen again (the reference raises "Only final clustering available currently" where it would decide,
 * object_memory/object_memory.py:230-235).  For detection d (the world-frame points det_off_host[d] .. det_off_host[d + 1] of
 * det_pts4) and instance m (the ORIGINAL point indices inst_off[m] .. inst_off[m + 1] of the grid)
 *       hits(d, m) = #{ p in d : some point q of m has d2(p, q) < r2 },
 *   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 with a strict <, r2 = (float)(radius * radius) as ibl_evaluate_batch forms its
 *   threshold.  A point near several instances counts once for each: "some point within r", not "the owner of the nearest point", so
 *   no tie between instances decides a count and hits is an exact integer.
 *   Per detection the call returns the instances with hits > 0 ordered by hits descending, then instance ascending, cut to k:
 *   pair_inst / pair_hits [HOST] n_det x k (-1 / 0 padded), n_hit_inst [HOST] n_det = the uncut number of such instances (may exceed k).
 *   inst_off [dev] n_inst + 1 ascending offsets (empty instances allowed), inst_off_end = its last entry as the caller knows it:
 *   it must equal the grid's n (checked without a device read).  det_pts4 [dev] float4 rows; det_off_host [HOST] n_det + 1.
 *   Two launches: one thread per detection point walks the cells of its +-radius box through the table (every probe bounded by the
 *   table size), reads the per-slot original index next to a point within r, maps it to its instance by a bounded search and adds 1
 *   to a dense int32 [n_det][n_inst] array (integer atomics: deterministic totals; an instance met in several cells of the box counts
 *   once, for any number of instances); one workgroup per detection then ranks the non-zero entries.
 *   Scratch from ctx's arena, released on return: 4 n_det n_inst + 8 n_det k + 4 (2 n_det + 1) bytes; exhaustion is the arena error.
 *   A LIVE grid is required: an immutable one keeps no per-slot indices.  IBL_ERR_ARG, decided on the host before anything is
 *   launched and leaving the outputs untouched: a grid built with live == 0; radius <= 0; radius > the grid's cell (a box is then at
 *   most 27 cells); k < 1; n_inst < 1; inst_off_end != n; det_off_host that begins below 0 or descends; null pointers.  n_det == 0
 *   succeeds and launches nothing.
 *   Synchronisation: the call synchronises `stream` before it returns (its results are host arrays); the grid is only read. */
int ibl_memgrid_overlap(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const int32_t* inst_off, int32_t n_inst, int32_t inst_off_end,
                        const float* det_pts4, const int32_t* det_off_host, int32_t n_det, double radius, int32_t k,
                        int32_t* pair_inst, int32_t* pair_hits, int32_t* n_hit_inst, void* stream);

/* evaluate_transform(all_detected_pcd, all_memory_pcd, T) for n_jobs candidates: job j transforms the detected
 * points [job_begin[j], job_end[j]) of det_pts4 [dev] by T_global[j] (host, 16 doubles row-major) and looks for
 * the nearest memory point within `threshold`.  rmse_out / fitness_out: HOST arrays (the call synchronises).
 *   d2_out [dev] floats or NULL: additionally the squared distance of every transformed detected point to its nearest memory point
 *   within `threshold` (+inf when there is none), job j's points at offset sum_{i<j} (job_end[i] - job_begin[i]).  This is the
 *   per-shard half of the sharded whole-memory evaluation of SURVEY 8(e): every rank evaluates against the memory points it owns, the
 *   distances are combined with an all-reduce(MIN) (RCCL) and fitness / rmse follow from the combined array
 *   (ibloc_amd.parallel.evaluate_sharded). */
int ibl_evaluate_batch(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const float* det_pts4, const int32_t* job_begin,
                       const int32_t* job_end, const double* T_global, int n_jobs, double threshold, float* d2_out /* [dev] or NULL */,
                       double* rmse_out, double* fitness_out, void* stream);

/* get_information_matrix_from_point_clouds (the third member of Open3D's registration trio) for n_jobs poses against the whole
 * memory: the 6 x 6 matrix sum G^T G over the correspondences of T_global[j], rotation first, then translation.
 *   Correspondences: those of ibl_evaluate_batch -- q = (float)(T p) for the detected points [job_begin[j], job_end[j]), its match the
 *   memory point m of the grid with the smallest fp32 d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), accepted when d2 < (float)(threshold *
 *   threshold).  n_corr_out[j] / (job_end[j] - job_begin[j]) is ibl_evaluate_batch's fitness exactly.  Among memory points at the same
 *   minimal d2 the match is the one with the lexicographically smallest (x, y, z), compared as floats: the result depends on the SET
 *   of memory points only, not on cell order, pruning or live edits (a live grid gives the bits of a grid built at once).
 *   Matrix: with (x, y, z) = (double)m - about, rows G1 = [0, z, -y, 1, 0, 0], G2 = [-z, 0, x, 0, 1, 0], G3 = [y, -x, 0, 0, 0, 1];
 *   the device reduces n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz in fp64 in a fixed order (no atomics: two calls give the same bits)
 *   and the host assembles rot-rot [[Syy+Szz, -Sxy, -Sxz], [., Sxx+Szz, -Syz], [., ., Sxx+Syy]], rot-trans [[0, -Sz, Sy], [Sz, 0, -Sx],
 *   [-Sy, Sx, 0]], trans-trans n I.  It belongs to the LEFT perturbation T' = exp(xi^) T_global, xi = (omega, v).
 *   about [HOST] 3 doubles or NULL = the origin (Open3D's convention); a scene far from the origin conditions better about its centroid.
 *   nn_out [dev, 16-byte aligned] or NULL: 4 floats per (job, point), jobs back to back as d2_out of ibl_evaluate_batch: the matched
 *   x, y, z and d2; (0, 0, 0, +inf) when none.  info_out [HOST] 36 per job, row-major, symmetric bit for bit; n_corr_out [HOST] per
 *   job.  An empty job gives a zero matrix and 0.
 *   IBL_ERR_ARG, decided before anything is launched and leaving the outputs untouched: null pointers (about and nn_out may be
 *   null), threshold <= 0, n_jobs <= 0, a range that descends or begins below 0.  More than 65 535 jobs go in several launches.
 *   Scratch from ctx's arena, released on return.  The call synchronises `stream` before it returns; the grid is only read. */
int ibl_evaluate_information(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const float* det_pts4, const int32_t* job_begin,
                             const int32_t* job_end, const double* T_global, int n_jobs, double threshold,
                             const double* about /* 3 doubles, host; NULL = origin */, float* nn_out /* [dev] or NULL */,
                             double* info_out /* host, 36 per job */, int64_t* n_corr_out /* host, per job */, void* stream);

/* Stage B of localise() for a batch of frames in ONE call (SURVEY 8b's fused driver; csrc/localise.hip): radius-outlier removal of
 * every detected cloud and ordered compaction (object_memory/object_memory.py:992-998), the detections' instance features, one
 * registration job per candidate assignment (:1020-1095), the global-frame transform of every job (:1096-1101), its whole-memory
 * evaluation (:1104) and the winner of every frame (highest whole-memory fitness, the first on ties, :1111-1114).  Everything is
 * the library's own stage entry points composed on the host -- the results are those of calling ibl_radius_outlier_batch,
 * ibl_instance_features_batch, ibl_register_jobs and ibl_evaluate_batch in turn, bit for bit.
 *   det: the RAW detected clouds, segments in frame order, q_per_frame [HOST][n_frames] of them per frame (<= 7 each); det->features
 *   must be NULL (the call computes them for the cleaned clouds), else IBL_ERR_ARG; assn [HOST][n_frames][max_assn][6] = up to three
 *   (detection within its frame, GLOBAL memory instance) pairs per assignment, assn_len [HOST][n_frames][max_assn] pairs used,
 *   assn_count [HOST][n_frames] -- the output layout of ibl_assign_batch / ibl_assign_candidates; mem: the memory pool with its
 *   resident instance features (required); grid: its spatial hash; params: as for ibl_register_jobs (job ids are job_id_base + j).
 * Outputs (HOST; the call synchronises): clean_off_host [det->n_seg + 1] offsets of the cleaned clouds, *n_jobs_out = J (jobs in
 * frame order, a frame's jobs in assignment order; J <= max_jobs = the capacity of the per-job arrays), out as for ibl_register_jobs
 * (means is required here), T_global_out [J][16], full_rmse_out / full_fitness_out [J], best_out [n_frames] = winning assignment of
 * the frame (index into its list) or -1 for a frame without assignments. */
int ibl_register_evaluate_batch(ibl_reg_ctx* ctx, const ibl_cloud_pool* det, const int32_t* q_per_frame, int n_frames, const int32_t* assn,
                                const int32_t* assn_len, const int32_t* assn_count, int max_assn, const ibl_cloud_pool* mem,
                                const ibl_memgrid* grid, const ibl_register_params* params, double outlier_radius, int outlier_nb_points,
                                double eval_threshold, int max_jobs, int32_t* clean_off_host, int32_t* n_jobs_out,
                                const ibl_register_out* out, double* T_global_out, double* full_rmse_out, double* full_fitness_out,
                                int32_t* best_out, void* stream);

/* 1 - IoU of the oriented boxes of n objects, as ObjectMemory._recluster_IoU feeds scikit-learn.
 * boxes [dev] n x 15 f64 (centre, R row-major, half extents); valid [dev] n int32 (0: no box -> IoU 0 with everything);
 * dist [dev] n x n f64 row-major, caller-owned; n_overlapping [host, may be NULL]: pairs that passed the separating-axis test
 * (synchronises the stream when non-NULL).  Scratch from ctx's arena, released on return. */
int ibl_obb_iou_matrix(ibl_reg_ctx* ctx, const double* boxes, const int32_t* valid, int64_t n, double* dist,
                       int64_t* n_overlapping, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IBLOC_H */
