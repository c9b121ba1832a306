// vit.hip -- ViT encoder forward on gfx950 (fp16 MFMA 16x16x32, fp32 accumulate, fp32 residual).
//
// Replaces the torch/cuDNN forward the reference reaches through
//   utils/embeddings.py:46 (CLIP ViT-B/32), :69 (DINOv2), :93 (ViT-B/16), :119 (DATOR streams,
//   dator/model/backbones/vit_pytorch.py:422-443)
// one crop at a time; here a whole batch of crops runs per call.
//
// HBM layout (all row-major, token-major): residual stream x fp32 [B*T][D]; LayerNorm output,
// QKV, attention output and MLP hidden as fp16 (11-bit significand: rel-L2 1.2e-3 on the 12-layer ViT-B/14 where bf16 operands gave 1.1e-2, same MFMA rate); weights fp16 [N][K] (K contiguous, i.e. the
// nn.Linear layout) so that both MFMA operands are 16-byte K-contiguous fragments.
//
// Kernels: gemm_f16_tn (256x256x64 / 128x128x64 LDS tiles filled by direct-to-LDS buffer loads, software-pipelined K loop, fused epilogues:
// bias / bias+GELU / bias*layerscale+residual / patch-embed scatter+pos-embed), layernorm (one
// wave per row), attention (one workgroup per (crop, head), K and V^T of the head staged in LDS,
// S^T = K Q^T so that the softmaxed probabilities are already the A operand of P V), CLS/final
// LayerNorm, prefix rows (class token + register tokens), rope (rotary position embedding of DINOv3, in place on q and k).
//
// One file per kernel: vit_gemm.hip, vit_layernorm.hip, vit_attention.hip (attention and rope), reached through the launchers of
// vit_kernels.h.  This file holds the prefix-row and class-row kernels, the workspace layout and its entries, and ONE forward behind two
// entries: a driver over one function per stage (embed, attention_half, mlp_half, head).
//   ibl_vit_forward          every crop at the model's grid: crop b owns rows b * T .. (b + 1) * T - 1 of every [rows][...] buffer
//   ibl_vit_forward_ragged   every crop at a patch grid of its own (native-aspect crops): crop b owns rows seq_off[b] .. seq_off[b + 1] - 1,
//                            its prefix rows (class token, registers), then its gh * gw patches
// Everything in the encoder but the attention is row-wise, so the two differ in three places only: the patch epilogue's row fields, the
// attention launcher, and where the class rows of the class-rows-only last block live (ClassRows below).
#include "vit_kernels.h"

// the prefix rows of every crop: x[r0 + 0][:] = cls_pos[:] (cls token + its position embedding), x[r0 + 1 + r][:] = reg[r][:] (register
// tokens, no position embedding); n_prefix = 1 + registers; r0 the crop's first row: seq_off[b], without a table b * T
__global__ void ibl_set_prefix_kernel(float* __restrict__ x, const float* __restrict__ cls_pos, const float* __restrict__ reg,
                                      const int* __restrict__ seq_off, int B, int T, int n_prefix, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n_prefix * dim) return;
    const int c = (int)(i % dim);
    const int64_t br = i / dim;
    const int b = (int)(br / n_prefix), r = (int)(br % n_prefix);
    const int64_t r0 = seq_off ? (int64_t)seq_off[b] : (int64_t)b * T;
    x[(r0 + r) * dim + c] = r == 0 ? cls_pos[c] : reg[(int64_t)(r - 1) * dim + c];
}

// the class rows, n16 x 16 bytes each: compact[b] <- rows[seq_off[b]] (scatter 0) or rows[seq_off[b]] <- compact[b] (scatter 1).
// ld_rows / ld_compact in units of 16 bytes
__global__ void ibl_class_rows_kernel(uint4* __restrict__ rows, int64_t ld_rows, uint4* __restrict__ compact, int64_t ld_compact,
                                      const int* __restrict__ seq_off, int B, int n16, int scatter) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n16) return;
    const int b = (int)(i / n16), c = (int)(i % n16);
    uint4* r = rows + (int64_t)seq_off[b] * ld_rows + c;
    uint4* k = compact + (int64_t)b * ld_compact + c;
    if (scatter) *r = *k;
    else *k = *r;
}

// widest K-extended input of a residual GEMM the workspace has room for
static int act_terms(const ibl_vit_desc* d) { return (d->flags & IBL_VIT_ACT_TERMS3) ? 3 : ((d->flags & IBL_VIT_ACT_TERMS2) ? 2 : 1); }

// The workspace layout, in one place: byte offsets of the first n buffers from the 256-byte-aligned workspace base, each buffer on a
// 256-byte boundary; returns the end.  The IBL_VIT_WS_* buffers come first: they are all the fixed grid has (n = IBL_VIT_WS_COUNT) and
// all that ibl_vit_workspace_bytes and ibl_vit_workspace_layout count and report.  The ragged grid (n = WS_ALL) adds the compact class
// rows: CX fp32 [batch][D] of the residual stream, CA fp16 [batch][D] of q, then of the attention output.
enum { WS_CX = IBL_VIT_WS_COUNT, WS_CA, WS_ALL };

static int64_t vit_layout(const ibl_vit_desc* d, int64_t rows, int batch, int64_t* offs, int n, int64_t* payload = nullptr) {
    const int64_t R = rows_pad(rows), Bp = rows_pad(batch);
    const int at = act_terms(d);
    int64_t bytes[WS_ALL];
    bytes[IBL_VIT_WS_X] = R * d->dim * 4;              // residual stream, fp32
    bytes[IBL_VIT_WS_XN] = R * d->dim * 2 * 3;         // LayerNorm output (up to three terms per row, two-term operands of the early blocks)
    bytes[IBL_VIT_WS_QKV] = R * 3 * d->dim * 2;
    bytes[IBL_VIT_WS_ATT] = R * d->dim * 2 * at;       // attention output
    bytes[IBL_VIT_WS_HID] = R * d->mlp_dim * 2 * at;   // MLP hidden layer
    bytes[IBL_VIT_WS_FIN] = Bp * d->dim * 2;           // CLS rows after a LayerNorm (fp16)
    bytes[WS_CX] = Bp * d->dim * 4;
    bytes[WS_CA] = Bp * d->dim * 2;
    int64_t p = 0, sum = 0;
    for (int i = 0; i < n; ++i) {
        p = (p + 255) & ~(int64_t)255;
        offs[i] = p;
        p += bytes[i];
        sum += bytes[i];
    }
    if (payload) *payload = sum;      // the buffers without their alignment gaps
    return p;
}

extern "C" int64_t ibl_vit_workspace_bytes(const ibl_vit_desc* d, int batch) {
    if (!d || batch <= 0) return -1;
    int64_t offs[IBL_VIT_WS_COUNT], sum = 0;
    vit_layout(d, (int64_t)batch * d->n_tokens, batch, offs, IBL_VIT_WS_COUNT, &sum);
    // the size callers have always been asked for: the buffers, fp32 final rows (reserved; nothing is carved for them) and nine alignment
    // gaps -- the base's and the five between the buffers fit in those
    return sum + rows_pad(batch) * d->dim * 4 + 9 * 256;
}

extern "C" int ibl_vit_workspace_layout(const ibl_vit_desc* d, int batch, int64_t* offsets, int n) {
    if (!d || batch <= 0 || !offsets || n < 0 || n > IBL_VIT_WS_COUNT)
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_workspace_layout: bad argument");
    vit_layout(d, (int64_t)batch * d->n_tokens, batch, offsets, n);
    return IBL_OK;
}

extern "C" int64_t ibl_vit_ragged_workspace_bytes(const ibl_vit_desc* d, int64_t total_tokens, int batch) {
    if (!d || batch <= 0 || total_tokens < batch || total_tokens > 0x7fffffff) return -1;
    int64_t offs[WS_ALL];
    return vit_layout(d, total_tokens, batch, offs, WS_ALL) + 256;      // + the gap to the first 256-byte boundary
}

// What block l runs with: the one place that decides it.
// cls_only: only the CLS row leaves the encoder (unless all tokens are asked for), so in the LAST block the other rows are dead
// after they have served as keys / values: its query projection, attention, output projection and MLP run on the CLS
// rows alone (M = batch instead of batch * T; every row of a GEMM is computed independently, so the CLS rows come out
// bit-identical).
// qkv / fc1: two-term operands (ibloc.h): only in blocks that run on every row (the CLS-only last block stays plain).
// o / fc2: K-extended inputs of the two residual GEMMs (w_o_x / w_fc2_x; round 4): ONE launch of K' = terms * K instead of one
// read-modify-write pass over the residual per term
struct BlockTerms {
    bool cls_only;
    int qkv, o, fc1, fc2;
};

static BlockTerms block_terms(const ibl_vit_desc* d, const ibl_vit_weights* w, int l) {
    const ibl_vit_layer* L = &w->layers[l];
    BlockTerms t;
    t.cls_only = (l == d->n_blocks_run - 1) && !(d->flags & IBL_VIT_OUT_ALL_TOKENS);
    t.qkv = (!t.cls_only && L->w_qkv_x && L->qkv_terms > 1) ? L->qkv_terms : 1;
    t.o = (!t.cls_only && L->w_o_x && L->o_terms > 1) ? L->o_terms : 1;
    t.fc1 = (!t.cls_only && L->w_fc1_x && L->fc1_terms > 1) ? L->fc1_terms : 1;
    t.fc2 = (!t.cls_only && L->w_fc2_x && L->fc2_terms > 1) ? L->fc2_terms : 1;
    return t;
}

// refused before anything is launched: a descriptor that is wrong in layer l must not leave blocks 0 .. l - 1 in the caller's workspace
static int check_block_terms(const char* fn, int l, const BlockTerms& t, int at) {
    if (t.qkv > 3 || t.fc1 > 3) return ibl_set_error(IBL_ERR_ARG, "%s: layer %d: at most three operand terms", fn, l);
    if (t.o > at || t.fc2 > at || t.o > 3 || t.fc2 > 3)
        return ibl_set_error(IBL_ERR_ARG, "%s: layer %d: o_terms / fc2_terms %d / %d need IBL_VIT_ACT_TERMS%d in the descriptor", fn, l, t.o, t.fc2, t.o > t.fc2 ? t.o : t.fc2);
    return IBL_OK;
}

// The forward: what one call works on, and one function per stage
struct VitCtx {
    const ibl_vit_desc* d;
    const ibl_vit_weights* w;
    int batch;
    hipStream_t s;
    float* x;                        // the six IBL_VIT_WS_* buffers, carved once from vit_layout
    u16 *xn, *qkv, *att, *hid, *fin;
    int64_t Rn;                      // rows: batch * n_tokens, or the ragged grid's total tokens
    int at;                          // act_terms(d)
    int n_prefix;                    // class token + registers; 0 with IBL_VIT_NO_CLS
    const int* seq_off;              // [dev] per-crop row offsets; null: equal rows of n_tokens per crop
    int max_tokens;                  // the longest crop
    float* cx;                       // WS_CX, WS_CA: the ragged grid's compact class rows; null on the fixed grid
    u16* ca;
};

// The class rows of a [rows][ld] buffer as (pointer, row stride in elements): what the class-rows-only last block and the head work on.
// The fixed grid addresses them in place, by the stride T * ld, and launches nothing; the ragged grid gathers them to a compact [batch][D]
// buffer and scatters them back, so that its GEMMs and LayerNorms run with the fixed grid's M, N, K on rows computed independently.
struct ClassRows {
    void* p;
    int64_t ld;
};

// the view alone: a destination, or rows that class_take has already gathered
static ClassRows class_view(const VitCtx& c, void* buf, int64_t ld, void* compact) {
    return c.seq_off ? ClassRows{compact, c.d->dim} : ClassRows{buf, (int64_t)c.d->n_tokens * ld};
}

static int class_copy(const VitCtx& c, void* buf, int64_t ld, int elem_bytes, void* compact, int scatter) {
    if (!c.seq_off) return IBL_OK;
    const int n16 = c.d->dim * elem_bytes / 16;       // 16-byte pieces of one class row
    const int64_t n = (int64_t)c.batch * n16;
    hipLaunchKernelGGL(ibl_class_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, reinterpret_cast<uint4*>(buf),
                       ld * elem_bytes / 16, reinterpret_cast<uint4*>(compact), (int64_t)n16, c.seq_off, c.batch, n16, scatter);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// the class rows of buf (D elements of elem_bytes each, row stride ld): gathered to `compact` on the ragged grid
static int class_take(const VitCtx& c, void* buf, int64_t ld, int elem_bytes, void* compact, ClassRows* v) {
    *v = class_view(c, buf, ld, compact);
    return class_copy(c, buf, ld, elem_bytes, compact, 0);
}

// ... and put back where the view is not the buffer itself
static int class_put(const VitCtx& c, void* buf, int64_t ld, int elem_bytes, void* compact) { return class_copy(c, buf, ld, elem_bytes, compact, 1); }

// patch embedding (conv as GEMM over im2col'ed patches) + position embedding, scattered into x; the prefix rows; CLIP's ln_pre.
// The ragged grid's patch matrix holds one row per TOKEN (zero prefix rows) and pos_rows one position row per token, so the whole batch
// is one "crop" of the patch epilogue: x[r] = acc + bias + pos_rows[r], the fixed grid's expression; the prefix rows are then overwritten
static int embed(const VitCtx& c, const void* patches, const float* pos_rows) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim, T = d->n_tokens, P = T - c.n_prefix;
    const int M = c.seq_off ? (int)c.Rn : c.batch * P;
    int st;
    GemmEpi e{};
    e.bias = w->b_patch; e.out = c.x; e.ldo = D;
    if (c.seq_off) {
        e.pos = pos_rows; e.tokens_per_crop = M; e.patches_per_crop = M; e.patch_row0 = 0;
    } else {
        e.pos = w->pos_patch; e.tokens_per_crop = T; e.patches_per_crop = P;
        e.patch_row0 = c.n_prefix;     // the patch rows follow the crop's prefix rows: class token and registers
    }
    st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                     reinterpret_cast<const u16*>(w->w_patch), d->patch_k_pad, M, D, d->patch_k_pad, e, c.s);
    if (st) return st;
    if (w->w_patch_lo) {             // second term of the patch weights: x += (patches W_lo'^T) / S
        GemmEpi e2 = e;
        e2.bias = nullptr; e2.accumulate = 1; e2.alpha = 1.0f / IBL_VIT_SPLIT_SCALE; e2.algo_k = -1;
        st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                         reinterpret_cast<const u16*>(w->w_patch_lo), d->patch_k_pad, M, D, d->patch_k_pad, e2, c.s);
        if (st) return st;
    }
    if (!(d->flags & IBL_VIT_NO_CLS)) {
        const int64_t n = (int64_t)c.batch * c.n_prefix * D;
        hipLaunchKernelGGL(ibl_set_prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, c.x, w->cls_pos, w->reg_tokens, c.seq_off,
                           c.batch, T, c.n_prefix, D);
        IBL_LAUNCH_CHECK();
    }
    if (d->flags & IBL_VIT_PRE_LN) {
        // CLIP ln_pre: normalise the residual stream in place (through the fp16-free f32 path)
        st = launch_layernorm(c.x, D, c.Rn, D, w->ln_pre_g, w->ln_pre_b, d->ln_eps, c.x, D, 0, c.s);
        if (st) return st;
    }
    return IBL_OK;
}

// out += scale * (a W'^T + bias): the output projection and fc2.  `terms` > 1: a and W' are K-extended rows, one launch of K' = terms * K
// (w_x).  terms == 1: the plain weights w, and where the layer carries them the (older form) second weight term as its own launch:
// out += (ls / S) * (a W_lo'^T).  a: `rows` rows of stride lda; out: the residual stream, in a CLS-only block its class rows
static int resid_gemm(const VitCtx& c, bool cls_only, ClassRows out, const u16* a, int64_t lda, int rows, int terms, int K, const void* w,
                      const void* w_x, const void* w_lo, const float* bias, const float* ls, const float* ls_lo) {
    const int D = c.d->dim;
    GemmEpi e{};
    e.bias = bias; e.scale = ls; e.out = out.p; e.ldo = out.ld; e.alpha = 1.0f; e.algo_k = K;
    const int64_t kx = (int64_t)terms * K;
    // no LayerScale vector (none in the model, or folded into W_o / b_o by the host): the residual tile is preloaded into the
    // accumulators (EPI_RESID_PRE_F32, lab); with one, the read-modify-write epilogue applies it
    int st = gemm_launch((ls || !gemm_resid_pre()) ? IBL_LINEAR_RESID_F32 : IBL_LINEAR_RESID_PRE_F32, IBL_ACT_GELU_ERF, a, lda,
                         reinterpret_cast<const u16*>(terms > 1 ? w_x : w), kx, rows, D, (int)kx, e, c.s);
    if (st) return st;
    if (!cls_only && terms == 1 && w_lo) {
        e.bias = nullptr; e.scale = ls_lo; e.algo_k = -1; e.alpha = 1.0f / IBL_VIT_SPLIT_SCALE;
        st = gemm_launch(ls_lo ? IBL_LINEAR_RESID_F32 : IBL_LINEAR_RESID_PRE_F32, IBL_ACT_GELU_ERF, a, K, reinterpret_cast<const u16*>(w_lo), K, rows,
                         D, K, e, c.s);
    }
    return st;
}

// LN1 -> QKV (a CLS-only block: K / V of every row, Q of the class rows) -> rotation -> attention -> x += output projection
static int attention_half(const VitCtx& c, int l, const BlockTerms& t) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_layer* L = &c.w->layers[l];
    const int D = d->dim, T = d->n_tokens, H = d->heads;
    int st = launch_layernorm(c.x, D, c.Rn, D, L->ln1_g, L->ln1_b, d->ln_eps, c.xn, (int64_t)t.qkv * D, t.qkv, c.s);
    if (st) return st;
    if (!t.cls_only) {
        GemmEpi e{};
        e.bias = L->b_qkv; e.out = c.qkv; e.ldo = 3 * D; e.algo_k = D;
        st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.xn, (int64_t)t.qkv * D, reinterpret_cast<const u16*>(t.qkv > 1 ? L->w_qkv_x : L->w_qkv),
                         (int64_t)t.qkv * D, (int)c.Rn, 3 * D, t.qkv * D, e, c.s);
        if (st) return st;
    } else {
        GemmEpi e{};                                  // keys and values of every token: weight rows D .. 3D
        e.bias = L->b_qkv + D; e.out = c.qkv + D; e.ldo = 3 * D;
        st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.xn, D, reinterpret_cast<const u16*>(L->w_qkv) + (int64_t)D * D, D, (int)c.Rn, 2 * D, D, e,
                         c.s);
        if (st) return st;
        // queries of the CLS rows only: the class rows of LN1's output (ragged: through FIN) into the q columns of their rows (through CA)
        ClassRows xn, q = class_view(c, c.qkv, 3 * D, c.ca);
        if ((st = class_take(c, c.xn, D, 2, c.fin, &xn)) != IBL_OK) return st;
        GemmEpi eq{};
        eq.bias = L->b_qkv; eq.out = q.p; eq.ldo = q.ld;
        st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(xn.p), xn.ld, reinterpret_cast<const u16*>(L->w_qkv), D, c.batch, D,
                         D, eq, c.s);
        if (st) return st;
        if ((st = class_put(c, c.qkv, 3 * D, 2, c.ca)) != IBL_OK) return st;
    }
    const int cls = t.cls_only ? 1 : 0;
    if (c.seq_off) {
        st = run_attention_ragged(c.qkv, c.att, c.seq_off, c.batch, c.max_tokens, D, H, cls, c.s, t.o);
    } else {
        if (c.w->rope_table) {  // DINOv3: q and k of the patch rows rotated in place; the class-rows-only block has no patch-row q to rotate
            st = run_rope(c.qkv, c.w->rope_table, c.batch, T, c.n_prefix, D, H, cls, c.s);
            if (st) return st;
        }
        st = run_attention(c.qkv, c.att, c.batch, T, D, H, cls, c.s, t.o);
    }
    if (st) return st;
    if (!t.cls_only)
        return resid_gemm(c, false, ClassRows{c.x, D}, c.att, (int64_t)t.o * D, (int)c.Rn, t.o, D, L->w_o, L->w_o_x, L->w_o_lo, L->b_o, L->ls1, L->ls1_lo);
    // the class rows of the attention output and of the residual stream: on the ragged grid compact (CA, CX) from here on
    ClassRows att, x;
    if ((st = class_take(c, c.att, D, 2, c.ca, &att)) != IBL_OK) return st;
    if ((st = class_take(c, c.x, D, 4, c.cx, &x)) != IBL_OK) return st;
    return resid_gemm(c, true, x, reinterpret_cast<const u16*>(att.p), att.ld, c.batch, 1, D, L->w_o, L->w_o_x, L->w_o_lo, L->b_o, L->ls1, L->ls1_lo);
}

// LN2 (the class rows of a CLS-only block go to FIN) -> fc1 + GELU -> x += fc2
static int mlp_half(const VitCtx& c, int l, const BlockTerms& t) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_layer* L = &c.w->layers[l];
    const int D = d->dim;
    // the rows of the residual stream this half runs on: every row, or the class rows attention_half left
    const ClassRows x = t.cls_only ? class_view(c, c.x, D, c.cx) : ClassRows{c.x, D};
    int st = t.cls_only ? launch_layernorm(reinterpret_cast<const float*>(x.p), x.ld, c.batch, D, L->ln2_g, L->ln2_b, d->ln_eps, c.fin, D, 1, c.s)
                        : launch_layernorm(c.x, D, c.Rn, D, L->ln2_g, L->ln2_b, d->ln_eps, c.xn, (int64_t)t.fc1 * D, t.fc1, c.s);
    if (st) return st;
    const u16* mlp_in = t.cls_only ? c.fin : c.xn;
    const int mlp_rows = t.cls_only ? c.batch : (int)c.Rn;
    GemmEpi e{};
    e.bias = L->b_fc1; e.out = c.hid; e.ldo = (int64_t)t.fc2 * d->mlp_dim; e.algo_k = D;
    // the hidden layer is written as the K-extended rows fc2 reads
    const int epi = t.fc2 == 3 ? IBL_LINEAR_GELU_F16_X3 : (t.fc2 == 2 ? IBL_LINEAR_GELU_F16_X2 : IBL_LINEAR_GELU_F16);
    const int act = (d->flags & IBL_VIT_QUICK_GELU) ? IBL_ACT_QUICK_GELU : ((d->flags & IBL_VIT_TANH_GELU) ? IBL_ACT_GELU_TANH : IBL_ACT_GELU_ERF);
    st = gemm_launch(epi, act, mlp_in, (int64_t)t.fc1 * D, reinterpret_cast<const u16*>(t.fc1 > 1 ? L->w_fc1_x : L->w_fc1), (int64_t)t.fc1 * D, mlp_rows,
                     d->mlp_dim, t.fc1 * D, e, c.s);
    if (st) return st;
    return resid_gemm(c, t.cls_only, x, c.hid, (int64_t)t.fc2 * d->mlp_dim, mlp_rows, t.fc2, d->mlp_dim, L->w_fc2, L->w_fc2_x, L->w_fc2_lo, L->b_fc2,
                      L->ls2, L->ls2_lo);
}

// x -> out: all tokens (DATOR streams; the ragged grid's rows packed), or the CLS rows -> (final LN) -> (projection) -> out fp32
// [batch][out_dim].  have_class_rows: the last block ran class rows only and has taken them
static int head(const VitCtx& c, float* out, bool have_class_rows) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim;
    int st;
    if (d->flags & IBL_VIT_OUT_ALL_TOKENS) {
        // all tokens, optionally through the final LayerNorm
        if (d->flags & IBL_VIT_FINAL_LN) return launch_layernorm(c.x, D, c.Rn, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
        IBL_HIP_CHECK(hipMemcpyAsync(out, c.x, c.Rn * D * 4, hipMemcpyDeviceToDevice, c.s));
        return IBL_OK;
    }
    ClassRows x = class_view(c, c.x, D, c.cx);
    if (!have_class_rows && (st = class_take(c, c.x, D, 4, c.cx, &x)) != IBL_OK) return st;
    const float* xc = reinterpret_cast<const float*>(x.p);
    if (d->flags & IBL_VIT_PROJ) {
        if (!(d->flags & IBL_VIT_FINAL_LN)) return ibl_set_error(IBL_ERR_UNSUPPORTED, "projection needs final LN");
        GemmEpi e{};
        e.bias = nullptr; e.out = out; e.ldo = d->out_dim;
        if (w->w_proj_x) {           // three-term operands: K' = 3 D, one accumulation (xn is free by now: batch <= R rows of 3 D)
            st = launch_layernorm(xc, x.ld, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, c.xn, (int64_t)3 * D, 3, c.s);
            if (st) return st;
            e.algo_k = D;
            return gemm_launch(IBL_LINEAR_F32, IBL_ACT_GELU_ERF, c.xn, (int64_t)3 * D, reinterpret_cast<const u16*>(w->w_proj_x), (int64_t)3 * D, c.batch,
                               d->out_dim, 3 * D, e, c.s);
        }
        st = launch_layernorm(xc, x.ld, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, c.fin, D, 1, c.s);
        if (st) return st;
        return gemm_launch(IBL_LINEAR_F32, IBL_ACT_GELU_ERF, c.fin, D, reinterpret_cast<const u16*>(w->w_proj), D, c.batch, d->out_dim, D, e, c.s);
    }
    if (d->flags & IBL_VIT_FINAL_LN) return launch_layernorm(xc, x.ld, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
    if (x.ld == D) {                 // compact rows: one copy, as the ragged grid has always made it
        IBL_HIP_CHECK(hipMemcpyAsync(out, xc, (size_t)c.batch * D * 4, hipMemcpyDeviceToDevice, c.s));
    } else {
        IBL_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)D * 4, xc, (size_t)x.ld * 4, (size_t)D * 4, c.batch, hipMemcpyDeviceToDevice, c.s));
    }
    return IBL_OK;
}

// the refusals both entries share, `fn` the entry's name
static int check_desc(const char* fn, const ibl_vit_desc* d, const ibl_vit_weights* w, bool any_null, int batch) {
    if (any_null) return ibl_set_error(IBL_ERR_ARG, "%s: null pointer", fn);
    if (batch <= 0) return ibl_set_error(IBL_ERR_ARG, "%s: batch must be positive", fn);
    if (d->n_registers < 0) return ibl_set_error(IBL_ERR_ARG, "%s: n_registers %d is negative", fn, d->n_registers);
    if (d->n_registers > 0 && !w->reg_tokens) return ibl_set_error(IBL_ERR_ARG, "%s: n_registers %d without reg_tokens", fn, d->n_registers);
    if ((d->flags & IBL_VIT_QUICK_GELU) && (d->flags & IBL_VIT_TANH_GELU))
        return ibl_set_error(IBL_ERR_ARG, "%s: IBL_VIT_QUICK_GELU and IBL_VIT_TANH_GELU are both set", fn);
    if (d->dim != d->heads * 64) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: head_dim must be 64", fn);
    if (d->dim % 128 || d->mlp_dim % 128 || d->patch_k_pad % 64 || d->dim > 1024)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: dim/mlp_dim %% 128, patch_k_pad %% 64, dim <= 1024", fn);
    if (d->n_blocks_run < 0 || d->n_blocks_run > d->depth || d->depth > IBL_VIT_MAX_LAYERS) return ibl_set_error(IBL_ERR_ARG, "%s: bad depth", fn);
    return IBL_OK;
}

// what both entries do once their own checks have passed: carve the workspace, validate every block, run the stages
static int forward(const char* fn, const ibl_vit_desc* d, const ibl_vit_weights* w, const void* patches, const float* pos_rows, const int* seq_off,
                   int max_tokens, int64_t rows, int batch, int n_prefix, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    int64_t offs[WS_ALL] = {};
    const int64_t end = vit_layout(d, rows, batch, offs, seq_off ? WS_ALL : IBL_VIT_WS_COUNT);
    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    if ((base - reinterpret_cast<unsigned char*>(workspace)) + end > workspace_bytes) return ibl_set_error(IBL_ERR_ARG, "%s: workspace too small", fn);
    auto ws16 = [&](int i) { return reinterpret_cast<u16*>(base + offs[i]); };
    const VitCtx c{d, w, batch, (hipStream_t)stream, reinterpret_cast<float*>(base + offs[IBL_VIT_WS_X]), ws16(IBL_VIT_WS_XN), ws16(IBL_VIT_WS_QKV),
                   ws16(IBL_VIT_WS_ATT), ws16(IBL_VIT_WS_HID), ws16(IBL_VIT_WS_FIN), rows, act_terms(d), n_prefix, seq_off, max_tokens,
                   seq_off ? reinterpret_cast<float*>(base + offs[WS_CX]) : nullptr, seq_off ? ws16(WS_CA) : nullptr};
    BlockTerms terms[IBL_VIT_MAX_LAYERS];
    int st;
    for (int l = 0; l < d->n_blocks_run; ++l) {
        terms[l] = block_terms(d, w, l);
        if ((st = check_block_terms(fn, l, terms[l], c.at)) != IBL_OK) return st;
    }
    if ((st = embed(c, patches, pos_rows)) != IBL_OK) return st;
    for (int l = 0; l < d->n_blocks_run; ++l) {
        if ((st = attention_half(c, l, terms[l])) != IBL_OK) return st;
        if ((st = mlp_half(c, l, terms[l])) != IBL_OK) return st;
    }
    return head(c, out, d->n_blocks_run > 0 && terms[d->n_blocks_run - 1].cls_only);
}

extern "C" int ibl_vit_forward(const ibl_vit_desc* d, const ibl_vit_weights* w, const void* patches, int batch,
                               float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "ibl_vit_forward";
    const bool any_null = !d || !w || !patches || !out || !workspace, no_cls = !any_null && (d->flags & IBL_VIT_NO_CLS);
    if (no_cls && d->n_registers != 0)
        return ibl_set_error(IBL_ERR_ARG, "%s: n_registers %d with IBL_VIT_NO_CLS: registers follow a class token", fn, d->n_registers);
    int st;
    if ((st = check_desc(fn, d, w, any_null, batch)) != IBL_OK) return st;
    const int T = d->n_tokens, n_prefix = no_cls ? 0 : 1 + d->n_registers;
    if (T - n_prefix < 1) return ibl_set_error(IBL_ERR_ARG, "%s: n_tokens %d leaves no patch row after a prefix of %d", fn, T, n_prefix);
    if (w->rope_table && (reinterpret_cast<uintptr_t>(w->rope_table) & 15)) return ibl_set_error(IBL_ERR_ARG, "%s: rope_table must be 16-byte aligned", fn);
    if (no_cls && !(d->flags & IBL_VIT_OUT_ALL_TOKENS))
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: IBL_VIT_NO_CLS needs IBL_VIT_OUT_ALL_TOKENS: without a class token there is no row to return", fn);
    if (workspace_bytes < ibl_vit_workspace_bytes(d, batch)) return ibl_set_error(IBL_ERR_ARG, "%s: workspace too small", fn);
    return forward(fn, d, w, patches, nullptr, nullptr, T, (int64_t)batch * T, batch, n_prefix, out, workspace, workspace_bytes, stream);
}

extern "C" int ibl_vit_forward_ragged(const ibl_vit_desc* d, const ibl_vit_weights* w, const void* patches, const float* pos_rows,
                                      const int32_t* seq_off_dev, const int32_t* seq_off_host, int batch, float* out, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    const char* fn = "ibl_vit_forward_ragged";
    const bool any_null = !d || !w || !patches || !pos_rows || !seq_off_dev || !seq_off_host || !out || !workspace;
    if (!any_null && batch > 0) {        // what has no position table for every grid, refused ahead of the descriptor's own faults
        if (w->rope_table) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: a rotary table (DINOv3) is not supported: it would have to be ragged too", fn);
        if (d->flags & IBL_VIT_NO_CLS) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: IBL_VIT_NO_CLS (SigLIP) is not supported: a class-token model is needed", fn);
        if (d->flags & (IBL_VIT_PROJ | IBL_VIT_PRE_LN))
            return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: IBL_VIT_PROJ / IBL_VIT_PRE_LN (CLIP) are not supported: its position table is not defined off its grid", fn);
    }
    int st, max_tokens;
    if ((st = check_desc(fn, d, w, any_null, batch)) != IBL_OK) return st;
    if ((reinterpret_cast<uintptr_t>(patches) & 15) || (reinterpret_cast<uintptr_t>(pos_rows) & 15) || (reinterpret_cast<uintptr_t>(seq_off_dev) & 3))
        return ibl_set_error(IBL_ERR_ARG, "%s: patches and pos_rows must be 16-byte, seq_off 4-byte aligned", fn);
    if ((st = ragged_offsets_check(fn, seq_off_host, batch, &max_tokens)) != IBL_OK) return st;
    if (seq_off_host[0] != 0) return ibl_set_error(IBL_ERR_ARG, "%s: seq_off[0] must be 0", fn);
    const int n_prefix = 1 + d->n_registers;
    for (int b = 0; b < batch; ++b)
        if (seq_off_host[b + 1] - seq_off_host[b] <= n_prefix)
            return ibl_set_error(IBL_ERR_ARG, "%s: crop %d has %d rows: no patch row after a prefix of %d", fn, b, seq_off_host[b + 1] - seq_off_host[b], n_prefix);
    return forward(fn, d, w, patches, pos_rows, seq_off_dev, max_tokens, seq_off_host[batch], batch, n_prefix, out, workspace, workspace_bytes, stream);
}
