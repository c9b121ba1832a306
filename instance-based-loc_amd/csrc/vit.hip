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
// vit_kernels.h.  This file holds the prefix-row kernel, the workspace layout and its two entries, and ibl_vit_forward: a driver over
// one function per stage (embed, attention_half, mlp_half, head).
#include "vit_kernels.h"

// the prefix rows of every crop: x[b*T + 0][:] = cls_pos[:] (cls token + its position embedding), x[b*T + 1 + r][:] = reg[r][:] (register
// tokens, no position embedding); n_prefix = 1 + registers
__global__ void ibl_set_prefix_kernel(float* __restrict__ x, const float* __restrict__ cls_pos, const float* __restrict__ reg, int B, int T,
                                      int n_prefix, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n_prefix * dim) return;
    const int c = (int)(i % dim);
    const int64_t br = i / dim;
    const int b = (int)(br / n_prefix), r = (int)(br % n_prefix);
    x[((int64_t)b * T + r) * dim + c] = r == 0 ? cls_pos[c] : reg[(int64_t)(r - 1) * dim + c];
}

// The workspace layout, in one place: byte offsets of the IBL_VIT_WS_* buffers from the 256-byte-aligned workspace base, each buffer on a
// 256-byte boundary.  ibl_vit_workspace_bytes, ibl_vit_workspace_layout and the forward pass all read this table.  Returns the end.
static int64_t vit_layout(const ibl_vit_desc* d, int batch, int64_t offs[IBL_VIT_WS_COUNT], int64_t* payload = nullptr) {
    const int64_t R = rows_pad((int64_t)batch * d->n_tokens);
    const int at = (d->flags & IBL_VIT_ACT_TERMS3) ? 3 : ((d->flags & IBL_VIT_ACT_TERMS2) ? 2 : 1);   // widest K-extended input of a residual GEMM
    int64_t bytes[IBL_VIT_WS_COUNT];
    bytes[IBL_VIT_WS_X] = R * d->dim * 4;              // residual stream, fp32
    bytes[IBL_VIT_WS_XN] = R * d->dim * 2 * 3;         // LayerNorm output (up to three terms per row, two-term operands of the early blocks)
    bytes[IBL_VIT_WS_QKV] = R * 3 * d->dim * 2;
    bytes[IBL_VIT_WS_ATT] = R * d->dim * 2 * at;       // attention output
    bytes[IBL_VIT_WS_HID] = R * d->mlp_dim * 2 * at;   // MLP hidden layer
    bytes[IBL_VIT_WS_FIN] = rows_pad(batch) * d->dim * 2;      // CLS rows after a LayerNorm (fp16)
    int64_t p = 0, sum = 0;
    for (int i = 0; i < IBL_VIT_WS_COUNT; ++i) {
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
    vit_layout(d, batch, offs, &sum);
    // the size callers have always been asked for: the buffers, fp32 final rows (reserved; nothing is carved for them) and nine alignment
    // gaps -- the base's and the five between the buffers fit in those
    return sum + rows_pad(batch) * d->dim * 4 + 9 * 256;
}

extern "C" int ibl_vit_workspace_layout(const ibl_vit_desc* d, int batch, int64_t* offsets, int n) {
    if (!d || batch <= 0 || !offsets || n < 0 || n > IBL_VIT_WS_COUNT)
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_workspace_layout: bad argument");
    int64_t offs[IBL_VIT_WS_COUNT];
    vit_layout(d, batch, offs);
    for (int i = 0; i < n; ++i) offsets[i] = offs[i];
    return IBL_OK;
}

// The forward: what one call works on, what each block runs with, and one function per stage
struct VitCtx {
    const ibl_vit_desc* d;
    const ibl_vit_weights* w;
    int batch;
    hipStream_t s;
    float* x;                        // the six IBL_VIT_WS_* buffers, carved once from vit_layout
    u16 *xn, *qkv, *att, *hid, *fin;
    int64_t Rn;                      // batch * n_tokens
    int at;                          // widest K-extended input of a residual GEMM the workspace has room for (IBL_VIT_ACT_TERMS*)
    int n_prefix;                    // class token + registers; 0 with IBL_VIT_NO_CLS
};

// What block l runs with: BlockTerms (vit_kernels.h).  In the class-rows-only last block the kernels take row strides, the CLS rows
// are addressed in place (stride T * D).

// patch embedding (conv as GEMM over im2col'ed patches) + position embedding, scattered into x; the prefix rows; CLIP's ln_pre
static int embed(const VitCtx& c, const void* patches) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim, T = d->n_tokens, P = T - c.n_prefix;
    int st;
    GemmEpi e{};
    e.bias = w->b_patch; e.pos = w->pos_patch; e.out = c.x; e.ldo = D; e.tokens_per_crop = T; e.patches_per_crop = P;
    e.patch_row0 = c.n_prefix;         // the patch rows follow the crop's prefix rows: class token and registers
    st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                     reinterpret_cast<const u16*>(w->w_patch), d->patch_k_pad, c.batch * P, D, d->patch_k_pad, e, c.s);
    if (st) return st;
    if (w->w_patch_lo) {             // second term of the patch weights: x += (patches W_lo'^T) / S
        GemmEpi e2 = e;
        e2.bias = nullptr; e2.accumulate = 1; e2.alpha = 1.0f / IBL_VIT_SPLIT_SCALE; e2.algo_k = -1;
        st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                         reinterpret_cast<const u16*>(w->w_patch_lo), d->patch_k_pad, c.batch * P, D, d->patch_k_pad, e2, c.s);
        if (st) return st;
    }
    if (!(d->flags & IBL_VIT_NO_CLS)) {
        const int64_t n = (int64_t)c.batch * c.n_prefix * D;
        hipLaunchKernelGGL(ibl_set_prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, c.x, w->cls_pos, w->reg_tokens, c.batch,
                           T, c.n_prefix, D);
        IBL_LAUNCH_CHECK();
    }
    if (d->flags & IBL_VIT_PRE_LN) {
        // CLIP ln_pre: normalise the residual stream in place (through the fp16-free f32 path)
        st = launch_layernorm(c.x, D, c.Rn, D, w->ln_pre_g, w->ln_pre_b, d->ln_eps, c.x, D, 0, c.s);
        if (st) return st;
    }
    return IBL_OK;
}

// x += scale * (a W'^T + bias): the output projection and fc2.  `terms` > 1: a and W' are K-extended rows, one launch of K' = terms * K
// (w_x).  terms == 1: the plain weights w, and where the layer carries them the (older form) second weight term as its own launch:
// x += (ls / S) * (a W_lo'^T).  a: `rows` rows of stride lda; in a CLS-only block the class rows of x are addressed in place.
static int resid_gemm(const VitCtx& c, bool cls_only, const u16* a, int64_t lda, int rows, int terms, int K, const void* w, const void* w_x,
                      const void* w_lo, const float* bias, const float* ls, const float* ls_lo) {
    const int D = c.d->dim;
    GemmEpi e{};
    e.bias = bias; e.scale = ls; e.out = c.x; e.ldo = cls_only ? (int64_t)c.d->n_tokens * D : D; e.alpha = 1.0f; e.algo_k = K;
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
    const int64_t TD = (int64_t)T * D;
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
        GemmEpi q{};                                  // queries of the CLS rows only
        q.bias = L->b_qkv; q.out = c.qkv; q.ldo = 3 * TD;
        st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.xn, TD, reinterpret_cast<const u16*>(L->w_qkv), D, c.batch, D, D, q, c.s);
        if (st) return st;
    }
    if (c.w->rope_table) {      // DINOv3: q and k of the patch rows rotated in place; the class-rows-only block has no patch-row q to rotate
        st = run_rope(c.qkv, c.w->rope_table, c.batch, T, c.n_prefix, D, H, t.cls_only ? 1 : 0, c.s);
        if (st) return st;
    }
    st = run_attention(c.qkv, c.att, c.batch, T, D, H, t.cls_only ? 1 : 0, c.s, t.o);
    if (st) return st;
    return resid_gemm(c, t.cls_only, c.att, t.cls_only ? TD : (int64_t)t.o * D, t.cls_only ? c.batch : (int)c.Rn, t.o, D, L->w_o, L->w_o_x, L->w_o_lo,
                      L->b_o, L->ls1, L->ls1_lo);
}

// LN2 (the class rows of a CLS-only block go to FIN) -> fc1 + GELU -> x += fc2
static int mlp_half(const VitCtx& c, int l, const BlockTerms& t) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_layer* L = &c.w->layers[l];
    const int D = d->dim;
    int st = t.cls_only ? launch_layernorm(c.x, (int64_t)d->n_tokens * D, c.batch, D, L->ln2_g, L->ln2_b, d->ln_eps, c.fin, D, 1, c.s)
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
    return resid_gemm(c, t.cls_only, c.hid, (int64_t)t.fc2 * d->mlp_dim, mlp_rows, t.fc2, d->mlp_dim, L->w_fc2, L->w_fc2_x, L->w_fc2_lo, L->b_fc2,
                      L->ls2, L->ls2_lo);
}

// x -> out: all tokens (DATOR streams), or the CLS rows -> (final LN) -> (projection) -> out fp32 [batch][out_dim]
static int head(const VitCtx& c, float* out) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim, T = d->n_tokens;
    int st;
    if (d->flags & IBL_VIT_OUT_ALL_TOKENS) {
        // DATOR streams: all tokens, optionally through the final LayerNorm
        if (d->flags & IBL_VIT_FINAL_LN) {
            st = launch_layernorm(c.x, D, c.Rn, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
            if (st) return st;
        } else {
            IBL_HIP_CHECK(hipMemcpyAsync(out, c.x, c.Rn * D * 4, hipMemcpyDeviceToDevice, c.s));
        }
        return IBL_OK;
    }
    if (d->flags & IBL_VIT_PROJ) {
        if (!(d->flags & IBL_VIT_FINAL_LN)) return ibl_set_error(IBL_ERR_UNSUPPORTED, "projection needs final LN");
        GemmEpi e{};
        e.bias = nullptr; e.out = out; e.ldo = d->out_dim;
        if (w->w_proj_x) {           // three-term operands: K' = 3 D, one accumulation (xn is free by now: batch <= R rows of 3 D)
            st = launch_layernorm(c.x, (int64_t)T * D, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, c.xn, (int64_t)3 * D, 3, c.s);
            if (st) return st;
            e.algo_k = D;
            return gemm_launch(IBL_LINEAR_F32, IBL_ACT_GELU_ERF, c.xn, (int64_t)3 * D, reinterpret_cast<const u16*>(w->w_proj_x), (int64_t)3 * D, c.batch,
                               d->out_dim, 3 * D, e, c.s);
        }
        st = launch_layernorm(c.x, (int64_t)T * D, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, c.fin, D, 1, c.s);
        if (st) return st;
        return gemm_launch(IBL_LINEAR_F32, IBL_ACT_GELU_ERF, c.fin, D, reinterpret_cast<const u16*>(w->w_proj), D, c.batch, d->out_dim, D, e, c.s);
    }
    if (d->flags & IBL_VIT_FINAL_LN) {
        st = launch_layernorm(c.x, (int64_t)T * D, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
        if (st) return st;
    } else {
        IBL_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)D * 4, c.x, (size_t)T * D * 4, (size_t)D * 4, c.batch,
                                       hipMemcpyDeviceToDevice, c.s));
    }
    return IBL_OK;
}

extern "C" int ibl_vit_forward(const ibl_vit_desc* d, const ibl_vit_weights* w, const void* patches, int batch,
                               float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!d || !w || !patches || !out || !workspace) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: null pointer");
    if (batch <= 0) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: batch must be positive");
    const bool no_cls = (d->flags & IBL_VIT_NO_CLS) != 0;
    const int D = d->dim, T = d->n_tokens, H = d->heads;
    const int n_reg = d->n_registers, n_prefix = no_cls ? 0 : 1 + n_reg, P = T - n_prefix;
    if (n_reg < 0 || (no_cls && n_reg != 0))
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: n_registers %d%s", n_reg, no_cls ? " with IBL_VIT_NO_CLS: registers follow a class token" : " is negative");
    if (P < 1) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: n_tokens %d leaves no patch row after a prefix of %d", T, n_prefix);
    if (n_reg > 0 && !w->reg_tokens) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: n_registers %d without reg_tokens", n_reg);
    if (w->rope_table && (reinterpret_cast<uintptr_t>(w->rope_table) & 15))
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: rope_table must be 16-byte aligned");
    if (no_cls && !(d->flags & IBL_VIT_OUT_ALL_TOKENS))
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_vit_forward: IBL_VIT_NO_CLS needs IBL_VIT_OUT_ALL_TOKENS: without a class token there is no row to return");
    if ((d->flags & IBL_VIT_QUICK_GELU) && (d->flags & IBL_VIT_TANH_GELU))
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: IBL_VIT_QUICK_GELU and IBL_VIT_TANH_GELU are both set");
    if (no_cls && T < 1) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: n_tokens %d with IBL_VIT_NO_CLS", T);
    if (D != H * 64) return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_vit_forward: head_dim must be 64");
    if (D % 128 || d->mlp_dim % 128 || d->patch_k_pad % 64 || D > 1024)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_vit_forward: dim/mlp_dim %% 128, patch_k_pad %% 64, dim <= 1024");
    if (d->n_blocks_run < 0 || d->n_blocks_run > d->depth || d->depth > IBL_VIT_MAX_LAYERS)
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: bad depth");
    if (workspace_bytes < ibl_vit_workspace_bytes(d, batch))
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: workspace too small");

    int64_t offs[IBL_VIT_WS_COUNT];
    const int64_t end = vit_layout(d, batch, offs);
    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    if ((base - reinterpret_cast<unsigned char*>(workspace)) + end > workspace_bytes)
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: workspace too small");
    auto ws16 = [&](int i) { return reinterpret_cast<u16*>(base + offs[i]); };
    const VitCtx c{d, w, batch, (hipStream_t)stream, reinterpret_cast<float*>(base + offs[IBL_VIT_WS_X]), ws16(IBL_VIT_WS_XN), ws16(IBL_VIT_WS_QKV),
                   ws16(IBL_VIT_WS_ATT), ws16(IBL_VIT_WS_HID), ws16(IBL_VIT_WS_FIN), (int64_t)batch * T,
                   (d->flags & IBL_VIT_ACT_TERMS3) ? 3 : ((d->flags & IBL_VIT_ACT_TERMS2) ? 2 : 1), n_prefix};
    BlockTerms terms[IBL_VIT_MAX_LAYERS];
    int st;
    for (int l = 0; l < d->n_blocks_run; ++l) {
        terms[l] = block_terms(d, w, l);
        if ((st = check_block_terms("ibl_vit_forward", l, terms[l], c.at)) != IBL_OK) return st;
    }
    if ((st = embed(c, patches)) != IBL_OK) return st;
    for (int l = 0; l < d->n_blocks_run; ++l) {
        if ((st = attention_half(c, l, terms[l])) != IBL_OK) return st;
        if ((st = mlp_half(c, l, terms[l])) != IBL_OK) return st;
    }
    return head(c, out);
}
