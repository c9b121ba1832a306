// vit_ragged.hip -- the ViT forward over a batch of crops with different patch grids (native-aspect crops): ibl_vit_forward_ragged and
// ibl_vit_ragged_workspace_bytes.  Crop b owns rows seq_off[b] .. seq_off[b + 1] - 1 of every [total_tokens][...] buffer: its prefix rows
// (class token, registers), then its gh * gw patches.  Everything in the encoder but the attention is row-wise, so the launches are
// those of vit.hip's forward with Rn = total_tokens; the attention is the ragged streaming kernel (vit_attention.hip).  Where the fixed
// forward addresses the class rows in place by the stride T * D, here they are gathered to compact [batch][D] buffers and scattered back:
// the GEMMs and LayerNorms of the class-rows-only last block then run with the fixed forward's M, N, K on rows computed independently.
#include "vit_kernels.h"

// x[seq_off[b] + 0][:] = cls_pos[:], x[seq_off[b] + 1 + r][:] = reg[r][:]: ibl_set_prefix_kernel (vit.hip) with an offset table
__global__ void ibl_set_prefix_ragged_kernel(float* __restrict__ x, const float* __restrict__ cls_pos, const float* __restrict__ reg,
                                             const int* __restrict__ seq_off, int B, int n_prefix, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n_prefix * dim) return;
    const int c = (int)(i % dim);
    const int64_t br = i / dim;
    const int b = (int)(br / n_prefix), r = (int)(br % n_prefix);
    x[((int64_t)seq_off[b] + r) * dim + c] = r == 0 ? cls_pos[c] : reg[(int64_t)(r - 1) * dim + c];
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

enum { RW_X = 0, RW_XN, RW_QKV, RW_ATT, RW_HID, RW_FIN, RW_CX, RW_CA, RW_COUNT };

static int act_terms(const ibl_vit_desc* d) { return (d->flags & IBL_VIT_ACT_TERMS3) ? 3 : ((d->flags & IBL_VIT_ACT_TERMS2) ? 2 : 1); }

// byte offsets of the buffers from the 256-byte-aligned base, each on a 256-byte boundary; returns the end.  The first six are
// ibl_vit_forward's with R = total_tokens rows; CX fp32 [batch][D] the class rows of the residual stream, CA fp16 [batch][D] the class
// rows of q, then of the attention output
static int64_t ragged_layout(const ibl_vit_desc* d, int64_t total_tokens, int batch, int64_t offs[RW_COUNT]) {
    const int64_t R = rows_pad(total_tokens), Bp = rows_pad(batch);
    const int at = act_terms(d);
    int64_t bytes[RW_COUNT];
    bytes[RW_X] = R * d->dim * 4;
    bytes[RW_XN] = R * d->dim * 2 * 3;
    bytes[RW_QKV] = R * 3 * d->dim * 2;
    bytes[RW_ATT] = R * d->dim * 2 * at;
    bytes[RW_HID] = R * d->mlp_dim * 2 * at;
    bytes[RW_FIN] = Bp * d->dim * 2;
    bytes[RW_CX] = Bp * d->dim * 4;
    bytes[RW_CA] = Bp * d->dim * 2;
    int64_t p = 0;
    for (int i = 0; i < RW_COUNT; ++i) {
        p = (p + 255) & ~(int64_t)255;
        offs[i] = p;
        p += bytes[i];
    }
    return p;
}

extern "C" int64_t ibl_vit_ragged_workspace_bytes(const ibl_vit_desc* d, int64_t total_tokens, int batch) {
    if (!d || batch <= 0 || total_tokens < batch || total_tokens > 0x7fffffff) return -1;
    int64_t offs[RW_COUNT];
    return ragged_layout(d, total_tokens, batch, offs) + 256;      // + the gap to the first 256-byte boundary
}

struct RaggedCtx {
    const ibl_vit_desc* d;
    const ibl_vit_weights* w;
    int batch;
    hipStream_t s;
    const int* seq_off;              // [dev]
    int max_tokens;                  // the longest crop
    float *x, *cx;
    u16 *xn, *qkv, *att, *hid, *fin, *ca;
    int64_t Rn;                      // total tokens
    int n_prefix;
};

// bytes: of one class row
static int class_rows(const RaggedCtx& c, void* rows, int64_t ld_rows_bytes, void* compact, int row_bytes, int scatter) {
    const int n16 = row_bytes / 16;
    const int64_t n = (int64_t)c.batch * n16;
    hipLaunchKernelGGL(ibl_class_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, reinterpret_cast<uint4*>(rows),
                       ld_rows_bytes / 16, reinterpret_cast<uint4*>(compact), (int64_t)n16, c.seq_off, c.batch, n16, scatter);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// the patch matrix holds one row per TOKEN (zero prefix rows), so the whole batch is one "crop" of the patch epilogue:
// x[r] = acc + bias + pos_rows[r], the fixed forward's expression; the prefix rows are then overwritten
static int embed(const RaggedCtx& c, const void* patches, const float* pos_rows) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim;
    GemmEpi e{};
    e.bias = w->b_patch; e.pos = pos_rows; e.out = c.x; e.ldo = D; e.tokens_per_crop = (int)c.Rn; e.patches_per_crop = (int)c.Rn; e.patch_row0 = 0;
    int st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                         reinterpret_cast<const u16*>(w->w_patch), d->patch_k_pad, (int)c.Rn, D, d->patch_k_pad, e, c.s);
    if (st) return st;
    if (w->w_patch_lo) {
        GemmEpi e2 = e;
        e2.bias = nullptr; e2.accumulate = 1; e2.alpha = 1.0f / IBL_VIT_SPLIT_SCALE; e2.algo_k = -1;
        st = gemm_launch(IBL_LINEAR_PATCH_F32, IBL_ACT_GELU_ERF, reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                         reinterpret_cast<const u16*>(w->w_patch_lo), d->patch_k_pad, (int)c.Rn, D, d->patch_k_pad, e2, c.s);
        if (st) return st;
    }
    const int64_t n = (int64_t)c.batch * c.n_prefix * D;
    hipLaunchKernelGGL(ibl_set_prefix_ragged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.s, c.x, w->cls_pos, w->reg_tokens,
                       c.seq_off, c.batch, c.n_prefix, D);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// vit.hip's resid_gemm: x += scale * (a W'^T + bias) into `out` rows of stride D (the residual stream, or its compact class rows)
static int resid_gemm(const RaggedCtx& c, bool cls_only, float* out, const u16* a, int64_t lda, int rows, int terms, int K, const void* w,
                      const void* w_x, const void* w_lo, const float* bias, const float* ls, const float* ls_lo) {
    const int D = c.d->dim;
    GemmEpi e{};
    e.bias = bias; e.scale = ls; e.out = out; e.ldo = D; e.alpha = 1.0f; e.algo_k = K;
    const int64_t kx = (int64_t)terms * K;
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

static int attention_half(const RaggedCtx& c, int l, const BlockTerms& t) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_layer* L = &c.w->layers[l];
    const int D = d->dim, H = d->heads;
    int st = launch_layernorm(c.x, D, c.Rn, D, L->ln1_g, L->ln1_b, d->ln_eps, c.xn, (int64_t)t.qkv * D, t.qkv, c.s);
    if (st) return st;
    if (!t.cls_only) {
        GemmEpi e{};
        e.bias = L->b_qkv; e.out = c.qkv; e.ldo = 3 * D; e.algo_k = D;
        st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.xn, (int64_t)t.qkv * D, reinterpret_cast<const u16*>(t.qkv > 1 ? L->w_qkv_x : L->w_qkv),
                         (int64_t)t.qkv * D, (int)c.Rn, 3 * D, t.qkv * D, e, c.s);
        if (st) return st;
        st = run_attention_ragged(c.qkv, c.att, c.seq_off, c.batch, c.max_tokens, D, H, 0, c.s, t.o);
        if (st) return st;
        return resid_gemm(c, false, c.x, c.att, (int64_t)t.o * D, (int)c.Rn, t.o, D, L->w_o, L->w_o_x, L->w_o_lo, L->b_o, L->ls1, L->ls1_lo);
    }
    GemmEpi e{};                                  // keys and values of every token: weight rows D .. 3D
    e.bias = L->b_qkv + D; e.out = c.qkv + D; e.ldo = 3 * D;
    st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.xn, D, reinterpret_cast<const u16*>(L->w_qkv) + (int64_t)D * D, D, (int)c.Rn, 2 * D, D, e, c.s);
    if (st) return st;
    // queries of the class rows: LN1 rows gathered (FIN), projected (CA), scattered into the q columns of their rows
    if ((st = class_rows(c, c.xn, (int64_t)D * 2, c.fin, D * 2, 0)) != IBL_OK) return st;
    GemmEpi q{};
    q.bias = L->b_qkv; q.out = c.ca; q.ldo = D;
    st = gemm_launch(IBL_LINEAR_F16, IBL_ACT_GELU_ERF, c.fin, D, reinterpret_cast<const u16*>(L->w_qkv), D, c.batch, D, D, q, c.s);
    if (st) return st;
    if ((st = class_rows(c, c.qkv, (int64_t)3 * D * 2, c.ca, D * 2, 1)) != IBL_OK) return st;
    st = run_attention_ragged(c.qkv, c.att, c.seq_off, c.batch, c.max_tokens, D, H, 1, c.s, 1);
    if (st) return st;
    // the class rows of the attention output (CA) and of the residual stream (CX), compact from here on
    if ((st = class_rows(c, c.att, (int64_t)D * 2, c.ca, D * 2, 0)) != IBL_OK) return st;
    if ((st = class_rows(c, c.x, (int64_t)D * 4, c.cx, D * 4, 0)) != IBL_OK) return st;
    return resid_gemm(c, true, c.cx, c.ca, D, c.batch, 1, D, L->w_o, L->w_o_x, L->w_o_lo, L->b_o, L->ls1, L->ls1_lo);
}

static int mlp_half(const RaggedCtx& c, int l, const BlockTerms& t) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_layer* L = &c.w->layers[l];
    const int D = d->dim;
    int st = t.cls_only ? launch_layernorm(c.cx, D, c.batch, D, L->ln2_g, L->ln2_b, d->ln_eps, c.fin, D, 1, c.s)
                        : launch_layernorm(c.x, D, c.Rn, D, L->ln2_g, L->ln2_b, d->ln_eps, c.xn, (int64_t)t.fc1 * D, t.fc1, c.s);
    if (st) return st;
    const u16* mlp_in = t.cls_only ? c.fin : c.xn;
    const int mlp_rows = t.cls_only ? c.batch : (int)c.Rn;
    GemmEpi e{};
    e.bias = L->b_fc1; e.out = c.hid; e.ldo = (int64_t)t.fc2 * d->mlp_dim; e.algo_k = D;
    const int epi = t.fc2 == 3 ? IBL_LINEAR_GELU_F16_X3 : (t.fc2 == 2 ? IBL_LINEAR_GELU_F16_X2 : IBL_LINEAR_GELU_F16);
    const int act = (d->flags & IBL_VIT_QUICK_GELU) ? IBL_ACT_QUICK_GELU : ((d->flags & IBL_VIT_TANH_GELU) ? IBL_ACT_GELU_TANH : IBL_ACT_GELU_ERF);
    st = gemm_launch(epi, act, mlp_in, (int64_t)t.fc1 * D, reinterpret_cast<const u16*>(t.fc1 > 1 ? L->w_fc1_x : L->w_fc1), (int64_t)t.fc1 * D, mlp_rows,
                     d->mlp_dim, t.fc1 * D, e, c.s);
    if (st) return st;
    return resid_gemm(c, t.cls_only, t.cls_only ? c.cx : c.x, c.hid, (int64_t)t.fc2 * d->mlp_dim, mlp_rows, t.fc2, d->mlp_dim, L->w_fc2,
                      L->w_fc2_x, L->w_fc2_lo, L->b_fc2, L->ls2, L->ls2_lo);
}

// x -> out: every row, packed (IBL_VIT_OUT_ALL_TOKENS), or the class rows; through the final LayerNorm where the model has one.
// have_cx: the last block left the class rows in CX (it ran class rows only)
static int head(const RaggedCtx& c, float* out, bool have_cx) {
    const ibl_vit_desc* d = c.d;
    const ibl_vit_weights* w = c.w;
    const int D = d->dim;
    int st;
    if (d->flags & IBL_VIT_OUT_ALL_TOKENS) {
        if (d->flags & IBL_VIT_FINAL_LN) return launch_layernorm(c.x, D, c.Rn, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
        IBL_HIP_CHECK(hipMemcpyAsync(out, c.x, c.Rn * D * 4, hipMemcpyDeviceToDevice, c.s));
        return IBL_OK;
    }
    if (!have_cx && (st = class_rows(c, c.x, (int64_t)D * 4, c.cx, D * 4, 0)) != IBL_OK) return st;     // n_blocks_run == 0
    if (d->flags & IBL_VIT_FINAL_LN) return launch_layernorm(c.cx, D, c.batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, c.s);
    IBL_HIP_CHECK(hipMemcpyAsync(out, c.cx, (size_t)c.batch * D * 4, hipMemcpyDeviceToDevice, c.s));
    return IBL_OK;
}

extern "C" int ibl_vit_forward_ragged(const ibl_vit_desc* d, const ibl_vit_weights* w, const void* patches, const float* pos_rows,
                                      const int32_t* seq_off_dev, const int32_t* seq_off_host, int batch, float* out, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    const char* fn = "ibl_vit_forward_ragged";
    if (!d || !w || !patches || !pos_rows || !seq_off_dev || !seq_off_host || !out || !workspace)
        return ibl_set_error(IBL_ERR_ARG, "%s: null pointer", fn);
    if (batch <= 0) return ibl_set_error(IBL_ERR_ARG, "%s: batch must be positive", fn);
    if (w->rope_table) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: a rotary table (DINOv3) is not supported: it would have to be ragged too", fn);
    if (d->flags & IBL_VIT_NO_CLS) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: IBL_VIT_NO_CLS (SigLIP) is not supported: a class-token model is needed", fn);
    if (d->flags & (IBL_VIT_PROJ | IBL_VIT_PRE_LN))
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: IBL_VIT_PROJ / IBL_VIT_PRE_LN (CLIP) are not supported: its position table is not defined off its grid", fn);
    const int D = d->dim, H = d->heads, n_reg = d->n_registers, n_prefix = 1 + n_reg;
    if (n_reg < 0) return ibl_set_error(IBL_ERR_ARG, "%s: n_registers %d is negative", fn, n_reg);
    if (n_reg > 0 && !w->reg_tokens) return ibl_set_error(IBL_ERR_ARG, "%s: n_registers %d without reg_tokens", fn, n_reg);
    if ((d->flags & IBL_VIT_QUICK_GELU) && (d->flags & IBL_VIT_TANH_GELU))
        return ibl_set_error(IBL_ERR_ARG, "%s: IBL_VIT_QUICK_GELU and IBL_VIT_TANH_GELU are both set", fn);
    if (D != H * 64) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: head_dim must be 64", fn);
    if (D % 128 || d->mlp_dim % 128 || d->patch_k_pad % 64 || D > 1024)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: dim/mlp_dim %% 128, patch_k_pad %% 64, dim <= 1024", fn);
    if (d->n_blocks_run < 0 || d->n_blocks_run > d->depth || d->depth > IBL_VIT_MAX_LAYERS) return ibl_set_error(IBL_ERR_ARG, "%s: bad depth", fn);
    if ((reinterpret_cast<uintptr_t>(patches) & 15) || (reinterpret_cast<uintptr_t>(pos_rows) & 15) || (reinterpret_cast<uintptr_t>(seq_off_dev) & 3))
        return ibl_set_error(IBL_ERR_ARG, "%s: patches and pos_rows must be 16-byte, seq_off 4-byte aligned", fn);
    int st, max_tokens;
    if ((st = ragged_offsets_check(fn, seq_off_host, batch, &max_tokens)) != IBL_OK) return st;
    if (seq_off_host[0] != 0) return ibl_set_error(IBL_ERR_ARG, "%s: seq_off[0] must be 0", fn);
    for (int b = 0; b < batch; ++b)
        if (seq_off_host[b + 1] - seq_off_host[b] <= n_prefix)
            return ibl_set_error(IBL_ERR_ARG, "%s: crop %d has %d rows: no patch row after a prefix of %d", fn, b, seq_off_host[b + 1] - seq_off_host[b], n_prefix);
    const int64_t Rn = seq_off_host[batch];
    int64_t offs[RW_COUNT];
    const int64_t end = ragged_layout(d, Rn, batch, offs);
    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    if ((base - reinterpret_cast<unsigned char*>(workspace)) + end > workspace_bytes) return ibl_set_error(IBL_ERR_ARG, "%s: workspace too small", fn);
    auto ws16 = [&](int i) { return reinterpret_cast<u16*>(base + offs[i]); };
    const RaggedCtx c{d, w, batch, (hipStream_t)stream, seq_off_dev, max_tokens, reinterpret_cast<float*>(base + offs[RW_X]),
                      reinterpret_cast<float*>(base + offs[RW_CX]), ws16(RW_XN), ws16(RW_QKV), ws16(RW_ATT), ws16(RW_HID), ws16(RW_FIN),
                      ws16(RW_CA), Rn, n_prefix};
    BlockTerms terms[IBL_VIT_MAX_LAYERS];
    const int at = act_terms(d);
    for (int l = 0; l < d->n_blocks_run; ++l) {
        terms[l] = block_terms(d, w, l);
        if ((st = check_block_terms(fn, l, terms[l], at)) != IBL_OK) return st;
    }
    if ((st = embed(c, patches, pos_rows)) != IBL_OK) return st;
    for (int l = 0; l < d->n_blocks_run; ++l) {
        if ((st = attention_half(c, l, terms[l])) != IBL_OK) return st;
        if ((st = mlp_half(c, l, terms[l])) != IBL_OK) return st;
    }
    return head(c, out, d->n_blocks_run > 0 && terms[d->n_blocks_run - 1].cls_only);
}
