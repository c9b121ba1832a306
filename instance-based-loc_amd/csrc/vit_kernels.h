// vit_kernels.h -- internal to the ViT encoder: what vit_gemm.hip, vit_layernorm.hip, vit_attention.hip and the forward (vit.hip) share.
// Without relocatable device code a kernel is launched from the file that defines it, so each file offers its kernels as a plain host
// launcher, declared at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "ibl_common.h"
#include "ibloc.h"

typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned short u16;

// fp32 -> fp16 operand, round-to-nearest-even (v_cvt_f16_f32), clamped to the finite range: an activation beyond 65504 would
// otherwise become an infinity and poison the row (not reached by ViT-B activations; the residual stream itself stays fp32)
__device__ __forceinline__ u16 f2h(float f) {
    const _Float16 h = (_Float16)__builtin_amdgcn_fmed3f(f, -65504.0f, 65504.0f);
    return __builtin_bit_cast(u16, h);
}

__device__ __forceinline__ float h2f(u16 h) { return (float)__builtin_bit_cast(_Float16, h); }

// two fp32 -> two fp16 operands in one dword: v_cvt_pk_f16_f32 (gfx950: packed round-to-nearest-even) + packed clamp to the finite range
// (an infinity becomes 65504: the same value f2h gives) -- three instructions per pair where med3 + cvt per element + pack took five
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned f2h_pk(float a, float b) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    h16x2 r = __builtin_convertvector(f32x2_{a, b}, h16x2);
    const h16x2 hi = {(_Float16)65504.0f, (_Float16)65504.0f};
    r = __builtin_elementwise_min(r, hi);
    r = __builtin_elementwise_max(r, -hi);
    return __builtin_bit_cast(unsigned, r);
}

struct GemmEpi {
    const float* bias;      // [N] or null
    const float* scale;     // [N] LayerScale or null (EPI_RESID)
    const float* pos;       // [P][N] position embedding rows for patches (EPI_PATCH)
    void* out;              // fp16 or fp32
    int64_t ldo;            // output row stride (elements)
    int tokens_per_crop;    // T (EPI_PATCH)
    int patches_per_crop;   // P (EPI_PATCH)
    int patch_row0;         // EPI_PATCH: the row of a crop its patch 0 goes to, i.e. the crop's prefix rows (the encoder: T - P -- 1 with a class token, 0 without; ibl_linear_f16_ex: 1, whatever T)
    int accumulate;         // EPI_PATCH: x += alpha * acc instead of x = acc + bias + pos (second weight term of a two-term operand)
    float alpha;
    int algo_k;             // K the in-process timer counts as algorithmic (0: K itself; -1: none -- extra terms of a two-term operand are overhead, not model FLOPs)
};

#define IBL_MFMA(a, b, c, x, y, z) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, x, y, z)

static inline int64_t rows_pad(int64_t r) { return ibl_align_up(r, 128); }

// ---- launchers (not part of the library's surface).  None checks its arguments beyond what it says: the entries and ibl_vit_forward
// validate what they pass.
#define VIT_INTERNAL __attribute__((visibility("hidden")))

// vit_gemm.hip.  epi: IBL_LINEAR_*; act: IBL_ACT_*, non-zero with the three GELU epilogues only (any other pair is refused)
VIT_INTERNAL int gemm_launch(int epi, int act, const u16* A, int64_t lda, const u16* W, int64_t ldw, int M, int N, int K, const GemmEpi& e,
                             hipStream_t s);
VIT_INTERNAL bool gemm_resid_pre();          // $IBL_GEMM_RESID_PRE (lab): IBL_LINEAR_RESID_PRE_F32 where a residual GEMM has no scale vector
// vit_layernorm.hip.  terms 0 = fp32 rows (in place allowed), 1 / 2 / 3 = fp16 rows of that many terms
VIT_INTERNAL int launch_layernorm(const float* x, int64_t ld_x, int64_t n_rows, int dim, const float* g, const float* b, float eps, void* out,
                                  int64_t ld_out, int terms, hipStream_t s);
// vit_attention.hip.  P >= 1, batch >= 1; T <= IBL_ATT_STREAM_MAX_TOKENS or refused
VIT_INTERNAL int run_rope(u16* qkv, const float* table, int B, int T, int n_prefix, int D, int heads, int k_only, hipStream_t s);
VIT_INTERNAL int run_attention(const u16* qkv, u16* out, int B, int T, int D, int heads, int cls_only, hipStream_t s, int terms);
// ragged rows (ibl_attention_ragged_f16, ibl_vit_forward_ragged): the host check of the offsets, which also finds the longest segment,
// and the launch, which takes what that check passed
VIT_INTERNAL int ragged_offsets_check(const char* fn, const int32_t* seq_off, int batch, int* max_tokens);
VIT_INTERNAL int run_attention_ragged(const u16* qkv, u16* out, const int* seq_off, int B, int max_tokens, int D, int heads, int cls_only,
                                      hipStream_t s, int terms);

// ---- what vit.hip and vit_ragged.hip decide alike
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

static inline BlockTerms block_terms(const ibl_vit_desc* d, const ibl_vit_weights* w, int l) {
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
static inline int check_block_terms(const char* fn, int l, const BlockTerms& t, int at) {
    if (t.qkv > 3 || t.fc1 > 3) return ibl_set_error(IBL_ERR_ARG, "%s: layer %d: at most three operand terms", fn, l);
    if (t.o > at || t.fc2 > at || t.o > 3 || t.fc2 > 3)
        return ibl_set_error(IBL_ERR_ARG, "%s: layer %d: o_terms / fc2_terms %d / %d need IBL_VIT_ACT_TERMS%d in the descriptor", fn, l, t.o, t.fc2, t.o > t.fc2 ? t.o : t.fc2);
    return IBL_OK;
}
