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
