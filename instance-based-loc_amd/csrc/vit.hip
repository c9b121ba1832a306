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
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <atomic>

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

// ------------------------------------------------------------------------------------------------
// GEMM  C[M][N] = A[M][K] * W[N][K]^T  (+ epilogue)
// ------------------------------------------------------------------------------------------------
enum { EPI_BIAS_H16 = 0, EPI_BIAS_GELU_H16 = 1, EPI_RESID_F32 = 2, EPI_PATCH_F32 = 3, EPI_BIAS_F32 = 4,
       // x += alpha * (a W^T + bias), alpha a power of two, with the residual tile PRELOADED into the accumulators: the MFMA chain starts
       // from (x + bias) / alpha and the epilogue is 32 plain stores per lane -- no read-modify-write after the K loop (round 4)
       EPI_RESID_PRE_F32 = 5,
       // EPI_BIAS_GELU_H16 writing K-extended operand rows for the next GEMM (round 4; ldo = terms * N):
       //   KX2: [h | h / S]  (fc2 weights in two terms)     KX3: [h | (value - h) * S | h / S]  (+ the hidden layer's second term)
       EPI_BIAS_GELU_H16KX2 = 6, EPI_BIAS_GELU_H16KX3 = 7,
       // internal (not in ibloc.h's enum; reached through ibl_linear_desc.activation and IBL_VIT_QUICK_GELU): epilogues 1, 6 and 7 with
       // QuickGELU, v * sigmoid(1.702 v), in place of the erf form -- everything after the activation is the same code
       EPI_BIAS_QGELU_H16 = 8, EPI_BIAS_QGELU_H16KX2 = 9, EPI_BIAS_QGELU_H16KX3 = 10,
       // likewise internal (ibl_linear_f16_act's IBL_ACT_GELU_TANH and IBL_VIT_TANH_GELU): the three with the tanh form of GELU (SigLIP)
       EPI_BIAS_TGELU_H16 = 11, EPI_BIAS_TGELU_H16KX2 = 12, EPI_BIAS_TGELU_H16KX3 = 13 };

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

constexpr int GBK = 64;                 // K granule every caller guarantees (K % 64 == 0)

// LDS images: a tile row holds 8 chunks of 16 bytes; chunk c of row r lives at chunk c ^ key(r).
//   activation tile: key = r & 7            (fragment rows are consecutive -> conflict-free ds_read_b128)
//   weight tile:     key = ((r >> 4) & 3) * 2 + ((r >> 1) & 1)   (fragment rows are 16a + 4j + b, see below)
__device__ __forceinline__ int key_act(int r) { return r & 7; }
__device__ __forceinline__ int key_w(int r) { return (((r >> 4) & 3) << 1) | ((r >> 1) & 1); }
__device__ __forceinline__ int key_pair(int r) { return (((r >> 3) & 3) << 1) | ((r >> 1) & 1); }   // rows 8 a + 4 b + c, a = 0..3, c = 0..3

// C[M][N] = A[M][K] * W[N][K]^T.  Block tile (2 * MI * 16) x (WN * 64) x 64, one wave per (MI * 16) x 64 sub-tile, two LDS stages.
// Two shapes (launch_gemm chooses from M and N):
//   T256 (MI = 8, WN = 4): 256 x 256, 512 threads, 128 KiB LDS, 1 block / CU, software-pipelined K loop, persistent grid
//                          -- N % 256 == 0; halves the operand traffic per FLOP (the 128 x 128 form saturates the L2 path at ~7 TB/s)
//   else (MI = 4, WN = 2): 128 x 128, 256 threads,  64 KiB LDS, 2 blocks / CU, plain two-stage loop, one block per tile -- any N % 128 == 0
// Every other tile shape, K granule and stage count that was built lost on every ViT-B shape: DESIGN.md records them.
// The MFMA computes the TRANSPOSED tile (W is the A operand, the activations the B operand) and MFMA row 4*fg + r of
// n-tile j is mapped to weight row 16*fg + 4*j + r, so that every lane ends up with 16 CONSECUTIVE output columns of one
// output row: the epilogue is 16-byte vector stores.  Operand tiles are staged with direct-to-LDS loads
// (buffer_load_dwordx4 ... offen lds): one wave instruction writes 1 KiB = 8 tile rows linearly, so the XOR swizzle is applied
// to the per-lane SOURCE offset.
// Exact-form GELU, 0.5 v (1 + erf(v / sqrt 2)), with erfc from Abramowitz & Stegun 7.1.26 (|error| < 1.5e-7 in erf, two orders
// below the fp16 rounding of the stored activation; libm's erff costs ~35 VALU instructions per element, which made the
// fc1 epilogue as long as its K loop).
// Two elements at a time on the packed fp32 pipe (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: two lanes of arithmetic per
// instruction).  The sign select of erf is folded away with |v| = sqrt(2) z:
//   0.5 v (1 + erf(v / sqrt 2)) = 0.5 v + 0.5 |v| (1 - erfc(z)) = 0.5 v + (z / sqrt 2) (1 - erfc(z))
// (for v << 0 the two terms cancel to an absolute error of ~|v| 6e-8, three orders below the fp16 rounding of the row's other
// activations).  13 packed + 3 scalar operations per pair against 19 scalar per element of the one-at-a-time form: the fc1 epilogue
// was VALU-bound.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 v) {
    f32x2 z;
    z.x = fabsf(v.x) * 0.70710678118654752f;
    z.y = fabsf(v.y) * 0.70710678118654752f;
    const f32x2 d = z * 0.3275911f + 1.0f;
    f32x2 t;
    t.x = __builtin_amdgcn_rcpf(d.x);
    t.y = __builtin_amdgcn_rcpf(d.y);
    f32x2 p = t * 1.061405429f + -1.453152027f;
    p = p * t + 1.421413741f;
    p = p * t + -0.284496736f;
    p = p * t + 0.254829592f;
    const f32x2 a = (z * -1.4426950408889634f) * z;
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(a.x);
    e.y = __builtin_amdgcn_exp2f(a.y);
    const f32x2 u = 1.0f - (p * t) * e;                       // erf(z)
    return (z * u) * 0.70710678118654752f + v * 0.5f;
}

// QuickGELU (OpenAI CLIP), v * sigmoid(1.702 v) = v * rcp(1 + exp2(c v)) with c = -1.702 log2(e): two packed operations and an exp2
// and a rcp per element.  v << 0: exp2 overflows to +inf, rcp gives 0 and the result is -0 (the true value lies below the fp16
// subnormals from v = -13 on); v >> 0: the result is v.  r is in [0, 1] and v finite, so no finite v gives a NaN.
__device__ __forceinline__ f32x2 quick_gelu2(f32x2 v) {
    const f32x2 a = v * -2.4554669595930157f;
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(a.x);
    e.y = __builtin_amdgcn_exp2f(a.y);
    const f32x2 d = e + 1.0f;
    f32x2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
    return v * r;
}

// tanh GELU (gelu_pytorch_tanh: SigLIP), 0.5 v (1 + tanh(z)) with z = sqrt(2 / pi) (v + 0.044715 v^3).  1 + tanh(z) = 2 / (1 + exp(-2 z)), so the
// value is v * rcp(1 + exp2(c w)) with w = v (1 + 0.044715 v^2) and c = -2 log2(e) sqrt(2 / pi): the shape of quick_gelu2 with a cubic in
// front -- a packed multiply, a packed fma, two more packed multiplies, an exp2 and a rcp per element.  v << 0 (from v = -10.07 on, c w >= 128):
// exp2 overflows to +inf, rcp gives 0 and the result is -0; v >> 0: exp2 underflows to 0 and the result is v.  v^2 may overflow to +inf
// (|v| > 1.8e19): w is then +-inf with the sign of v and both ends behave as above.  r is in [0, 1] and v finite, so no finite v gives a NaN.
__device__ __forceinline__ f32x2 tanh_gelu2(f32x2 v) {
    const f32x2 u = v * v;
    const f32x2 k = u * 0.044715f + 1.0f;
    const f32x2 w = v * k;
    const f32x2 a = w * -2.3022081985131374f;
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(a.x);
    e.y = __builtin_amdgcn_exp2f(a.y);
    const f32x2 d = e + 1.0f;
    f32x2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
    return v * r;
}

#ifdef IBL_GEMM_STAMPS     // lab builds only (tools/perf_gemm.py --stamps): phase clocks of every tile a (persistent) block walks
// [block < 512][tile iteration < 16][4]: 0 = tile loop top, 1 = first stage landed (after the barrier), 2 = K loop done, 3 = epilogue issued
__device__ long long ibl_gemm_stamps[512 * 16 * 4];
__device__ int ibl_gemm_stamp_iter[512];
#define GEMM_STAMP(k)                                                                                  \
    do {                                                                                               \
        if (threadIdx.x == 0 && blockIdx.x < 512 && stamp_it < 16)                                     \
            ibl_gemm_stamps[(blockIdx.x * 16 + stamp_it) * 4 + (k)] = (long long)__builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int ibl_gemm_stamps_read(long long* dst, int n) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(ibl_gemm_stamps), sizeof(long long) * n) == hipSuccess ? 0 : -1;
}
extern "C" int ibl_gemm_stamps_clear() {
    static long long zeros[512 * 16 * 4];
    return hipMemcpyToSymbol(HIP_SYMBOL(ibl_gemm_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : -1;
}
#else
#define GEMM_STAMP(k)
#endif

#define IBL_MFMA(a, b, c, x, y, z) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, x, y, z)

template <int EPI, bool T256>
__global__ __launch_bounds__(T256 ? 512 : 256, T256 ? 1 : 2) void ibl_gemm_f16_tn(const u16* __restrict__ A, int64_t lda, const u16* __restrict__ W,
                                                                                int64_t ldw, int M, int N, int K, GemmEpi epi) {
#if defined(__HIP_DEVICE_COMPILE__)          // the buffer-resource type and builtins exist in the device pass only
    constexpr int MI = T256 ? 8 : 4, WM = 2, WN = T256 ? 4 : 2, BK = GBK, NS = 2;      // NS: LDS stages
    constexpr bool PIPE = T256;              // the 256 x 256 shape is the pipelined, persistent one
    constexpr int BM = WM * MI * 16, BN = WN * 64, NW = WM * WN;
    constexpr int LDS_ROW = BK * 2;          // bytes per tile row, XOR-swizzled 16-byte chunks (no padding)
    constexpr int CPR = BK / 8, RPI = 64 / CPR;             // chunks per row; rows per 1 KiB wave instruction
    constexpr int A_BYTES = BM * LDS_ROW, W_BYTES = BN * LDS_ROW, STAGE = A_BYTES + W_BYTES;
    constexpr int GA = BM / RPI / NW, GW = BN / RPI / NW;   // 1 KiB wave instructions per wave and stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    // fp32 read-modify-write epilogue: MFMA row 4 fg + r of n-tile j is weight row 16 j + 4 fg + r (natural order), so that one
    // wave instruction covers 64 contiguous bytes of each of its 16 output rows; with the 16-consecutive-columns-per-lane map
    // of the fp16 epilogues every float4 instruction touched 64 separate cache lines and the address coalescer (not HBM) bound
    // the epilogue: 52 k clocks per tile, more than the projection's K loop.
    constexpr bool NAT = EPI == EPI_RESID_F32 || EPI == EPI_RESID_PRE_F32;
    constexpr bool PRE = EPI == EPI_RESID_PRE_F32;
    // fp16 epilogues: MFMA row 4 fg + r of n-tile j is weight row 32 (j / 2) + 8 fg + 4 (j % 2) + r: a lane owns 8 consecutive
    // columns (one 16-byte store) of n-tile pair j / 2 and the four lane groups cover 64 contiguous bytes of the row
    constexpr bool QGELU = EPI == EPI_BIAS_QGELU_H16 || EPI == EPI_BIAS_QGELU_H16KX2 || EPI == EPI_BIAS_QGELU_H16KX3;
    constexpr bool TGELU = EPI == EPI_BIAS_TGELU_H16 || EPI == EPI_BIAS_TGELU_H16KX2 || EPI == EPI_BIAS_TGELU_H16KX3;
    constexpr int GT = (EPI == EPI_BIAS_GELU_H16KX3 || EPI == EPI_BIAS_QGELU_H16KX3 || EPI == EPI_BIAS_TGELU_H16KX3) ? 3
                       : ((EPI == EPI_BIAS_GELU_H16KX2 || EPI == EPI_BIAS_QGELU_H16KX2 || EPI == EPI_BIAS_TGELU_H16KX2) ? 2 : 1);     // column blocks the fp16 epilogue writes
    constexpr bool GELU = EPI == EPI_BIAS_GELU_H16 || GT > 1 || QGELU || TGELU;
    constexpr bool PAIR = EPI == EPI_BIAS_H16 || GELU;
    constexpr int PAIR_STORES = GT * 2 * MI;          // stores per lane of a full tile's fp16 epilogue
#define KEYW(r) (NAT ? key_act(r) : (PAIR ? key_pair(r) : key_w(r)))
    const int nbn = N / BN;
    const int nbm = (M + BM - 1) / BM;
    const int nwg = nbn * nbm;
    // source of piece i: a buffer resource on the tile's first row (SGPRs) + a per-lane 32-bit byte offset + the K offset (SGPR):
    // buffer_load_dwordx4 ... offen lds needs no 64-bit address pair per piece (16 VGPRs with global_load_lds)
    __amdgpu_buffer_rsrc_t a_rsrc, w_rsrc;
    unsigned a_off[GA], w_off[GW];
    int row0, col0;
    // tile t of the launch -> (row0, col0) and this wave's source addresses.  XCD-aware remap: consecutive tiles along N (sharing
    // the A panel) stay on one XCD's L2 (t % 8 labels the XCD for the one-shot grid and for the persistent one, whose stride is a
    // multiple of 8)
#define GEMM_SET_TILE(t)                                                                           \
    do {                                                                                           \
        int _bid = (t);                                                                            \
        {                                                                                          \
            const int _q = nwg / 8, _r = nwg % 8, _xcd = _bid % 8;                                 \
            _bid = (_xcd < _r ? _xcd * (_q + 1) : _r * (_q + 1) + (_xcd - _r) * _q) + _bid / 8;    \
        }                                                                                          \
        row0 = (_bid / nbn) * BM;                                                                  \
        col0 = (_bid % nbn) * BN;                                                                  \
        a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (int64_t)row0 * lda), 0, -1, 0x00020000); \
        w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (int64_t)col0 * ldw), 0, -1, 0x00020000); \
        _Pragma("unroll") for (int _i = 0; _i < GA; ++_i) {                                        \
            const int _rr = (wave + NW * _i) * RPI + lane / CPR, _pch = lane % CPR;                \
            int _ar = _rr;                                                                         \
            if (row0 + _ar >= M) _ar = M - 1 - row0;                                               \
            a_off[_i] = (unsigned)(((int64_t)_ar * lda + ((_pch ^ key_act(_rr)) << 3)) * 2);  \
        }                                                                                          \
        _Pragma("unroll") for (int _i = 0; _i < GW; ++_i) {                                        \
            const int _rr = (wave + NW * _i) * RPI + lane / CPR, _pch = lane % CPR;                \
            w_off[_i] = (unsigned)(((int64_t)_rr * ldw + ((_pch ^ KEYW(_rr)) << 3)) * 2);          \
        }                                                                                          \
    } while (0)
    int tile = blockIdx.x;
    GEMM_SET_TILE(tile);
#define GEMM_GLDS(buf, kt)                                                                                              \
    do {                                                                                                                \
        const int64_t _ko = (int64_t)(kt) * BK;                                                                         \
        _Pragma("unroll") for (int _i = 0; _i < GA; ++_i)                                                               \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(smem + (buf) * STAGE + (wave + NW * _i) * 1024), \
                                                     16, a_off[_i], (unsigned)(_ko * 2), 0, 0);                          \
        _Pragma("unroll") for (int _i = 0; _i < GW; ++_i)                                                               \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (__attribute__((address_space(3))) void*)(smem + (buf) * STAGE + A_BYTES + (wave + NW * _i) * 1024), \
                                                     16, w_off[_i], (unsigned)(_ko * 2), 0, 0);                          \
    } while (0)

    f32x4 acc[MI][4];      // [m-tile i][n-tile j]
    const int nk = K / BK;
    constexpr int NP = GA + GW;
    const int fr = lane & 15, fg = lane >> 4;
    int arow[MI], wrow[4];
#pragma unroll
    for (int i = 0; i < MI; ++i) arow[i] = wm * (MI * 16) + i * 16 + fr;              // activation row (B operand column)
#pragma unroll
    for (int j = 0; j < 4; ++j)                   // weight row of MFMA row fr in n-tile j
        wrow[j] = NAT ? wn * 64 + 16 * j + fr
                      : (PAIR ? wn * 64 + 32 * (j >> 1) + 8 * (fr >> 2) + 4 * (j & 1) + (fr & 3) : wn * 64 + 16 * (fr >> 2) + 4 * j + (fr & 3));
#define GEMM_PIECE(stage, pc)                                                                                                       \
    do {                                                                                                                            \
        const int64_t _ko = (int64_t)(stage) * BK;                                                                                  \
        unsigned char* _dst = smem + ((stage) & 1) * STAGE;                                                                         \
        if ((pc) < GA)                                                                                                              \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(_dst + (wave + NW * (pc)) * 1024), 16,   \
                                                     a_off[(pc) < GA ? (pc) : 0], (unsigned)(_ko * 2), 0, 0);                               \
        else                                                                                                                        \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (__attribute__((address_space(3))) void*)(_dst + A_BYTES + (wave + NW * ((pc) - GA)) * 1024), \
                                                     16, w_off[(pc) >= GA ? (pc) - GA : 0], (unsigned)(_ko * 2), 0, 0);                     \
    } while (0)
#define FRAG_W(buf, ks, j) (*reinterpret_cast<const h16x8*>(smem + (buf) * STAGE + A_BYTES + wrow[j] * LDS_ROW + (((4 * (ks) + fg) ^ KEYW(wrow[j])) << 4)))
#define FRAG_A(buf, ks, i) (*reinterpret_cast<const h16x8*>(smem + (buf) * STAGE + arow[i] * LDS_ROW + (((4 * (ks) + fg) ^ key_act(arow[i])) << 4)))
    // The pipelined form is launched as a persistent grid (one workgroup per CU walks the tiles t, t + grid, ...): the next tile's
    // first stage is requested before the epilogue of the current one, so its latency hides under the stores.
    static_assert(MI % 2 == 0, "pipelined loop: groups in halves");
    constexpr int HA = MI / 4, N2B = MI - HA;                     // groups before / after the barrier in the second K half
    constexpr int NL = MI + 4;                                    // fragment reads per K half
    constexpr int LB = (NL + MI - 2) / (MI - 1);                  // set-B reads per phase-1 group (none after the last group)
    constexpr int LA = (NL + N2B - 2) / (N2B - 1);                // set-A reads per phase-2b group (none before the last group)
    constexpr int NSLOT = N2B + MI;
    static_assert(!PIPE || NP <= 2 * NSLOT, "pieces per stage exceed the slots of a step");
    bool first_tile = true;
    bool stores_pending = false;      // the previous tile's epilogue issued exactly 2 * MI stores per lane after this tile's first pieces
#ifdef IBL_GEMM_STAMPS
    int stamp_it = 0;
#endif
    for (;;) {
    GEMM_STAMP(0);
    if constexpr (PRE) {
        // Residual tile -> accumulators.  Per-tile stamps (round 4): the fp32 read-modify-write AFTER the K loop cost 38 k clocks of a proj
        // tile's 85 k (eight dependent rounds of 4 loads / 4 stores per lane, each waiting for the previous round's stores: vmcnt counts
        // stores on gfx9).  Here the 32 float4 of the tile are requested at the tile top, where the wait for the first operand stage
        // already sits, and the epilogue only stores.  Lane (fr, fg): rows row0 + wm * 128 + 16 i + fr, columns col0 + wn * 64 + 16 j +
        // 4 fg .. + 3 (rows beyond M read row M - 1; their lanes store nothing).
        const int nbp = col0 + wn * 64 + 4 * fg;
        const float ia = 1.0f / epi.alpha;                    // alpha is a power of two: exact
        if (row0 + BM <= M) {
            const float* const xb = reinterpret_cast<const float*>(epi.out) + (int64_t)(row0 + wm * (MI * 16) + fr) * epi.ldo + nbp;
            const int64_t gstride = 16 * epi.ldo;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 x4 = *reinterpret_cast<const float4*>(xb + i * gstride + 16 * j);
                    acc[i][j] = f32x4{x4.x, x4.y, x4.z, x4.w};
                }
        } else {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                int row = row0 + wm * (MI * 16) + i * 16 + fr;
                row = row < M ? row : M - 1;
                const float* xr = reinterpret_cast<const float*>(epi.out) + (int64_t)row * epi.ldo + nbp;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 x4 = *reinterpret_cast<const float4*>(xr + 16 * j);
                    acc[i][j] = f32x4{x4.x, x4.y, x4.z, x4.w};
                }
            }
        }
        if (epi.bias) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 b4 = *reinterpret_cast<const float4*>(epi.bias + nbp + 16 * j);
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    acc[i][j][0] += b4.x; acc[i][j][1] += b4.y; acc[i][j][2] += b4.z; acc[i][j][3] += b4.w;
                }
            }
        }
        if (epi.alpha != 1.0f) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] *= ia;
        }
        // (the compiler's own wait for these loads lands here, before the K loop: without the empty asm it would sit in front of the
        // first MFMA of every accumulator, i.e. between the direct-to-LDS pieces of the first K step, as vmcnt(0))
#pragma unroll
        for (int i = 0; i < MI; ++i)
            asm volatile("" : "+v"(acc[i][0]), "+v"(acc[i][1]), "+v"(acc[i][2]), "+v"(acc[i][3]));
    } else {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (PIPE) {
        // Software-pipelined K loop (BK = 64, two LDS stages, two fragment register sets).  One K step of a wave:
        //   phase 1   MI groups of 4 MFMAs on the step's first K half (set A), the reads of its second half (set B) between them
        //   phase 2a  MI / 2 groups on set B
        //   wait for this wave's pieces of the NEXT stage, workgroup barrier
        //   phase 2b  MI / 2 groups on set B, the reads of the next stage's first half (set A) between them
        // so that no MFMA waits on an LDS read issued just before it (the compiler's own schedule of the plain loop read each
        // fragment pair right before its use: five exposed LDS round trips per step, in all eight waves at once).  The direct-to-LDS
        // pieces of stage s + 2 overwrite the buffer of stage s: the first half of them is issued in phase 2b of step s (every wave has
        // passed the barrier, so every wave's reads of that buffer have returned), the rest in phase 1 of step s + 1; they have a
        // whole step to land before the wait that precedes the barrier of step s + 1.
        // Piece slots: one after each MFMA group of phase 2b (stage kt + 2) and of phase 1 (stage kt + 1, i.e. the same stage one step
        // later); slot u carries piece u, the pieces beyond the slot count ride on the first slots.  (Giving the two waves of a SIMD
        // alternate slots, so that one issues MFMAs while the other waits on its piece, measured 4 % slower.)
#define GEMM_SLOT(u, stage)                                                                        \
    do {                                                                                           \
        if ((u) < NP) GEMM_PIECE(stage, (u) < NP ? (u) : 0);                                       \
        if (NSLOT + (u) < NP) GEMM_PIECE(stage, NSLOT + (u) < NP ? NSLOT + (u) : 0);               \
    } while (0)
#define GEMM_PROLOGUE()                                                                            \
    do {                                                                                           \
        _Pragma("unroll") for (int _pc = 0; _pc < NP; ++_pc) GEMM_PIECE(0, _pc);                   \
        if (nk > 1) {                                   /* the phase-2b slots of a step before the first */ \
            _Pragma("unroll") for (int _g = 0; _g < N2B; ++_g) GEMM_SLOT(_g, 1);                   \
        }                                                                                          \
    } while (0)
        if (first_tile) GEMM_PROLOGUE();
        // fp16 epilogues: the 2 * MI stores of the previous (full) tile were issued AFTER this tile's first pieces, so "at most 2 * MI
        // operations outstanding" already means the pieces have landed (vmcnt retires in issue order): the stores drain under the first K
        // step instead of in front of it (a raw barrier: __syncthreads() would add its own vmcnt(0) while LDS-DMA is pending).  The count
        // holds only while the compiler adds no scratch access of its own: the build fails if this kernel spills (csrc/Makefile)
        if (PAIR && stores_pending) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PAIR_STORES) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        GEMM_STAMP(1);
        __builtin_amdgcn_sched_barrier(0);
        h16x8 afA[MI], wfA[4], afB[MI], wfB[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wfA[j] = FRAG_W(0, 0, j);
#pragma unroll
        for (int i = 0; i < MI; ++i) afA[i] = FRAG_A(0, 0, i);
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            const bool more1 = kt + 1 < nk, more2 = kt + 2 < nk;
            // ---- phase 1: read t of a K half is weight fragment t / 2 (t even, t < 8) or the next activation fragment
#pragma unroll
            for (int g = 0; g < MI; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[g][j] = IBL_MFMA(wfA[j], afA[g], acc[g][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);         // reads after the group: the wait before it then covers set A only
#pragma unroll
                for (int t = g * LB; t < (g + 1) * LB && t < NL; ++t) {
                    if (t < 8 && (t & 1) == 0) wfB[t / 2] = FRAG_W(buf, 1, t / 2);
                    else afB[t < 8 ? t / 2 : t - 4] = FRAG_A(buf, 1, t < 8 ? t / 2 : t - 4);
                }
                if (more1) GEMM_SLOT(N2B + g, kt + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- phase 2a
#pragma unroll
            for (int g = 0; g < HA; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[g][j] = IBL_MFMA(wfB[j], afB[g], acc[g][j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // this wave's pieces have landed, its set-B reads have returned
            __syncthreads();
            // ---- phase 2b
            const int nb = buf ^ 1;
#pragma unroll
            for (int g = 0; g < N2B; ++g) {
                if (more1) {
#pragma unroll
                    for (int t = g * LA; t < (g + 1) * LA && t < NL; ++t) {
                        if (t < 8 && (t & 1) == 0) wfA[t / 2] = FRAG_W(nb, 0, t / 2);
                        else afA[t < 8 ? t / 2 : t - 4] = FRAG_A(nb, 0, t < 8 ? t / 2 : t - 4);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[HA + g][j] = IBL_MFMA(wfB[j], afB[HA + g], acc[HA + g][j], 0, 0, 0);
                if (more2) GEMM_SLOT(g, kt + 2);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
    // NS LDS stages: the loads of K steps 0 .. NS - 2 are in flight before the loop, step kt issues those of step kt + NS - 1
    static_assert(NS == 2, "the vmcnt(0) that closes a step leaves no later stage in flight");
#pragma unroll
    for (int st = 0; st < NS - 1; ++st)
        if (st < nk) GEMM_GLDS(st, st);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    GEMM_STAMP(1);
    // One K step = 2 * MI groups of 4 MFMAs.  The GA + GW direct-to-LDS pieces of the NEXT tile are issued one at a time
    // between those groups: a piece blocks its wave's issue port for ~100 cycles, and eight of them back to back at the top
    // of the step (right after the barrier, in every wave at once) left the MFMA pipe idle for a third of the step.
    constexpr int KS = BK / 32, NG = KS * MI;                      // K halves (one MFMA deep each), MFMA groups per step
    constexpr int NGI = NG / 2;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt % NS;
        const bool more = kt + NS - 1 < nk;
        const int64_t ko = (int64_t)(kt + NS - 1) * BK;
        unsigned char* nxt = smem + ((kt + NS - 1) % NS) * STAGE;
        const unsigned char* pa = smem + buf * STAGE;
        const unsigned char* pw = pa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ch = 4 * ks + fg;
            h16x8 af[MI], wf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const h16x8*>(pw + wrow[j] * LDS_ROW + ((ch ^ KEYW(wrow[j])) << 4));
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *reinterpret_cast<const h16x8*>(pa + arow[i] * LDS_ROW + ((ch ^ key_act(arow[i])) << 4));
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = IBL_MFMA(wf[j], af[i], acc[i][j], 0, 0, 0);
                const int g = ks * MI + i;
#pragma unroll
                // pieces are issued over the first half of the step's groups: one issued in the last groups has not landed at the
                // vmcnt(0) that closes the step (744 -> 760 TFLOP/s per layer; the first quarter only: 753)
                for (int pc = (g < NGI ? g * NP / NGI : NP); pc < (g < NGI ? (g + 1) * NP / NGI : NP); ++pc) {
                    if (more) {
                        if (pc < GA)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(nxt + (wave + NW * pc) * 1024), 16,
                                                                     a_off[pc], (unsigned)(ko * 2), 0, 0);
                        else
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (__attribute__((address_space(3))) void*)(nxt + A_BYTES + (wave + NW * (pc - GA)) * 1024), 16,
                                                                     w_off[pc - GA], (unsigned)(ko * 2), 0, 0);
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // stage kt + NS - 1 has landed
        __syncthreads();
    }
    }
    GEMM_STAMP(2);
    // the tile this block computes next: its first stage is requested now (both LDS buffers are free: every wave's last LDS read
    // returned before the barrier of the final K step)
    const int erow0 = row0, ecol0 = col0;
    // fp16 epilogues: this lane's 16 bias values are fetched -- and waited for -- BEFORE the next tile's direct-to-LDS pieces are issued.
    // Round 4 (per-tile stamps, tools/perf_gemm.py --stamps): "prologue of the next tile + epilogue" took 12.9 k of a qkv tile's 51 k
    // clocks although it stores 128 KB.  The bias loads used to follow the pieces, and with LDS-DMA pieces in flight the compiler waits
    // vmcnt(0) at every use of an ordinary load's result -- in each of the eight per-row-group blocks (`if (row >= M) continue`), i.e.
    // also for the previous group's STORES to complete: eight exposed store latencies per tile.  Now: bias first (the empty asm consumes
    // the registers, so the compiler's wait sits here, with nothing else outstanding), then the pieces, then branch-free stores.
    float bb[2][8];
    if constexpr (PAIR) {
        const int nbp = ecol0 + wn * 64 + 8 * fg;
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 b4 = epi.bias ? *reinterpret_cast<const float4*>(epi.bias + nbp + 32 * j2 + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
                bb[j2][4 * h] = b4.x; bb[j2][4 * h + 1] = b4.y; bb[j2][4 * h + 2] = b4.z; bb[j2][4 * h + 3] = b4.w;
            }
        asm volatile("" ::"v"(bb[0][0]), "v"(bb[0][1]), "v"(bb[0][2]), "v"(bb[0][3]), "v"(bb[0][4]), "v"(bb[0][5]), "v"(bb[0][6]), "v"(bb[0][7]),
                     "v"(bb[1][0]), "v"(bb[1][1]), "v"(bb[1][2]), "v"(bb[1][3]), "v"(bb[1][4]), "v"(bb[1][5]), "v"(bb[1][6]), "v"(bb[1][7]));
    }
    float4 b4[4], s4[4];
    if constexpr (NAT && !PRE) {               // read-modify-write epilogue: bias and scale of this lane's 16 columns, likewise ahead of the pieces
        const int nbq = ecol0 + wn * 64 + 4 * fg;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b4[j] = epi.bias ? *reinterpret_cast<const float4*>(epi.bias + nbq + 16 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            s4[j] = epi.scale ? *reinterpret_cast<const float4*>(epi.scale + nbq + 16 * j) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            asm volatile("" ::"v"(b4[j].x), "v"(b4[j].y), "v"(b4[j].z), "v"(b4[j].w), "v"(s4[j].x), "v"(s4[j].y), "v"(s4[j].z), "v"(s4[j].w));
    }
    tile += gridDim.x;
    const bool has_next = PIPE && tile < nwg;
    if constexpr (PIPE) {
        if (has_next) {
            GEMM_SET_TILE(tile);
            GEMM_PROLOGUE();
        }
    }


    // epilogue.  D layout: col = lane & 15 -> output row m; MFMA row 4*fg + r of n-tile j -> output column 16*fg + 4*j + r
    if (PRE) {
        // the accumulators hold (x + bias) / alpha + a W^T: 32 plain stores
        const int nb = ecol0 + wn * 64 + 4 * fg;
        const float al = epi.alpha;
        if (erow0 + BM <= M) {
            float* const obase = reinterpret_cast<float*>(epi.out) + (int64_t)(erow0 + wm * (MI * 16) + fr) * epi.ldo + nb;
            const int64_t gstride = 16 * epi.ldo;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<float4*>(obase + i * gstride + 16 * j) =
                        make_float4(acc[i][j][0] * al, acc[i][j][1] * al, acc[i][j][2] * al, acc[i][j][3] * al);
        } else {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = erow0 + wm * (MI * 16) + i * 16 + fr;
                if (row >= M) continue;
                float* orow = reinterpret_cast<float*>(epi.out) + (int64_t)row * epi.ldo + nb;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<float4*>(orow + 16 * j) = make_float4(acc[i][j][0] * al, acc[i][j][1] * al, acc[i][j][2] * al, acc[i][j][3] * al);
            }
        }
    } else if (NAT) {
        // x[row][n] += scale[n] * (acc + bias[n]); lane (fr, fg) owns columns 16 j + 4 fg + 0..3 of n-tile j
        const int nb = ecol0 + wn * 64 + 4 * fg;
        // (b4 / s4 were fetched before the next tile's pieces went out, above)
#define RESID_RMW(X, I, PTR)                                                                                                        \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                             \
            float4 x = X[j];                                                                                                        \
            x.x += (acc[I][j][0] + b4[j].x) * s4[j].x; x.y += (acc[I][j][1] + b4[j].y) * s4[j].y;                                   \
            x.z += (acc[I][j][2] + b4[j].z) * s4[j].z; x.w += (acc[I][j][3] + b4[j].w) * s4[j].w;                                   \
            *reinterpret_cast<float4*>((PTR) + 16 * j) = x;                                                                         \
        }
        if (erow0 + BM <= M) {
            // Full tile: the read-modify-write of a 16-row group used to be 4 loads, wait, 4 stores -- and since vmcnt retires in order
            // and counts stores, the wait of group i + 1 also waited for the stores of group i: eight rounds of (store latency + load
            // latency), 38 k clocks of a proj tile's 85 k.  Now the loads of group i + 1 are issued BEFORE the stores of group i (two
            // groups of the residual tile in registers instead of one; same arithmetic, same bits), and a round waits for ONE load:
            //     L0 L1 | wait(4) S0 L2 | wait(8) S1 L3 | ... | wait(8) S6 | wait(4) S7
            // The memory operations and their waits are inline assembly: with loads AND stores pending the compiler treats vmcnt as
            // unordered and waits vmcnt(0) at every use (LLVM SIInsertWaitcnts: mixed pending events), which is the serial form again.
            // No compiler-issued memory operation may sit between them: bias / scale were consumed above, and the build fails if this
            // kernel has a private segment, i.e. spills (csrc/Makefile, spill guard).
            float* const obase = reinterpret_cast<float*>(epi.out) + (int64_t)(erow0 + wm * (MI * 16) + fr) * epi.ldo + nb;
            const int64_t gstride = 16 * epi.ldo;
            f32x4 xa[4], xb[4];
#define RMW_LOAD(X, PTR)                                                                                                            \
            do {                                                                                                                    \
                const float* _p = (PTR);                                                                                            \
                asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(X[0]) : "v"(_p) : "memory");                                 \
                asm volatile("global_load_dwordx4 %0, %1, off offset:64" : "=&v"(X[1]) : "v"(_p) : "memory");                       \
                asm volatile("global_load_dwordx4 %0, %1, off offset:128" : "=&v"(X[2]) : "v"(_p) : "memory");                      \
                asm volatile("global_load_dwordx4 %0, %1, off offset:192" : "=&v"(X[3]) : "v"(_p) : "memory");                      \
            } while (0)
#define RMW_WAIT(N, X) asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3])::"memory")
#define RMW_STORE(X, I, PTR)                                                                                                        \
            do {                                                                                                                    \
                float* _p = (PTR);                                                                                                  \
                f32x4 _v[4];                                                                                                        \
                _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                     \
                    _v[j][0] = X[j][0] + (acc[I][j][0] + b4[j].x) * s4[j].x; _v[j][1] = X[j][1] + (acc[I][j][1] + b4[j].y) * s4[j].y; \
                    _v[j][2] = X[j][2] + (acc[I][j][2] + b4[j].z) * s4[j].z; _v[j][3] = X[j][3] + (acc[I][j][3] + b4[j].w) * s4[j].w; \
                }                                                                                                                   \
                asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(_p), "v"(_v[0]) : "memory");                                  \
                asm volatile("global_store_dwordx4 %0, %1, off offset:64" ::"v"(_p), "v"(_v[1]) : "memory");                        \
                asm volatile("global_store_dwordx4 %0, %1, off offset:128" ::"v"(_p), "v"(_v[2]) : "memory");                       \
                asm volatile("global_store_dwordx4 %0, %1, off offset:192" ::"v"(_p), "v"(_v[3]) : "memory");                       \
            } while (0)
            static_assert(MI % 2 == 0, "read-modify-write epilogue: row groups in pairs");
            RMW_LOAD(xa, obase);
#pragma unroll
            for (int i = 0; i < MI; i += 2) {
                RMW_LOAD(xb, obase + (i + 1) * gstride);
                if (i == 0) RMW_WAIT(4, xa); else RMW_WAIT(8, xa);
                RMW_STORE(xa, i, obase + i * gstride);
                if (i + 2 < MI) {
                    RMW_LOAD(xa, obase + (i + 2) * gstride);
                    RMW_WAIT(8, xb);
                } else {
                    RMW_WAIT(4, xb);
                }
                RMW_STORE(xb, i + 1, obase + (i + 1) * gstride);
            }
#undef RMW_LOAD
#undef RMW_WAIT
#undef RMW_STORE
        } else {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = erow0 + wm * (MI * 16) + i * 16 + fr;
                if (row >= M) continue;
                float* orow = reinterpret_cast<float*>(epi.out) + (int64_t)row * epi.ldo + nb;
                float4 xr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xr[j] = *reinterpret_cast<const float4*>(orow + 16 * j);
                RESID_RMW(xr, i, orow)
            }
        }
#undef RESID_RMW
    } else if (PAIR) {
        const int nb = ecol0 + wn * 64 + 8 * fg;
#define PAIR_STORE(I, OROW)                                                                                                         \
        _Pragma("unroll") for (int j2 = 0; j2 < 2; ++j2) {                                                                          \
            float v[8];                                                                                                             \
            _Pragma("unroll") for (int t = 0; t < 8; t += 2) {                                                                      \
                f32x2 x = {acc[I][2 * j2 + (t >> 2)][t & 3], acc[I][2 * j2 + (t >> 2)][(t & 3) + 1]};                               \
                x += f32x2{bb[j2][t], bb[j2][t + 1]};                                                                               \
                if (GELU) x = QGELU ? quick_gelu2(x) : (TGELU ? tanh_gelu2(x) : gelu_erf2(x));                                      \
                v[t] = x.x; v[t + 1] = x.y;                                                                                         \
            }                                                                                                                       \
            const uint4 hi4 = make_uint4(f2h_pk(v[0], v[1]), f2h_pk(v[2], v[3]), f2h_pk(v[4], v[5]), f2h_pk(v[6], v[7]));           \
            *reinterpret_cast<uint4*>((OROW) + 32 * j2) = hi4;                                                                      \
            if (GT > 1) {                                                                                                           \
                const unsigned hw_[4] = {hi4.x, hi4.y, hi4.z, hi4.w};                                                               \
                unsigned lw_[4], sw_[4];                                                                                            \
                _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                                     \
                    const float h0 = h2f((u16)(hw_[t] & 0xFFFFu)), h1 = h2f((u16)(hw_[t] >> 16));                                   \
                    sw_[t] = f2h_pk(h0 * (1.0f / IBL_VIT_SPLIT_SCALE), h1 * (1.0f / IBL_VIT_SPLIT_SCALE));                          \
                    lw_[t] = f2h_pk((v[2 * t] - h0) * IBL_VIT_SPLIT_SCALE, (v[2 * t + 1] - h1) * IBL_VIT_SPLIT_SCALE);              \
                }                                                                                                                   \
                if (GT == 3) *reinterpret_cast<uint4*>((OROW) + N + 32 * j2) = make_uint4(lw_[0], lw_[1], lw_[2], lw_[3]);          \
                *reinterpret_cast<uint4*>((OROW) + (GT - 1) * (int64_t)N + 32 * j2) = make_uint4(sw_[0], sw_[1], sw_[2], sw_[3]);   \
            }                                                                                                                       \
        }
        if (erow0 + BM <= M) {                 // full tile (all but the last row of tiles): no per-row branch between the stores
            u16* const obase = reinterpret_cast<u16*>(epi.out) + (int64_t)(erow0 + wm * (MI * 16) + fr) * epi.ldo + nb;
            const int64_t gstride = 16 * epi.ldo;
#pragma unroll
            for (int i = 0; i < MI; ++i) { PAIR_STORE(i, obase + i * gstride) }
            stores_pending = true;
        } else {
            stores_pending = false;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int row = erow0 + wm * (MI * 16) + i * 16 + fr;
                if (row >= M) continue;
                u16* orow = reinterpret_cast<u16*>(epi.out) + (int64_t)row * epi.ldo + nb;
                PAIR_STORE(i, orow)
            }
        }
#undef PAIR_STORE
    } else {                                           // EPI_PATCH_F32, EPI_BIAS_F32
    const int n0 = ecol0 + wn * 64 + 16 * fg;          // first of this lane's 16 consecutive columns
    float bias[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (epi.bias) b4 = *reinterpret_cast<const float4*>(epi.bias + n0 + 4 * q);
        bias[4 * q] = b4.x; bias[4 * q + 1] = b4.y; bias[4 * q + 2] = b4.z; bias[4 * q + 3] = b4.w;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int row = erow0 + wm * (MI * 16) + i * 16 + fr;
        if (row >= M) continue;
        float v[16];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r] + bias[4 * j + r];
        if (EPI == EPI_PATCH_F32) {
            const int b = row / epi.patches_per_crop, p = row - b * epi.patches_per_crop;
            // the patch rows follow the crop's prefix rows (the CLS token; none with IBL_VIT_NO_CLS)
            const int64_t orow = (int64_t)b * epi.tokens_per_crop + epi.patch_row0 + p;
            float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(epi.out) + orow * epi.ldo + n0);
            if (epi.accumulate) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 xx = o[q];
                    xx.x = fmaf(v[4 * q], epi.alpha, xx.x); xx.y = fmaf(v[4 * q + 1], epi.alpha, xx.y);
                    xx.z = fmaf(v[4 * q + 2], epi.alpha, xx.z); xx.w = fmaf(v[4 * q + 3], epi.alpha, xx.w);
                    o[q] = xx;
                }
            } else {
                const float4* ps = reinterpret_cast<const float4*>(epi.pos + (int64_t)p * N + n0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 pp = ps[q];
                    o[q] = make_float4(v[4 * q] + pp.x, v[4 * q + 1] + pp.y, v[4 * q + 2] + pp.z, v[4 * q + 3] + pp.w);
                }
            }
        } else {
            float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(epi.out) + (int64_t)row * epi.ldo + n0);
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    }
    }
    GEMM_STAMP(3);                 // epilogue issued (its stores drain under the next tile's top wait)
#ifdef IBL_GEMM_STAMPS
    ++stamp_it;
#endif
    if (!has_next) break;
    first_tile = false;
    }
#undef GEMM_PROLOGUE
#undef GEMM_SLOT
#undef GEMM_PIECE
#undef FRAG_W
#undef FRAG_A
#undef GEMM_GLDS
#undef GEMM_SET_TILE
#endif
}

template <int EPI, bool T256>
static int launch_gemm_cfg(const u16* A, int64_t lda, const u16* W, int64_t ldw, int M, int N, int K, const GemmEpi& epi, hipStream_t s) {
    constexpr int BM = T256 ? 256 : 128, BN = BM;
    const int nwg = (N / BN) * ((M + BM - 1) / BM);
    const size_t lds = 2 * (size_t)(BM + BN) * GBK * 2;          // two stages (NS) of fp16 operand tiles
    // the dynamic-LDS limit is a per-device property of the function: set once per device of this process.  The bit mask is only
    // a cache -- two threads racing here both set the same value (localise_concurrent lanes launch from several host threads)
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    IBL_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        IBL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ibl_gemm_f16_tn<EPI, T256>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    int grid = nwg;
    if (T256) {                              // persistent: one workgroup per CU (a multiple of 8, see GEMM_SET_TILE)
        static std::atomic<int> n_cu{0};
        int cus = n_cu.load(std::memory_order_relaxed);
        if (cus == 0) {
            IBL_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            cus = cus >= 8 ? cus / 8 * 8 : 8;
            n_cu.store(cus, std::memory_order_relaxed);
        }
        if (grid > cus) grid = cus;
    }
    void* tok;
    ibl_prof_begin(IBL_PROF_GEMM, 2.0 * (double)M * (double)N * (double)(epi.algo_k < 0 ? 0 : (epi.algo_k ? epi.algo_k : K)), s, &tok);
    hipLaunchKernelGGL((ibl_gemm_f16_tn<EPI, T256>), dim3(grid), dim3(T256 ? 512 : 256), lds, s, A, lda, W, ldw, M, N, K, epi);
    ibl_prof_end(tok, s);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// EPI_RESID_PRE_F32 (residual tile preloaded into the accumulators, store-only epilogue) is a lab switch: measured per tile with
// tools/perf_gemm.py --stamps, the preload of the 256 KB tile at the tile top costs what the read-modify-write behind the K loop costs
// (30 k vs 38 - 12 k clocks: a CU sustains ~8.5 B / clock of L2-missing loads whatever their arrangement, and the count does not change
// with 32 instead of 256 active CUs), end to end proj 131 -> 138 us, fc2 298 -> 309 us.  IBL_GEMM_RESID_PRE=1 selects it where no scale
// vector is given.
static bool gemm_resid_pre() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("IBL_GEMM_RESID_PRE"); v = (e && atoi(e)) ? 1 : 0; }
    return v == 1;
}

template <int EPI>
static int launch_gemm(const u16* A, int64_t lda, const u16* W, int64_t ldw, int M, int N, int K, const GemmEpi& epi,
                       hipStream_t s) {
    if (M <= 0) return IBL_OK;
    if (N % 128 != 0 || K % GBK != 0)
        return ibl_set_error(IBL_ERR_ARG, "gemm: N (%d) must be a multiple of 128 and K (%d) of 64", N, K);
    // the 256 x 256 shape where it divides N and M is large, else 128 x 128
    if (N % 256 == 0 && M >= 4096) return launch_gemm_cfg<EPI, true>(A, lda, W, ldw, M, N, K, epi, s);
    return launch_gemm_cfg<EPI, false>(A, lda, W, ldw, M, N, K, epi, s);
}

// ------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row, fp32 in -> fp16 out (or fp32 out for the final CLS rows)
// ------------------------------------------------------------------------------------------------
// TERMS (fp16 output only): 1 = the row; 2 = [a_hi | a_hi / S]; 3 = [a_hi | a_lo * S | a_hi / S] (two-term operand rows, ibloc.h)
template <bool OUT_F32, int TERMS = 1>
__global__ __launch_bounds__(256) void ibl_layernorm_kernel(const float* x, int64_t in_row_stride,
                                                            int64_t n_rows, int dim, const float* __restrict__ g,
                                                            const float* __restrict__ b, float eps, void* out,
                                                            int64_t out_row_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const float* xr = x + row * in_row_stride;
    constexpr int MAXV = 4;                 // dim <= 1024
    float4 v[MAXV];
    const int nv = dim / 256;               // float4 per lane (dim % 256 == 0 handled; remainder below)
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv) {
            v[i] = *reinterpret_cast<const float4*>(xr + (i * 64 + lane) * 4);
            s += v[i].x + v[i].y + v[i].z + v[i].w;
        }
    const int rem0 = nv * 256;
    float tail[4] = {0.f, 0.f, 0.f, 0.f};     // up to 255 remaining elements, 4 per lane
    int ntail = 0;
    for (int i = rem0 + lane; i < dim; i += 64) { tail[ntail] = xr[i]; s += tail[ntail]; ++ntail; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv) {
            const float a = v[i].x - mean, c = v[i].y - mean, d = v[i].z - mean, e = v[i].w - mean;
            q += a * a + c * c + d * d + e * e;
        }
    for (int t = 0; t < ntail; ++t) { const float a = tail[t] - mean; q += a * a; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = rsqrtf(q / (float)dim + eps);
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv) {
            const int c0 = (i * 64 + lane) * 4;
            const float4 gg = *reinterpret_cast<const float4*>(g + c0);
            const float4 bb = *reinterpret_cast<const float4*>(b + c0);
            const float y0 = (v[i].x - mean) * rstd * gg.x + bb.x;
            const float y1 = (v[i].y - mean) * rstd * gg.y + bb.y;
            const float y2 = (v[i].z - mean) * rstd * gg.z + bb.z;
            const float y3 = (v[i].w - mean) * rstd * gg.w + bb.w;
            if (OUT_F32) {
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + row * out_row_stride + c0) =
                    make_float4(y0, y1, y2, y3);
            } else {
                ushort4 o;
                o.x = f2h(y0); o.y = f2h(y1); o.z = f2h(y2); o.w = f2h(y3);
                u16* orow = reinterpret_cast<u16*>(out) + row * out_row_stride;
                *reinterpret_cast<ushort4*>(orow + c0) = o;
                if (TERMS > 1) {
                    const float h0 = (float)__builtin_bit_cast(_Float16, o.x), h1 = (float)__builtin_bit_cast(_Float16, o.y);
                    const float h2 = (float)__builtin_bit_cast(_Float16, o.z), h3 = (float)__builtin_bit_cast(_Float16, o.w);
                    constexpr float S = IBL_VIT_SPLIT_SCALE, IS = 1.0f / IBL_VIT_SPLIT_SCALE;
                    ushort4 d;
                    d.x = f2h(h0 * IS); d.y = f2h(h1 * IS); d.z = f2h(h2 * IS); d.w = f2h(h3 * IS);
                    *reinterpret_cast<ushort4*>(orow + (TERMS - 1) * dim + c0) = d;
                    if (TERMS == 3) {
                        ushort4 l;
                        l.x = f2h((y0 - h0) * S); l.y = f2h((y1 - h1) * S); l.z = f2h((y2 - h2) * S); l.w = f2h((y3 - h3) * S);
                        *reinterpret_cast<ushort4*>(orow + dim + c0) = l;
                    }
                }
            }
        }
    int t = 0;
    for (int i = rem0 + lane; i < dim; i += 64, ++t) {
        const float y = (tail[t] - mean) * rstd * g[i] + b[i];
        if (OUT_F32) reinterpret_cast<float*>(out)[row * out_row_stride + i] = y;
        else {
            u16* orow = reinterpret_cast<u16*>(out) + row * out_row_stride;
            const u16 hb = f2h(y);
            orow[i] = hb;
            if (TERMS > 1) {
                const float hf = (float)__builtin_bit_cast(_Float16, hb);
                orow[(TERMS - 1) * dim + i] = f2h(hf * (1.0f / IBL_VIT_SPLIT_SCALE));
                if (TERMS == 3) orow[dim + i] = f2h((y - hf) * IBL_VIT_SPLIT_SCALE);
            }
        }
    }
}

// Every LayerNorm launch of this file: one wave per row, four rows per block.  terms 0 = fp32 rows (in place allowed), 1 / 2 / 3 = fp16
// rows of that many terms.  No argument checks here: ibl_vit_forward and ibl_layernorm_f32 validate what they pass.
static int launch_layernorm(const float* x, int64_t ld_x, int64_t n_rows, int dim, const float* g, const float* b, float eps, void* out,
                            int64_t ld_out, int terms, hipStream_t s) {
    const dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
    if (terms == 0) hipLaunchKernelGGL((ibl_layernorm_kernel<true>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else if (terms == 1) hipLaunchKernelGGL((ibl_layernorm_kernel<false, 1>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else if (terms == 2) hipLaunchKernelGGL((ibl_layernorm_kernel<false, 2>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else hipLaunchKernelGGL((ibl_layernorm_kernel<false, 3>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

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

// ------------------------------------------------------------------------------------------------
// Rotary position embedding (DINOv3), in place on q and k of the patch rows of qkv fp16 [B*T][3*D].  table fp32 [P][64] = [cos(32) | sin(32)].
// One lane owns the eight pairs (i, i + 32), i = 8c .. 8c + 7, of one (patch row, head) -- of q and of k, which share the table row -- so
// the in-place update has no cross-lane hazard: two 16-byte loads and two 16-byte stores per operand, four lanes cover a head's 128 bytes.
// Streaming: no LDS, no reuse but the table (P * 256 bytes, cache resident).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ibl_rope_kernel(u16* __restrict__ qkv, const float* __restrict__ table, unsigned n_items, int T,
                                                       int n_prefix, int D, int heads, int x0) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n_items) return;
    const unsigned c = idx & 3u, rh = idx >> 2;
    const unsigned r = rh / (unsigned)heads, h = rh - r * (unsigned)heads;       // r = b * P + p
    const unsigned P = (unsigned)(T - n_prefix);
    const unsigned b = r / P, p = r - b * P;
    const float4* tc = reinterpret_cast<const float4*>(table + (int64_t)p * 64 + 8 * c);
    const float4 c0 = tc[0], c1 = tc[1], s0 = tc[8], s1 = tc[9];
    const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    u16* row = qkv + ((int64_t)b * T + n_prefix + p) * (3 * (int64_t)D) + h * 64 + 8 * c;
    for (int x = x0; x < 2; ++x) {
        uint4* plo = reinterpret_cast<uint4*>(row + (int64_t)x * D);
        uint4* phi = reinterpret_cast<uint4*>(row + (int64_t)x * D + 32);
        const uint4 vlo = *plo, vhi = *phi;
        const unsigned lo[4] = {vlo.x, vlo.y, vlo.z, vlo.w}, hi[4] = {vhi.x, vhi.y, vhi.z, vhi.w};
        unsigned olo[4], ohi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float ra[2], rb[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float a = h2f((u16)(lo[j] >> (16 * e))), bb = h2f((u16)(hi[j] >> (16 * e)));
                const float cc = cs[2 * j + e], ss = sn[2 * j + e];
                ra[e] = fmaf(a, cc, -(bb * ss));       // x[i] cos - x[i + 32] sin
                rb[e] = fmaf(bb, cc, a * ss);          // x[i + 32] cos + x[i] sin
            }
            olo[j] = f2h_pk(ra[0], ra[1]);
            ohi[j] = f2h_pk(rb[0], rb[1]);
        }
        *plo = make_uint4(olo[0], olo[1], olo[2], olo[3]);
        *phi = make_uint4(ohi[0], ohi[1], ohi[2], ohi[3]);
    }
}

// no argument checks: ibl_rope_f16 and ibl_vit_forward validate what they pass.  P >= 1, batch >= 1
static int run_rope(u16* qkv, const float* table, int B, int T, int n_prefix, int D, int heads, int k_only, hipStream_t s) {
    const int64_t items = (int64_t)B * (T - n_prefix) * heads * 4;
    if (items > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "rope: batch * patches * heads * 4 exceeds the grid");
    hipLaunchKernelGGL(ibl_rope_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, qkv, table, (unsigned)items, T, n_prefix, D,
                       heads, k_only ? 1 : 0);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// ------------------------------------------------------------------------------------------------
// Attention: one workgroup (4 waves) per (crop, head); head_dim = 64; T <= 16 * NT.
// qkv fp16 [B*T][3*D] = [q | k | v], each [heads][64].   out fp16 [B*T][D].
// ------------------------------------------------------------------------------------------------
#ifndef ATT_THREADS
#define ATT_THREADS 512
#endif
// TERMS: the output as K-extended operand rows for the projection (row stride TERMS * D; round 4): 2 = [a | a / S] (projection weights
// in two terms), 3 = [a | (value - a) * S | a / S] (+ the attention output's own second term)
template <int NT, int TERMS = 1>
__global__ __launch_bounds__(ATT_THREADS, 2) void ibl_attention_kernel(const u16* __restrict__ qkv, u16* __restrict__ out, int T,
                                                            int D, int heads, float scale, int cls_only) {
    constexpr int KEYS = NT * 16;
    constexpr int KROW = 144;               // bytes per K row (64 fp16 + 16 B pad)
    constexpr int VROW = KEYS * 2 + 16;     // bytes per V^T row
    __shared__ __attribute__((aligned(16))) unsigned char sK[KEYS * KROW];
    __shared__ __attribute__((aligned(16))) unsigned char sV[64 * VROW];
#ifdef ATT_LAB_PAD_LDS       // lab: pad the LDS so that one workgroup fits a CU (is the kernel bound by its resident workgroups?)
    __shared__ int lab_pad[ATT_LAB_PAD_LDS / 4];
    if (threadIdx.x == 0 && T == -12345) lab_pad[D] = 1;
#endif

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int64_t tok0 = (int64_t)b * T;
    const int64_t ld = 3 * (int64_t)D;
    const u16* qbase = qkv + tok0 * ld + h * 64;
    const u16* kbase = qbase + D;
    const u16* vbase = qbase + 2 * D;

    // stage K rows (zero beyond T)
    for (int c = tid; c < KEYS * 8; c += ATT_THREADS) {
        const int key = c >> 3, c16 = c & 7;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (key < T) val = *reinterpret_cast<const uint4*>(kbase + (int64_t)key * ld + c16 * 8);
        *reinterpret_cast<uint4*>(sK + key * KROW + c16 * 16) = val;
    }
    // stage V transposed: task = (key pair, 8-wide d chunk); writes packed dwords V^T[d][key..key+1]
    for (int c = tid; c < (KEYS / 2) * 8; c += ATT_THREADS) {
        const int kp = c % (KEYS / 2), dch = c / (KEYS / 2);
        const int key = kp * 2;
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = make_uint4(0, 0, 0, 0);
        if (key < T) v0 = *reinterpret_cast<const uint4*>(vbase + (int64_t)key * ld + dch * 8);
        if (key + 1 < T) v1 = *reinterpret_cast<const uint4*>(vbase + (int64_t)(key + 1) * ld + dch * 8);
        const unsigned int a[4] = {v0.x, v0.y, v0.z, v0.w}, d[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned int lo = (a[i] & 0xFFFFu) | (d[i] << 16);            // element 2i of both keys
            const unsigned int hi = (a[i] >> 16) | (d[i] & 0xFFFF0000u);        // element 2i+1
            *reinterpret_cast<unsigned int*>(sV + (dch * 8 + 2 * i) * VROW + key * 2) = lo;
            *reinterpret_cast<unsigned int*>(sV + (dch * 8 + 2 * i + 1) * VROW + key * 2) = hi;
        }
    }
    __syncthreads();

    const int fr = lane & 15, fg = lane >> 4;
    const int nqt = cls_only ? 1 : (T + 15) / 16;        // cls_only: only token 0 of every crop is a query (last block of the ViT)
    for (int qt = wave; qt < nqt; qt += ATT_THREADS / 64) {
        // B operand = Q^T: lane (q = fr, g): Q[q0 + fr][32 ks + 8 g .. +7]
        int qrow = qt * 16 + fr;
        if (qrow >= T) qrow = T - 1;
        const u16* qp = qbase + (int64_t)qrow * ld + fg * 8;
        const h16x8 qf0 = *reinterpret_cast<const h16x8*>(qp);
        const h16x8 qf1 = *reinterpret_cast<const h16x8*>(qp + 32);

        // S^T tiles: acc[t][r] = S[q = fr][key = 16 t + 4 g + r]
        f32x4 sc[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const unsigned char* kp = sK + (t * 16 + fr) * KROW + fg * 16;
            const h16x8 k0 = *reinterpret_cast<const h16x8*>(kp);
            const h16x8 k1 = *reinterpret_cast<const h16x8*>(kp + 64);
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
            a = IBL_MFMA(k0, qf0, a, 0, 0, 0);
            a = IBL_MFMA(k1, qf1, a, 0, 0, 0);
            // raw scores: the softmax scale is folded into the exponent below (scale > 0: the maximum commutes); only a tile that
            // reaches past T needs the key mask (the softmax arithmetic, not the MFMAs, bounds this kernel: ~10 VALU per score before)
            if (t * 16 + 16 > T) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t * 16 + fg * 4 + r >= T) a[r] = -INFINITY;
            }
            mx = fmaxf(mx, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
            sc[t] = a;
            // keep the K fragments of later tiles from being hoisted up here: unrolled, the 34 ds_read_b128 of a query tile were
            // all issued first (398 VGPRs -> one block per CU); with two blocks per CU the other block hides this latency
            asm volatile("" ::: "memory");
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
        const float c2 = scale * 1.4426950408889634f, mc = -mx * c2;       // exp(scale (s - mx)) = exp2(s c2 - mx c2)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(sc[t][r], c2, mc));
                sc[t][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);

        // O = P V : A operand (P) element j of lane (q = fr, g) for k-step s is key
        //   32 s + 4 g + j (j < 4, tile 2s)   or   32 s + 16 + 4 g + (j - 4) (tile 2s + 1);
        // B operand (V) uses the same key permutation, read from V^T rows.
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        constexpr int NS = (NT + 1) / 2;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            h16x8 pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pf[j] = (_Float16)sc[2 * s][j];
                pf[4 + j] = (2 * s + 1 < NT) ? (_Float16)sc[(2 * s + 1 < NT) ? 2 * s + 1 : 0][j] : (_Float16)0.0f;
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const unsigned char* vp = sV + (dt * 16 + fr) * VROW + (32 * s + 4 * fg) * 2;
                const uint2 lo = *reinterpret_cast<const uint2*>(vp);
                uint2 hi = make_uint2(0, 0);
                if (2 * s + 1 < NT) hi = *reinterpret_cast<const uint2*>(vp + 32);
                uint4 packed = make_uint4(lo.x, lo.y, hi.x, hi.y);
                const h16x8 vf = *reinterpret_cast<const h16x8*>(&packed);
                o[dt] = IBL_MFMA(vf, pf, o[dt], 0, 0, 0);     // O^T tile: rows = d, columns = q
            }
            asm volatile("" ::: "memory");
        }
        // O^T layout: row = d = 16 dt + 4 g + r, col = q = fr -> a lane owns four consecutive head dimensions of ONE query row
        // (8-byte stores; the untransposed product left it with single fp16 elements of four rows) and that row's softmax
        // sum is already on this lane (it was reduced over the lane groups above).
        const int qg = qt * 16 + fr;
        if (qg < (cls_only ? 1 : T)) {
            const float inv = 1.0f / sum;
            u16* orow = out + (tok0 + qg) * (int64_t)(TERMS * D) + h * 64 + 4 * fg;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                float v[4];
                unsigned short h4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { v[r] = o[dt][r] * inv; h4[r] = f2h(v[r]); }
                uint2 pk;
                pk.x = (unsigned)h4[0] | ((unsigned)h4[1] << 16);
                pk.y = (unsigned)h4[2] | ((unsigned)h4[3] << 16);
                *reinterpret_cast<uint2*>(orow + dt * 16) = pk;
                if (TERMS > 1) {
                    unsigned short l4[4], s4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float hf = h2f(h4[r]);
                        s4[r] = f2h(hf * (1.0f / IBL_VIT_SPLIT_SCALE));
                        l4[r] = f2h((v[r] - hf) * IBL_VIT_SPLIT_SCALE);
                    }
                    if (TERMS == 3)
                        *reinterpret_cast<uint2*>(orow + D + dt * 16) = make_uint2((unsigned)l4[0] | ((unsigned)l4[1] << 16), (unsigned)l4[2] | ((unsigned)l4[3] << 16));
                    *reinterpret_cast<uint2*>(orow + (TERMS - 1) * D + dt * 16) =
                        make_uint2((unsigned)s4[0] | ((unsigned)s4[1] << 16), (unsigned)s4[2] | ((unsigned)s4[3] << 16));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Streaming attention (T beyond the resident kernel's 272): one workgroup (4 waves) per (block of 64 queries, crop * head); a wave
// owns one tile of 16 queries and walks ALL keys in chunks of 128 that pass through LDS (K rows padded to 144 B, V^T rows to 272 B: the
// resident kernel's layouts, one chunk wide).  fp32 online softmax: running maximum m, running sum l of the unrounded p (kept as the
// lane's partial over its own keys and reduced once at the end), O rescaled by exp2((m_old - m_new) c2) at every chunk -- no deferred
// rescale.  p is rounded to fp16 only as the MFMA operand of P V; 1 / l is applied once in fp32 and the TERMS blocks derive from the
// one fp16 rounding as in the resident kernel.  No atomics, the key order of every reduction is fixed: a crop's result does not
// depend on its batch, and cls_only (query tile 0 alone, walked by wave 0 exactly as in the full run) is bit-identical to row 0 of the
// full run.  The next chunk's global loads are issued before the compute on the current one and written to LDS after the barrier.
// ------------------------------------------------------------------------------------------------
#define ATT_S_THREADS 256
#define ATT_S_KV 128         // keys per chunk
#define ATT_S_QB 64          // queries per workgroup (16 per wave)
template <int TERMS>
__global__ __launch_bounds__(ATT_S_THREADS, 3) void ibl_attention_stream_kernel(const u16* __restrict__ qkv, u16* __restrict__ out, int T,
                                                                                  int D, int heads, float scale, int cls_only) {
    constexpr int KV = ATT_S_KV, NT = KV / 16, NS = NT / 2;
    constexpr int KROW = 144;               // bytes per K row (64 fp16 + 16 B pad)
    constexpr int VROW = KV * 2 + 16;       // bytes per V^T row
    constexpr int KL = KV * 8 / ATT_S_THREADS;          // uint4 of K per thread and chunk
    constexpr int VL = (KV / 2) * 8 / ATT_S_THREADS;    // (key pair, 8-wide d chunk) tasks of V per thread and chunk
    __shared__ __attribute__((aligned(16))) unsigned char sK[KV * KROW];
    __shared__ __attribute__((aligned(16))) unsigned char sV[64 * VROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = cls_only ? 1 : T;                    // rows that are queries
    const int nqb = (nq + ATT_S_QB - 1) / ATT_S_QB;     // the query blocks of a (crop, head) are neighbours in the grid: they share K and V in L2
    const int bh = blockIdx.x / nqb, qb = blockIdx.x % nqb;
    const int b = bh / heads, h = bh % heads;
    const int64_t tok0 = (int64_t)b * T;
    const int64_t ld = 3 * (int64_t)D;
    const u16* qbase = qkv + tok0 * ld + h * 64;
    const u16* kbase = qbase + D;
    const u16* vbase = qbase + 2 * D;

    const int fr = lane & 15, fg = lane >> 4;
    const int qt = qb * (ATT_S_QB / 16) + wave;
    const bool active = qt * 16 < nq;                   // wave-uniform; an idle wave still stages and meets the barriers
    int qrow = qt * 16 + fr;
    if (qrow >= T) qrow = T - 1;
    const u16* qp = qbase + (int64_t)qrow * ld + fg * 8;
    const h16x8 qf0 = *reinterpret_cast<const h16x8*>(qp);
    const h16x8 qf1 = *reinterpret_cast<const h16x8*>(qp + 32);

    uint4 kreg[KL], vreg[VL][2];
    // a chunk's rows from global memory into registers (zero at and beyond T: a masked key has p = 0, its V must not be NaN bytes)
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            const int c = tid + i * ATT_S_THREADS, key = k0 + (c >> 3), c16 = c & 7;
            kreg[i] = make_uint4(0, 0, 0, 0);
            if (key < T) kreg[i] = *reinterpret_cast<const uint4*>(kbase + (int64_t)key * ld + c16 * 8);
        }
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int c = tid + i * ATT_S_THREADS, key = k0 + (c % (KV / 2)) * 2, dch = c / (KV / 2);
            vreg[i][0] = make_uint4(0, 0, 0, 0);
            vreg[i][1] = make_uint4(0, 0, 0, 0);
            if (key < T) vreg[i][0] = *reinterpret_cast<const uint4*>(vbase + (int64_t)key * ld + dch * 8);
            if (key + 1 < T) vreg[i][1] = *reinterpret_cast<const uint4*>(vbase + (int64_t)(key + 1) * ld + dch * 8);
        }
    };
    // registers -> LDS: K rows as they are, V transposed as packed dwords V^T[d][key .. key + 1]
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < KL; ++i) {
            const int c = tid + i * ATT_S_THREADS;
            *reinterpret_cast<uint4*>(sK + (c >> 3) * KROW + (c & 7) * 16) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VL; ++i) {
            const int c = tid + i * ATT_S_THREADS, key = (c % (KV / 2)) * 2, dch = c / (KV / 2);
            const unsigned int a[4] = {vreg[i][0].x, vreg[i][0].y, vreg[i][0].z, vreg[i][0].w};
            const unsigned int d[4] = {vreg[i][1].x, vreg[i][1].y, vreg[i][1].z, vreg[i][1].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                *reinterpret_cast<unsigned int*>(sV + (dch * 8 + 2 * j) * VROW + key * 2) = (a[j] & 0xFFFFu) | (d[j] << 16);
                *reinterpret_cast<unsigned int*>(sV + (dch * 8 + 2 * j + 1) * VROW + key * 2) = (a[j] >> 16) | (d[j] & 0xFFFF0000u);
            }
        }
    };

    const float c2 = scale * 1.4426950408889634f;       // exp(scale (s - m)) = exp2(s c2 - m c2)
    float m = -INFINITY, l = 0.f;                       // l: this lane's share (keys 16 t + 4 fg + r of every chunk) of the row sum
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    store_chunk();
    __syncthreads();
    for (int k0 = 0; k0 < T; k0 += KV) {
        const bool more = k0 + KV < T;
        if (more) load_chunk(k0 + KV);
        if (active) {
            // S^T tiles of the chunk: sc[t][r] = S[q = fr][key = k0 + 16 t + 4 fg + r]
            f32x4 sc[NT];
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const unsigned char* kp = sK + (t * 16 + fr) * KROW + fg * 16;
                const h16x8 kf0 = *reinterpret_cast<const h16x8*>(kp);
                const h16x8 kf1 = *reinterpret_cast<const h16x8*>(kp + 64);
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
                a = IBL_MFMA(kf0, qf0, a, 0, 0, 0);
                a = IBL_MFMA(kf1, qf1, a, 0, 0, 0);
                if (k0 + t * 16 + 16 > T) {             // only the last chunk's tiles that reach past T
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + t * 16 + fg * 4 + r >= T) a[r] = -INFINITY;
                }
                mx = fmaxf(mx, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
                sc[t] = a;
                asm volatile("" ::: "memory");          // keep the K fragments of later tiles from all being read first
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // every chunk holds a key below T (the first one key 0), so mn is finite from the first chunk on; m = -inf gives alpha = 0
            const float mn = fmaxf(m, mx);
            const float alpha = __builtin_amdgcn_exp2f((m - mn) * c2);
            const float mc = -mn * c2;
            m = mn;
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(sc[t][r], c2, mc));
                    sc[t][r] = p;
                    sum += p;
                }
            l = fmaf(l, alpha, sum);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;      // the lane's 16 values all belong to query fr
            // O += P V with the resident kernel's key permutation: A element j of lane (fr, g), k-step s, is key 32 s + 4 g + j
            // (j < 4, tile 2 s) or 32 s + 16 + 4 g + (j - 4) (tile 2 s + 1); V^T rows are read with the same permutation
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                h16x8 pf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pf[j] = (_Float16)sc[2 * s][j];
                    pf[4 + j] = (_Float16)sc[2 * s + 1][j];
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const unsigned char* vp = sV + (dt * 16 + fr) * VROW + (32 * s + 4 * fg) * 2;
                    const uint2 lo = *reinterpret_cast<const uint2*>(vp);
                    const uint2 hi = *reinterpret_cast<const uint2*>(vp + 32);
                    uint4 packed = make_uint4(lo.x, lo.y, hi.x, hi.y);
                    const h16x8 vf = *reinterpret_cast<const h16x8*>(&packed);
                    o[dt] = IBL_MFMA(vf, pf, o[dt], 0, 0, 0);       // O^T tile: rows = d, columns = q
                }
                asm volatile("" ::: "memory");
            }
        }
        if (more) {
            __syncthreads();        // every wave has read the current chunk
            store_chunk();
            __syncthreads();
        }
    }

    const int qg = qt * 16 + fr;
    l += __shfl_xor(l, 16, 64);     // the four lane groups of a query, in a fixed order
    l += __shfl_xor(l, 32, 64);
    if (active && qg < nq) {
        const float inv = 1.0f / l;
        u16* orow = out + (tok0 + qg) * (int64_t)(TERMS * D) + h * 64 + 4 * fg;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            float v[4];
            unsigned short h4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = o[dt][r] * inv; h4[r] = f2h(v[r]); }
            uint2 pk;
            pk.x = (unsigned)h4[0] | ((unsigned)h4[1] << 16);
            pk.y = (unsigned)h4[2] | ((unsigned)h4[3] << 16);
            *reinterpret_cast<uint2*>(orow + dt * 16) = pk;
            if (TERMS > 1) {
                unsigned short l4[4], s4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hf = h2f(h4[r]);
                    s4[r] = f2h(hf * (1.0f / IBL_VIT_SPLIT_SCALE));
                    l4[r] = f2h((v[r] - hf) * IBL_VIT_SPLIT_SCALE);
                }
                if (TERMS == 3)
                    *reinterpret_cast<uint2*>(orow + D + dt * 16) = make_uint2((unsigned)l4[0] | ((unsigned)l4[1] << 16), (unsigned)l4[2] | ((unsigned)l4[3] << 16));
                *reinterpret_cast<uint2*>(orow + (TERMS - 1) * D + dt * 16) =
                    make_uint2((unsigned)s4[0] | ((unsigned)s4[1] << 16), (unsigned)s4[2] | ((unsigned)s4[3] << 16));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static inline int64_t rows_pad(int64_t r) { return ibl_align_up(r, 128); }

static_assert(IBL_LINEAR_F16 == EPI_BIAS_H16 && IBL_LINEAR_GELU_F16 == EPI_BIAS_GELU_H16 && IBL_LINEAR_RESID_F32 == EPI_RESID_F32 &&
                  IBL_LINEAR_PATCH_F32 == EPI_PATCH_F32 && IBL_LINEAR_F32 == EPI_BIAS_F32 && IBL_LINEAR_RESID_PRE_F32 == EPI_RESID_PRE_F32 &&
                  IBL_LINEAR_GELU_F16_X2 == EPI_BIAS_GELU_H16KX2 && IBL_LINEAR_GELU_F16_X3 == EPI_BIAS_GELU_H16KX3,
              "the header's epilogue numbers are the kernel's");
static_assert(sizeof(ibl_linear_desc) == 112, "activation fills the tail padding of ibl_linear_desc: its size is part of the ABI");

// a finite, normal, positive power of two: the factor EPI_RESID_PRE_F32 divides by and multiplies with must do both exactly
static bool pow2_positive(float a) {
    int e;
    return a >= 1.17549435e-38f && a <= 3.0e38f && frexpf(a, &e) == 0.5f;
}

// ibl_linear_f16_ex and ibl_linear_f16_act: one validation, one launch.  `act` is the activation the GELU epilogues apply (d->activation is
// not read here), `act_max` the largest one the entry takes, `fn` the entry's name for the messages.
static int linear_f16_run(const ibl_linear_desc* d, int act, int act_max, void* stream, const char* fn);

extern "C" int ibl_linear_f16_ex(const ibl_linear_desc* d, void* stream) {
    if (!d) return ibl_set_error(IBL_ERR_ARG, "ibl_linear_f16_ex: null descriptor");
    if (d->rows == 0) return IBL_OK;
    // 0 and 1 only, as before IBL_ACT_GELU_TANH existed: the tanh form comes through ibl_linear_f16_act
    return linear_f16_run(d, d->activation, IBL_ACT_QUICK_GELU, stream, "ibl_linear_f16_ex");
}

extern "C" int ibl_linear_f16_act(const ibl_linear_desc* d, int activation, void* stream) {
    if (!d) return ibl_set_error(IBL_ERR_ARG, "ibl_linear_f16_act: null descriptor");
    if (d->activation != 0)
        return ibl_set_error(IBL_ERR_ARG, "ibl_linear_f16_act: the descriptor's activation field (%d) must be 0: the activation is the argument", d->activation);
    if (activation < IBL_ACT_GELU_ERF || activation > IBL_ACT_GELU_TANH)
        return ibl_set_error(IBL_ERR_ARG, "ibl_linear_f16_act: unknown activation %d (0, 1 or 2)", activation);
    if (d->rows == 0) return IBL_OK;
    return linear_f16_run(d, activation, IBL_ACT_GELU_TANH, stream, "ibl_linear_f16_act");
}

static int linear_f16_run(const ibl_linear_desc* d, int act, int act_max, void* stream, const char* fn) {
    if (!d->x || !d->W || !d->out) return ibl_set_error(IBL_ERR_ARG, "%s: null operand", fn);
    if (d->rows < 0 || d->rows > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "%s: rows out of range", fn);
    const int n_out = d->n_out, n_in = d->n_in, epi = d->epilogue;
    if (n_out <= 0 || n_in <= 0 || n_out % 128 != 0 || n_in % GBK != 0)
        return ibl_set_error(IBL_ERR_ARG, "%s: n_out (%d) must be a positive multiple of 128 and n_in (%d) of 64", fn, n_out, n_in);
    if (epi < EPI_BIAS_H16 || epi > EPI_BIAS_GELU_H16KX3) return ibl_set_error(IBL_ERR_ARG, "%s: unknown epilogue %d", fn, epi);
    const bool gelu = epi == EPI_BIAS_GELU_H16 || epi == EPI_BIAS_GELU_H16KX2 || epi == EPI_BIAS_GELU_H16KX3;
    if (act != IBL_ACT_GELU_ERF && !(gelu && act > 0 && act <= act_max))
        return ibl_set_error(IBL_ERR_ARG, "%s: activation %d with epilogue %d (0, or a known one with a GELU epilogue)", fn, act, epi);
    const int terms = epi == EPI_BIAS_GELU_H16KX3 ? 3 : (epi == EPI_BIAS_GELU_H16KX2 ? 2 : 1);
    if ((d->ldx & 7) || (d->ldw & 7) || (d->ldo & 7) || d->ldx < n_in || d->ldw < n_in || d->ldo < (int64_t)terms * n_out)
        return ibl_set_error(IBL_ERR_ARG, "%s: row strides must be >= the row length (%d in, %d out) and multiples of 8 elements", fn,
                             n_in, terms * n_out);
    GemmEpi e{};
    e.bias = d->bias;
    e.out = d->out;
    e.ldo = d->ldo;
    if (epi == EPI_RESID_F32) e.scale = d->scale;
    if (epi == EPI_RESID_PRE_F32 || (epi == EPI_PATCH_F32 && d->accumulate)) {
        if (!pow2_positive(d->alpha)) return ibl_set_error(IBL_ERR_ARG, "%s: alpha (%g) must be a positive power of two", fn, (double)d->alpha);
        e.alpha = d->alpha;
    }
    if (epi == EPI_PATCH_F32) {
        if (d->patches_per_crop <= 0 || d->tokens_per_crop <= d->patches_per_crop || d->rows % d->patches_per_crop != 0)
            return ibl_set_error(IBL_ERR_ARG, "%s: patch scatter needs 0 < patches_per_crop (%d) < tokens_per_crop (%d) and whole crops (%lld rows)", fn,
                                 d->patches_per_crop, d->tokens_per_crop, (long long)d->rows);
        if (d->accumulate != 0 && d->accumulate != 1) return ibl_set_error(IBL_ERR_ARG, "%s: accumulate must be 0 or 1", fn);
        if (!d->accumulate && !d->pos) return ibl_set_error(IBL_ERR_ARG, "%s: null position rows without accumulate", fn);
        e.pos = d->pos;
        e.tokens_per_crop = d->tokens_per_crop;
        e.patches_per_crop = d->patches_per_crop;
        e.patch_row0 = 1;                  // this entry's contract: row b * tokens_per_crop + 1 + p, also where tokens_per_crop > patches_per_crop + 1
        e.accumulate = d->accumulate;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const u16* a = reinterpret_cast<const u16*>(d->x);
    const u16* w = reinterpret_cast<const u16*>(d->W);
    const int rows = (int)d->rows;
    switch (epi) {
        case EPI_BIAS_H16: return launch_gemm<EPI_BIAS_H16>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_BIAS_GELU_H16:
            return act == IBL_ACT_QUICK_GELU  ? launch_gemm<EPI_BIAS_QGELU_H16>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                   : act == IBL_ACT_GELU_TANH ? launch_gemm<EPI_BIAS_TGELU_H16>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                                              : launch_gemm<EPI_BIAS_GELU_H16>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_RESID_F32: return launch_gemm<EPI_RESID_F32>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_PATCH_F32: return launch_gemm<EPI_PATCH_F32>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_BIAS_F32: return launch_gemm<EPI_BIAS_F32>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_RESID_PRE_F32: return launch_gemm<EPI_RESID_PRE_F32>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        case EPI_BIAS_GELU_H16KX2:
            return act == IBL_ACT_QUICK_GELU  ? launch_gemm<EPI_BIAS_QGELU_H16KX2>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                   : act == IBL_ACT_GELU_TANH ? launch_gemm<EPI_BIAS_TGELU_H16KX2>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                                              : launch_gemm<EPI_BIAS_GELU_H16KX2>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
        default:
            return act == IBL_ACT_QUICK_GELU  ? launch_gemm<EPI_BIAS_QGELU_H16KX3>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                   : act == IBL_ACT_GELU_TANH ? launch_gemm<EPI_BIAS_TGELU_H16KX3>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s)
                                              : launch_gemm<EPI_BIAS_GELU_H16KX3>(a, d->ldx, w, d->ldw, rows, n_out, n_in, e, s);
    }
}

extern "C" int ibl_linear_f16(const void* x, int64_t ldx, const void* W, int64_t ldw, const float* bias, const float* scale,
                               int64_t rows, int n_out, int n_in, int epilogue, void* out, int64_t ldo, void* stream) {
    if (epilogue != EPI_BIAS_H16 && epilogue != EPI_BIAS_GELU_H16 && epilogue != EPI_RESID_F32 && epilogue != EPI_BIAS_F32 && rows != 0)
        return ibl_set_error(IBL_ERR_ARG, "ibl_linear_f16: unknown epilogue %d", epilogue);
    ibl_linear_desc d{};
    d.x = x; d.ldx = ldx; d.W = W; d.ldw = ldw; d.bias = bias; d.scale = scale; d.out = out; d.ldo = ldo;
    d.rows = rows; d.n_out = n_out; d.n_in = n_in; d.epilogue = epilogue;
    d.alpha = 1.0f;
    // the lab switch of the encoder ($IBL_GEMM_RESID_PRE, see gemm_resid_pre) keeps working through this entry; ibl_linear_f16_ex never reads it
    if (epilogue == EPI_RESID_F32 && !scale && gemm_resid_pre()) d.epilogue = EPI_RESID_PRE_F32;
    return ibl_linear_f16_ex(&d, stream);
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

// any 1 <= T <= IBL_ATT_STREAM_MAX_TOKENS; the caller has checked that the grid fits
static int run_attention_stream(const u16* qkv, u16* out, int B, int T, int D, int heads, int cls_only, hipStream_t s, int terms) {
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nqb = ((cls_only ? 1 : T) + ATT_S_QB - 1) / ATT_S_QB;
    const int64_t wgs = (int64_t)B * heads * nqb;
    if (wgs > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "attention: batch * heads * query blocks exceeds the grid");
    dim3 grid((unsigned)wgs), block(ATT_S_THREADS);
    if (terms == 3) hipLaunchKernelGGL((ibl_attention_stream_kernel<3>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);
    else if (terms == 2) hipLaunchKernelGGL((ibl_attention_stream_kernel<2>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);
    else hipLaunchKernelGGL((ibl_attention_stream_kernel<1>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

static int run_attention(const u16* qkv, u16* out, int B, int T, int D, int heads, int cls_only, hipStream_t s, int terms = 1) {
    if (T > 272) {      // beyond the resident kernel's widest tier: keys and values stream through LDS
        if (T > IBL_ATT_STREAM_MAX_TOKENS)
            return ibl_set_error(IBL_ERR_UNSUPPORTED, "attention: n_tokens %d > %d not supported", T, IBL_ATT_STREAM_MAX_TOKENS);
        return run_attention_stream(qkv, out, B, T, D, heads, cls_only, s, terms);
    }
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nt = (T + 15) / 16;
    dim3 grid(B * heads), block(ATT_THREADS);
#define IBL_ATT(NTV)                                                                                      \
    do {                                                                                                  \
        if (terms == 3) hipLaunchKernelGGL((ibl_attention_kernel<NTV, 3>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);        \
        else if (terms == 2) hipLaunchKernelGGL((ibl_attention_kernel<NTV, 2>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);   \
        else hipLaunchKernelGGL((ibl_attention_kernel<NTV, 1>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);                    \
    } while (0)
    if (getenv("IBL_DEBUG_OCC")) {
        int nb = -1;
        hipFuncAttributes fa{};
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, ibl_attention_kernel<17, 1>, ATT_THREADS, 0);
        (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&ibl_attention_kernel<17, 1>));
        fprintf(stderr, "[occ] attention<17>: %d blocks/CU, %d regs, %zu B static LDS\n", nb, fa.numRegs, fa.sharedSizeBytes);
    }
    if (nt <= 4) IBL_ATT(4);
    else if (nt <= 9) IBL_ATT(9);
    else if (nt <= 13) IBL_ATT(13);
    else if (nt <= 17) IBL_ATT(17);
    else return ibl_set_error(IBL_ERR_UNSUPPORTED, "attention: n_tokens %d > 272 not supported", T);
#undef IBL_ATT
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

extern "C" int ibl_attention_f16(const void* qkv, void* out, int batch, int n_tokens, int dim, int heads, int cls_only, int terms,
                                 void* stream) {
    if (batch < 0 || n_tokens < 0) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: negative batch (%d) or n_tokens (%d)", batch, n_tokens);
    if (terms < 1 || terms > 3) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: terms %d outside 1..3", terms);
    if (cls_only != 0 && cls_only != 1) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: cls_only must be 0 or 1");
    if (heads <= 0 || dim != heads * 64)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_attention_f16: dim (%d) must be 64 * heads (%d): head_dim is 64", dim, heads);
    if (n_tokens > 272) return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_attention_f16: n_tokens %d > 272 not supported", n_tokens);
    if ((int64_t)batch * heads > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: batch * heads exceeds the grid");
    if (batch == 0 || n_tokens == 0) return IBL_OK;
    if (!qkv || !out) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: null pointer");
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return ibl_set_error(IBL_ERR_ARG, "ibl_attention_f16: qkv must be 16-byte and out 8-byte aligned");
    return run_attention(reinterpret_cast<const u16*>(qkv), reinterpret_cast<u16*>(out), batch, n_tokens, dim, heads, cls_only,
                         reinterpret_cast<hipStream_t>(stream), terms);
}

extern "C" int ibl_rope_f16(void* qkv, const float* table, int batch, int n_tokens, int n_prefix, int dim, int heads, int k_only,
                            void* stream) {
    if (batch < 0 || n_tokens < 0) return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: negative batch (%d) or n_tokens (%d)", batch, n_tokens);
    if (n_prefix < 0 || n_prefix > n_tokens)
        return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: n_prefix %d outside 0..n_tokens (%d)", n_prefix, n_tokens);
    if (k_only != 0 && k_only != 1) return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: k_only must be 0 or 1");
    if (heads <= 0 || dim != heads * 64)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_rope_f16: dim (%d) must be 64 * heads (%d): head_dim is 64", dim, heads);
    if ((int64_t)batch * n_tokens > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: batch * n_tokens out of range");
    if (batch == 0 || n_prefix == n_tokens) return IBL_OK;
    if (!qkv || !table) return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: null pointer");
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(table) & 15))
        return ibl_set_error(IBL_ERR_ARG, "ibl_rope_f16: qkv and table must be 16-byte aligned");
    return run_rope(reinterpret_cast<u16*>(qkv), table, batch, n_tokens, n_prefix, dim, heads, k_only, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int ibl_attention_stream_f16(const void* qkv, void* out, int batch, int n_tokens, int dim, int heads, int cls_only, int terms,
                                        void* stream) {
    if (batch < 0 || n_tokens < 0)
        return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: negative batch (%d) or n_tokens (%d)", batch, n_tokens);
    if (terms < 1 || terms > 3) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: terms %d outside 1..3", terms);
    if (cls_only != 0 && cls_only != 1) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: cls_only must be 0 or 1");
    if (heads <= 0 || dim != heads * 64)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_attention_stream_f16: dim (%d) must be 64 * heads (%d): head_dim is 64", dim, heads);
    if (n_tokens > IBL_ATT_STREAM_MAX_TOKENS)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_attention_stream_f16: n_tokens %d > %d not supported", n_tokens, IBL_ATT_STREAM_MAX_TOKENS);
    if ((int64_t)batch * heads * ((n_tokens + ATT_S_QB - 1) / ATT_S_QB) > 0x7fffffff)
        return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: batch * heads * query blocks exceeds the grid");
    if (batch == 0 || n_tokens == 0) return IBL_OK;
    if (!qkv || !out) return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: null pointer");
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return ibl_set_error(IBL_ERR_ARG, "ibl_attention_stream_f16: qkv must be 16-byte and out 8-byte aligned");
    return run_attention_stream(reinterpret_cast<const u16*>(qkv), reinterpret_cast<u16*>(out), batch, n_tokens, dim, heads, cls_only,
                                reinterpret_cast<hipStream_t>(stream), terms);
}

extern "C" int ibl_layernorm_f32(const float* x, int64_t ld_x, int64_t n_rows, int dim, const float* gamma, const float* beta, float eps,
                                 void* out, int64_t ld_out, int out_kind, void* stream) {
    if (n_rows < 0 || n_rows > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: n_rows out of range");
    if (out_kind < IBL_LN_OUT_F32 || out_kind > IBL_LN_OUT_F16_X3) return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: unknown out_kind %d", out_kind);
    // the kernel keeps a row in 4 float4 per lane (+ a tail of up to 255 elements): beyond 1024 columns would be dropped, not refused
    if (dim <= 0 || dim > 1024 || (dim & 3))
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "ibl_layernorm_f32: dim %d must be a multiple of 4 in 4..1024", dim);
    if (!(eps >= 0.f)) return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: eps must be >= 0");
    const int terms = out_kind == IBL_LN_OUT_F32 ? 1 : out_kind;          // column blocks of an output row
    if (ld_x < dim || ld_out < (int64_t)terms * dim || (ld_x & 3) || (ld_out & 3))
        return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: row strides must be >= the row length (%d in, %d out) and multiples of 4 elements",
                             dim, terms * dim);
    if (n_rows == 0) return IBL_OK;
    if (!x || !gamma || !beta || !out) return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(gamma) & 15) || (reinterpret_cast<uintptr_t>(beta) & 15) ||
        (reinterpret_cast<uintptr_t>(out) & (out_kind == IBL_LN_OUT_F32 ? 15 : 7)))
        return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: x / gamma / beta / fp32 out must be 16-byte aligned, fp16 out 8-byte");
    if (out == (const void*)x && (out_kind != IBL_LN_OUT_F32 || ld_out != ld_x))
        return ibl_set_error(IBL_ERR_ARG, "ibl_layernorm_f32: in place needs fp32 output with the input's row stride");
    return launch_layernorm(x, ld_x, n_rows, dim, gamma, beta, eps, out, ld_out, out_kind, reinterpret_cast<hipStream_t>(stream));
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
    hipStream_t s = (hipStream_t)stream;
    const int64_t Rn = (int64_t)batch * T, R = rows_pad(Rn);

    int64_t offs[IBL_VIT_WS_COUNT];
    const int64_t end = vit_layout(d, batch, offs);
    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    if ((base - reinterpret_cast<unsigned char*>(workspace)) + end > workspace_bytes)
        return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: workspace too small");
    float* x = reinterpret_cast<float*>(base + offs[IBL_VIT_WS_X]);
    u16* xn = reinterpret_cast<u16*>(base + offs[IBL_VIT_WS_XN]);
    u16* qkv = reinterpret_cast<u16*>(base + offs[IBL_VIT_WS_QKV]);
    const int at = (d->flags & IBL_VIT_ACT_TERMS3) ? 3 : ((d->flags & IBL_VIT_ACT_TERMS2) ? 2 : 1);
    u16* att = reinterpret_cast<u16*>(base + offs[IBL_VIT_WS_ATT]);
    u16* hid = reinterpret_cast<u16*>(base + offs[IBL_VIT_WS_HID]);
    u16* fin_bf = reinterpret_cast<u16*>(base + offs[IBL_VIT_WS_FIN]);

    int st;
    // patch embedding (conv as GEMM over im2col'ed patches) + position embedding, scattered into x
    {
        GemmEpi e{};
        e.bias = w->b_patch; e.pos = w->pos_patch; e.out = x; e.ldo = D; e.tokens_per_crop = T; e.patches_per_crop = P;
        e.patch_row0 = n_prefix;           // the patch rows follow the crop's prefix rows: class token and registers
        st = launch_gemm<EPI_PATCH_F32>(reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                                        reinterpret_cast<const u16*>(w->w_patch), d->patch_k_pad, batch * P, D,
                                        d->patch_k_pad, e, s);
        if (st) return st;
        if (w->w_patch_lo) {             // second term of the patch weights: x += (patches W_lo'^T) / S
            GemmEpi e2 = e;
            e2.bias = nullptr; e2.accumulate = 1; e2.alpha = 1.0f / IBL_VIT_SPLIT_SCALE; e2.algo_k = -1;
            st = launch_gemm<EPI_PATCH_F32>(reinterpret_cast<const u16*>(patches), d->patch_k_pad,
                                            reinterpret_cast<const u16*>(w->w_patch_lo), d->patch_k_pad, batch * P, D,
                                            d->patch_k_pad, e2, s);
            if (st) return st;
        }
        if (!no_cls) {
            const int64_t n = (int64_t)batch * n_prefix * D;
            hipLaunchKernelGGL(ibl_set_prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, w->cls_pos, w->reg_tokens, batch,
                               T, n_prefix, D);
            IBL_LAUNCH_CHECK();
        }
    }
    if (d->flags & IBL_VIT_PRE_LN) {
        // CLIP ln_pre: normalise the residual stream in place (through the fp16-free f32 path)
        st = launch_layernorm(x, D, Rn, D, w->ln_pre_g, w->ln_pre_b, d->ln_eps, x, D, 0, s);
        if (st) return st;
    }
    for (int l = 0; l < d->n_blocks_run; ++l) {
        const ibl_vit_layer* L = &w->layers[l];
        // Only the CLS row leaves the encoder (unless all tokens are asked for), so in the LAST block the other rows are dead
        // after they have served as keys / values: its query projection, attention, output projection and MLP run on the CLS
        // rows alone (M = batch instead of batch * T; every row of a GEMM is computed independently, so the CLS rows come out
        // bit-identical).  The kernels take row strides, the CLS rows are addressed in place (stride T * D).
        const bool cls_only = (l == d->n_blocks_run - 1) && !(d->flags & IBL_VIT_OUT_ALL_TOKENS);
        const int64_t TD = (int64_t)T * D;
        // two-term operands (ibloc.h): only in blocks that run on every row (the CLS-only last block stays plain)
        const int qt = (!cls_only && L->w_qkv_x && L->qkv_terms > 1) ? L->qkv_terms : 1;
        const int ft = (!cls_only && L->w_fc1_x && L->fc1_terms > 1) ? L->fc1_terms : 1;
        if (qt > 3 || ft > 3) return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: layer %d: at most three operand terms", l);
        st = launch_layernorm(x, D, Rn, D, L->ln1_g, L->ln1_b, d->ln_eps, xn, (int64_t)qt * D, qt, s);
        if (st) return st;
        if (!cls_only) {
            GemmEpi e{};
            e.bias = L->b_qkv; e.out = qkv; e.ldo = 3 * D; e.algo_k = D;
            st = launch_gemm<EPI_BIAS_H16>(xn, (int64_t)qt * D, reinterpret_cast<const u16*>(qt > 1 ? L->w_qkv_x : L->w_qkv), (int64_t)qt * D, (int)Rn,
                                           3 * D, qt * D, e, s);
            if (st) return st;
        } else {
            GemmEpi e{};                                  // keys and values of every token: weight rows D .. 3D
            e.bias = L->b_qkv + D; e.out = qkv + D; e.ldo = 3 * D;
            st = launch_gemm<EPI_BIAS_H16>(xn, D, reinterpret_cast<const u16*>(L->w_qkv) + (int64_t)D * D, D, (int)Rn, 2 * D, D, e, s);
            if (st) return st;
            GemmEpi q{};                                  // queries of the CLS rows only
            q.bias = L->b_qkv; q.out = qkv; q.ldo = 3 * TD;
            st = launch_gemm<EPI_BIAS_H16>(xn, TD, reinterpret_cast<const u16*>(L->w_qkv), D, batch, D, D, q, s);
            if (st) return st;
        }
        // K-extended inputs of the two residual GEMMs (w_o_x / w_fc2_x; round 4): ONE launch of K' = terms * K instead of one
        // read-modify-write pass over the residual per term
        const int ot = (!cls_only && L->w_o_x && L->o_terms > 1) ? L->o_terms : 1;
        const int f2t = (!cls_only && L->w_fc2_x && L->fc2_terms > 1) ? L->fc2_terms : 1;
        if (ot > at || f2t > at || ot > 3 || f2t > 3)
            return ibl_set_error(IBL_ERR_ARG, "ibl_vit_forward: layer %d: o_terms / fc2_terms %d / %d need IBL_VIT_ACT_TERMS%d in the descriptor", l, ot, f2t, ot > f2t ? ot : f2t);
        if (w->rope_table) {      // DINOv3: q and k of the patch rows rotated in place; the class-rows-only block has no patch-row q to rotate
            st = run_rope(qkv, w->rope_table, batch, T, n_prefix, D, H, cls_only ? 1 : 0, s);
            if (st) return st;
        }
        st = run_attention(qkv, att, batch, T, D, H, cls_only ? 1 : 0, s, ot);
        if (st) return st;
        {
            GemmEpi e{};
            e.bias = L->b_o; e.scale = L->ls1; e.out = x; e.ldo = cls_only ? TD : D; e.alpha = 1.0f; e.algo_k = D;
            const u16* wo = reinterpret_cast<const u16*>(ot > 1 ? L->w_o_x : L->w_o);
            const int64_t lda = cls_only ? TD : (int64_t)ot * D;
            // no LayerScale vector (none in the model, or folded into W_o / b_o by the host): the residual tile is preloaded into the
            // accumulators (EPI_RESID_PRE_F32, lab); with one, the read-modify-write epilogue applies it
            st = (L->ls1 || !gemm_resid_pre()) ? launch_gemm<EPI_RESID_F32>(att, lda, wo, (int64_t)ot * D, cls_only ? batch : (int)Rn, D, ot * D, e, s)
                        : launch_gemm<EPI_RESID_PRE_F32>(att, lda, wo, (int64_t)ot * D, cls_only ? batch : (int)Rn, D, ot * D, e, s);
            if (st) return st;
            if (!cls_only && ot == 1 && L->w_o_lo) {         // (older form) second weight term as its own launch: x += (ls1 / S) * (att W_lo'^T)
                e.bias = nullptr; e.scale = L->ls1_lo; e.algo_k = -1; e.alpha = 1.0f / IBL_VIT_SPLIT_SCALE;
                st = L->ls1_lo ? launch_gemm<EPI_RESID_F32>(att, D, reinterpret_cast<const u16*>(L->w_o_lo), D, (int)Rn, D, D, e, s)
                               : launch_gemm<EPI_RESID_PRE_F32>(att, D, reinterpret_cast<const u16*>(L->w_o_lo), D, (int)Rn, D, D, e, s);
                if (st) return st;
            }
        }
        st = cls_only ? launch_layernorm(x, TD, batch, D, L->ln2_g, L->ln2_b, d->ln_eps, fin_bf, D, 1, s)
                      : launch_layernorm(x, D, Rn, D, L->ln2_g, L->ln2_b, d->ln_eps, xn, (int64_t)ft * D, ft, s);
        if (st) return st;
        const u16* mlp_in = cls_only ? fin_bf : xn;
        const int mlp_rows = cls_only ? batch : (int)Rn;
        {
            GemmEpi e{};
            e.bias = L->b_fc1; e.out = hid; e.ldo = (int64_t)f2t * d->mlp_dim; e.algo_k = D;
            const u16* w1 = reinterpret_cast<const u16*>(ft > 1 ? L->w_fc1_x : L->w_fc1);
            if (d->flags & IBL_VIT_QUICK_GELU) {
                if (f2t == 3) st = launch_gemm<EPI_BIAS_QGELU_H16KX3>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
                else if (f2t == 2) st = launch_gemm<EPI_BIAS_QGELU_H16KX2>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
                else st = launch_gemm<EPI_BIAS_QGELU_H16>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
            } else if (d->flags & IBL_VIT_TANH_GELU) {
                if (f2t == 3) st = launch_gemm<EPI_BIAS_TGELU_H16KX3>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
                else if (f2t == 2) st = launch_gemm<EPI_BIAS_TGELU_H16KX2>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
                else st = launch_gemm<EPI_BIAS_TGELU_H16>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
            } else if (f2t == 3) st = launch_gemm<EPI_BIAS_GELU_H16KX3>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
            else if (f2t == 2) st = launch_gemm<EPI_BIAS_GELU_H16KX2>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
            else st = launch_gemm<EPI_BIAS_GELU_H16>(mlp_in, (int64_t)ft * D, w1, (int64_t)ft * D, mlp_rows, d->mlp_dim, ft * D, e, s);
            if (st) return st;
        }
        {
            GemmEpi e{};
            e.bias = L->b_fc2; e.scale = L->ls2; e.out = x; e.ldo = cls_only ? TD : D; e.alpha = 1.0f; e.algo_k = d->mlp_dim;
            const u16* w2 = reinterpret_cast<const u16*>(f2t > 1 ? L->w_fc2_x : L->w_fc2);
            const int64_t k2 = (int64_t)f2t * d->mlp_dim;
            st = (L->ls2 || !gemm_resid_pre()) ? launch_gemm<EPI_RESID_F32>(hid, k2, w2, k2, mlp_rows, D, (int)k2, e, s)
                        : launch_gemm<EPI_RESID_PRE_F32>(hid, k2, w2, k2, mlp_rows, D, (int)k2, e, s);
            if (st) return st;
            if (!cls_only && f2t == 1 && L->w_fc2_lo) {
                e.bias = nullptr; e.scale = L->ls2_lo; e.algo_k = -1; e.alpha = 1.0f / IBL_VIT_SPLIT_SCALE;
                st = L->ls2_lo ? launch_gemm<EPI_RESID_F32>(hid, d->mlp_dim, reinterpret_cast<const u16*>(L->w_fc2_lo), d->mlp_dim, mlp_rows, D, d->mlp_dim, e, s)
                               : launch_gemm<EPI_RESID_PRE_F32>(hid, d->mlp_dim, reinterpret_cast<const u16*>(L->w_fc2_lo), d->mlp_dim, mlp_rows, D, d->mlp_dim, e, s);
                if (st) return st;
            }
        }
    }
    if (d->flags & IBL_VIT_OUT_ALL_TOKENS) {
        // DATOR streams: all tokens, optionally through the final LayerNorm
        if (d->flags & IBL_VIT_FINAL_LN) {
            st = launch_layernorm(x, D, Rn, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, s);
            if (st) return st;
        } else {
            IBL_HIP_CHECK(hipMemcpyAsync(out, x, Rn * D * 4, hipMemcpyDeviceToDevice, s));
        }
        return IBL_OK;
    }
    // CLS rows -> (final LN) -> (projection) -> out fp32 [batch][out_dim]
    if (d->flags & IBL_VIT_PROJ) {
        if (!(d->flags & IBL_VIT_FINAL_LN)) return ibl_set_error(IBL_ERR_UNSUPPORTED, "projection needs final LN");
        GemmEpi e{};
        e.bias = nullptr; e.out = out; e.ldo = d->out_dim;
        if (w->w_proj_x) {           // three-term operands: K' = 3 D, one accumulation (xn is free by now: batch <= R rows of 3 D)
            st = launch_layernorm(x, (int64_t)T * D, batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, xn, (int64_t)3 * D, 3, s);
            if (st) return st;
            e.algo_k = D;
            return launch_gemm<EPI_BIAS_F32>(xn, (int64_t)3 * D, reinterpret_cast<const u16*>(w->w_proj_x), (int64_t)3 * D, batch, d->out_dim,
                                             3 * D, e, s);
        }
        st = launch_layernorm(x, (int64_t)T * D, batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, fin_bf, D, 1, s);
        if (st) return st;
        return launch_gemm<EPI_BIAS_F32>(fin_bf, D, reinterpret_cast<const u16*>(w->w_proj), D, batch, d->out_dim, D, e, s);
    }
    if (d->flags & IBL_VIT_FINAL_LN) {
        st = launch_layernorm(x, (int64_t)T * D, batch, D, w->ln_f_g, w->ln_f_b, d->ln_eps, out, D, 0, s);
        if (st) return st;
    } else {
        IBL_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)D * 4, x, (size_t)T * D * 4, (size_t)D * 4, batch,
                                       hipMemcpyDeviceToDevice, s));
    }
    return IBL_OK;
}
