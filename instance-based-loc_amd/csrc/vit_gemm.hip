// vit_gemm.hip -- the ViT encoder's fp16 GEMM on gfx950 (vit.hip says where it sits in the forward): the kernel ibl_gemm_f16_tn with its
// fused epilogues and three GELU forms, the tile choice, gemm_launch (the one run-time -> compile-time dispatch) and the entries
// ibl_linear_f16, ibl_linear_f16_ex and ibl_linear_f16_act.
#include <atomic>

#include "vit_kernels.h"

// ------------------------------------------------------------------------------------------------
// GEMM  C[M][N] = A[M][K] * W[N][K]^T  (+ epilogue)
// ------------------------------------------------------------------------------------------------
// EPI: the header's eight IBL_LINEAR_* numbers (static_assert below)
enum { EPI_BIAS_H16 = 0, EPI_BIAS_GELU_H16 = 1, EPI_RESID_F32 = 2, EPI_PATCH_F32 = 3, EPI_BIAS_F32 = 4,
       // x += alpha * (a W^T + bias), alpha a power of two, with the residual tile PRELOADED into the accumulators: the MFMA chain starts
       // from (x + bias) / alpha and the epilogue is 32 plain stores per lane -- no read-modify-write after the K loop (round 4)
       EPI_RESID_PRE_F32 = 5,
       // EPI_BIAS_GELU_H16 writing K-extended operand rows for the next GEMM (round 4; ldo = terms * N):
       //   KX2: [h | h / S]  (fc2 weights in two terms)     KX3: [h | (value - h) * S | h / S]  (+ the hidden layer's second term)
       EPI_BIAS_GELU_H16KX2 = 6, EPI_BIAS_GELU_H16KX3 = 7 };
// ACT, the kernel's second template argument: the header's IBL_ACT_* numbers, read by epilogues 1, 6 and 7 only (no other epilogue is
// instantiated with a non-zero ACT).  IBL_ACT_QUICK_GELU (reached through ibl_linear_desc.activation and IBL_VIT_QUICK_GELU): QuickGELU,
// v * sigmoid(1.702 v), in place of the erf form -- everything after the activation is the same code.  IBL_ACT_GELU_TANH (ibl_linear_f16_act
// and IBL_VIT_TANH_GELU): likewise the tanh form of GELU (SigLIP)

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

template <int EPI, int ACT, bool T256>
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
    constexpr bool QGELU = ACT == IBL_ACT_QUICK_GELU, TGELU = ACT == IBL_ACT_GELU_TANH;
    constexpr int GT = EPI == EPI_BIAS_GELU_H16KX3 ? 3 : (EPI == EPI_BIAS_GELU_H16KX2 ? 2 : 1);     // column blocks the fp16 epilogue writes
    constexpr bool GELU = EPI == EPI_BIAS_GELU_H16 || GT > 1;
    static_assert(GELU || ACT == IBL_ACT_GELU_ERF, "an activation with an epilogue that applies none");
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

template <int EPI, int ACT, bool T256>
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
        IBL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ibl_gemm_f16_tn<EPI, ACT, T256>),
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
    hipLaunchKernelGGL((ibl_gemm_f16_tn<EPI, ACT, T256>), dim3(grid), dim3(T256 ? 512 : 256), lds, s, A, lda, W, ldw, M, N, K, epi);
    ibl_prof_end(tok, s);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// EPI_RESID_PRE_F32 (residual tile preloaded into the accumulators, store-only epilogue) is a lab switch: measured per tile with
// tools/perf_gemm.py --stamps, the preload of the 256 KB tile at the tile top costs what the read-modify-write behind the K loop costs
// (30 k vs 38 - 12 k clocks: a CU sustains ~8.5 B / clock of L2-missing loads whatever their arrangement, and the count does not change
// with 32 instead of 256 active CUs), end to end proj 131 -> 138 us, fc2 298 -> 309 us.  IBL_GEMM_RESID_PRE=1 selects it where no scale
// vector is given.
bool gemm_resid_pre() {
    static int v = -1;
    if (v < 0) { const char* e = getenv("IBL_GEMM_RESID_PRE"); v = (e && atoi(e)) ? 1 : 0; }
    return v == 1;
}

template <int EPI, int ACT>
static int launch_gemm(const u16* A, int64_t lda, const u16* W, int64_t ldw, int M, int N, int K, const GemmEpi& epi,
                       hipStream_t s) {
    if (M <= 0) return IBL_OK;
    if (N % 128 != 0 || K % GBK != 0)
        return ibl_set_error(IBL_ERR_ARG, "gemm: N (%d) must be a multiple of 128 and K (%d) of 64", N, K);
    // the 256 x 256 shape where it divides N and M is large, else 128 x 128
    if (N % 256 == 0 && M >= 4096) return launch_gemm_cfg<EPI, ACT, true>(A, lda, W, ldw, M, N, K, epi, s);
    return launch_gemm_cfg<EPI, ACT, false>(A, lda, W, ldw, M, N, K, epi, s);
}

// Run-time (epilogue, activation) -> instantiation: the only place that names one.  The 14 rows below, each in both tiles, are the 28
// kernels of the library: the eight epilogues, and the quick and tanh forms of the three that apply a GELU.  Any other pair is refused.
int gemm_launch(int epi, int act, const u16* A, int64_t lda, const u16* W, int64_t ldw, int M, int N, int K, const GemmEpi& e, hipStream_t s) {
    if (epi < EPI_BIAS_H16 || epi > EPI_BIAS_GELU_H16KX3) return ibl_set_error(IBL_ERR_ARG, "%s: unknown epilogue %d", "gemm", epi);
    switch (act * 8 + epi) {
#define GEMM_ROW(EPI, ACT) \
    case (ACT) * 8 + (EPI): return launch_gemm<EPI, ACT>(A, lda, W, ldw, M, N, K, e, s)
        GEMM_ROW(EPI_BIAS_H16, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_BIAS_GELU_H16, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_RESID_F32, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_PATCH_F32, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_BIAS_F32, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_RESID_PRE_F32, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_BIAS_GELU_H16KX2, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_BIAS_GELU_H16KX3, IBL_ACT_GELU_ERF);
        GEMM_ROW(EPI_BIAS_GELU_H16, IBL_ACT_QUICK_GELU);
        GEMM_ROW(EPI_BIAS_GELU_H16KX2, IBL_ACT_QUICK_GELU);
        GEMM_ROW(EPI_BIAS_GELU_H16KX3, IBL_ACT_QUICK_GELU);
        GEMM_ROW(EPI_BIAS_GELU_H16, IBL_ACT_GELU_TANH);
        GEMM_ROW(EPI_BIAS_GELU_H16KX2, IBL_ACT_GELU_TANH);
        GEMM_ROW(EPI_BIAS_GELU_H16KX3, IBL_ACT_GELU_TANH);
#undef GEMM_ROW
    }
    return ibl_set_error(IBL_ERR_ARG, "%s: activation %d with epilogue %d (0, or a known one with a GELU epilogue)", "gemm", act, epi);
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
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
    return gemm_launch(epi, act, reinterpret_cast<const u16*>(d->x), d->ldx, reinterpret_cast<const u16*>(d->W), d->ldw, (int)d->rows, n_out, n_in,
                       e, reinterpret_cast<hipStream_t>(stream));
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
