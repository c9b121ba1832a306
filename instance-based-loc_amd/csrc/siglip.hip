// siglip.hip -- SigLIP attention-pooling head (transformers' SiglipMultiheadAttentionPoolingHead) on gfx950, fp32 throughout.
//
// The trunk (vit.hip with IBL_VIT_NO_CLS | IBL_VIT_TANH_GELU | IBL_VIT_OUT_ALL_TOKENS | IBL_VIT_FINAL_LN) hands over fp32 tokens
// [B][T][D].  One learned probe attends over them (nn.MultiheadAttention with a single, constant query), then x + MLP(LayerNorm(x)).
// With a constant query the key and value projections over all B * T tokens fold away (include/ibloc.h): per head one vector u_h, a
// softmax over the tokens and one weighted token sum, then dim x head_dim values per crop.  The head is 0.03 % of the trunk's FLOPs and
// the last arithmetic before the output, so nothing in it is rounded to fp16.
//
// Kernels: ibl_probe_pool_kernel (scores, softmax, weighted sum: one workgroup per crop), a 64 x 64 LDS-tiled fp32 linear with the
// epilogues the head needs (a k-ordered fmaf chain per output, so a row does not depend on the batch it runs in), LayerNorm (one wave
// per row).
#include <hip/hip_runtime.h>

#include <atomic>

#include "ibl_common.h"
#include "ibloc.h"

#define PP_THREADS 512        // 8 waves per crop
#define PP_MAXH 16            // heads (accumulators a lane keeps)
#define PP_MAXD 1024          // dim: one float4 column group per thread of the weighted sum, at most PP_THREADS / 2 of them
#define PP_MAXSPLIT 4         // token interleave of the weighted sum
#define PP_LDS_MAX (160 * 1024)

// token interleave of the weighted sum: as many groups of dim / 4 threads as the workgroup holds, at most PP_MAXSPLIT (a function of dim
// alone: the summation order of a crop never depends on the batch or on the token count)
__host__ __device__ static inline int pp_split(int dim) {
    const int s = PP_THREADS / (dim / 4);
    return s > PP_MAXSPLIT ? PP_MAXSPLIT : s;
}

// LDS floats: [heads][dim] (u, later the partial sums of groups 1 .. S - 1) + [heads][n_tokens] (scores, then probabilities)
static inline int64_t pp_lds_bytes(int n_tokens, int dim, int heads) {
    const int s = pp_split(dim);
    const int64_t a = (int64_t)(s > 2 ? s - 1 : 1) * heads * dim;
    return (a + ((int64_t)heads * n_tokens + 3) / 4 * 4) * 4;
}

// x [B][T][D], u [H][D] -> probs [B][H][T] (optional), pooled [B][H][D].  One workgroup per crop.
//   1. scores: a wave per token (two at a time), lanes own float4 column groups, H accumulators per lane, xor butterfly 32 .. 1
//   2. softmax: a wave per head over the scores in LDS (max, exp, sum in the same lane-strided order, butterfly), IEEE division
//   3. weighted sum: thread (g, j) owns columns 4 j .. 4 j + 3 and the tokens g, g + S, ...; groups 1 .. S - 1 hand their partial sums to
//      group 0 through LDS (the u region, dead by then), which adds them in the order 1, 2, ... and stores
__global__ __launch_bounds__(PP_THREADS) void ibl_probe_pool_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                    float* __restrict__ pooled, float* __restrict__ probs, int T, int D,
                                                                    int H) {
    extern __shared__ __attribute__((aligned(16))) float pp_smem[];
    const int S = pp_split(D);
    const int D4 = D >> 2;
    float* const su = pp_smem;
    float* const sp = pp_smem + (int64_t)(S > 2 ? S - 1 : 1) * H * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = PP_THREADS / 64;
    const int64_t b = blockIdx.x;
    const float4* const xb = reinterpret_cast<const float4*>(x + b * T * D);

    for (int e = tid; e < H * D4; e += PP_THREADS) reinterpret_cast<float4*>(su)[e] = reinterpret_cast<const float4*>(u)[e];
    __syncthreads();

    // ---- 1. scores (two tokens of a wave at a time: their loads fly together and share the reads of u; a token's own order is unchanged)
    for (int t = wave; t < T; t += 2 * NW) {
        const int t2 = t + NW;
        const bool two = t2 < T;
        float acc[PP_MAXH], acc2[PP_MAXH];
#pragma unroll
        for (int h = 0; h < PP_MAXH; ++h) acc[h] = acc2[h] = 0.f;
        for (int j = lane; j < D4; j += 64) {
            const float4 xv = xb[(int64_t)t * D4 + j];
            const float4 yv = two ? xb[(int64_t)t2 * D4 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int h = 0; h < PP_MAXH; ++h)
                if (h < H) {
                    const float4 uv = reinterpret_cast<const float4*>(su)[h * D4 + j];
                    acc[h] = fmaf(xv.x, uv.x, acc[h]);
                    acc[h] = fmaf(xv.y, uv.y, acc[h]);
                    acc[h] = fmaf(xv.z, uv.z, acc[h]);
                    acc[h] = fmaf(xv.w, uv.w, acc[h]);
                    acc2[h] = fmaf(yv.x, uv.x, acc2[h]);
                    acc2[h] = fmaf(yv.y, uv.y, acc2[h]);
                    acc2[h] = fmaf(yv.z, uv.z, acc2[h]);
                    acc2[h] = fmaf(yv.w, uv.w, acc2[h]);
                }
        }
#pragma unroll
        for (int h = 0; h < PP_MAXH; ++h)
            if (h < H) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    acc[h] += __shfl_xor(acc[h], off, 64);
                    acc2[h] += __shfl_xor(acc2[h], off, 64);
                }
                if (lane == 0) {
                    sp[h * T + t] = acc[h];
                    if (two) sp[h * T + t2] = acc2[h];
                }
            }
    }
    __syncthreads();

    // ---- 2. softmax over the tokens, per head
    for (int h = wave; h < H; h += NW) {
        float* const row = sp + h * T;
        float m = -INFINITY;
        for (int t = lane; t < T; t += 64) m = fmaxf(m, row[t]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float sum = 0.f;
        for (int t = lane; t < T; t += 64) {
            const float e = expf(row[t] - m);
            row[t] = e;
            sum += e;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        for (int t = lane; t < T; t += 64) {
            const float p = row[t] / sum;
            row[t] = p;
            if (probs) probs[(b * H + h) * T + t] = p;
        }
    }
    __syncthreads();

    // ---- 3. pooled[h] = sum_t p[h][t] x[t]
    const int g = tid / D4, j = tid - g * D4;
    float4 acc[PP_MAXH];
#pragma unroll
    for (int h = 0; h < PP_MAXH; ++h) acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g < S) {
#pragma unroll 8
        for (int t = g; t < T; t += S) {      // eight loads in flight; an accumulator's order over t is unchanged
            const float4 xv = xb[(int64_t)t * D4 + j];
#pragma unroll
            for (int h = 0; h < PP_MAXH; ++h)
                if (h < H) {
                    const float p = sp[h * T + t];
                    acc[h].x = fmaf(p, xv.x, acc[h].x);
                    acc[h].y = fmaf(p, xv.y, acc[h].y);
                    acc[h].z = fmaf(p, xv.z, acc[h].z);
                    acc[h].w = fmaf(p, xv.w, acc[h].w);
                }
        }
        if (g > 0) {
#pragma unroll
            for (int h = 0; h < PP_MAXH; ++h)
                if (h < H) reinterpret_cast<float4*>(su)[((int64_t)(g - 1) * H + h) * D4 + j] = acc[h];
        }
    }
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int h = 0; h < PP_MAXH; ++h)
            if (h < H) {
                float4 a = acc[h];
                for (int gg = 1; gg < S; ++gg) {
                    const float4 q = reinterpret_cast<const float4*>(su)[((int64_t)(gg - 1) * H + h) * D4 + j];
                    a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
                }
                reinterpret_cast<float4*>(pooled)[(b * H + h) * D4 + j] = a;
            }
    }
}

static int probe_pool_check(const char* fn, int batch, int n_tokens, int dim, int heads) {
    if (batch < 1 || n_tokens < 1) return ibl_set_error(IBL_ERR_ARG, "%s: batch (%d) and n_tokens (%d) must be positive", fn, batch, n_tokens);
    if (heads < 1 || dim < 4 || (dim & 3) || dim % heads != 0)
        return ibl_set_error(IBL_ERR_ARG, "%s: dim (%d) must be a positive multiple of 4 and of heads (%d)", fn, dim, heads);
    if (heads > PP_MAXH || dim > PP_MAXD)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: heads (%d) > %d or dim (%d) > %d not supported", fn, heads, PP_MAXH, dim, PP_MAXD);
    if (pp_lds_bytes(n_tokens, dim, heads) > PP_LDS_MAX)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: heads * (dim + n_tokens) floats (%d, %d, %d) exceed the LDS of a workgroup", fn, heads, dim, n_tokens);
    return IBL_OK;
}

static int launch_probe_pool(const float* x, int batch, int n_tokens, int dim, int heads, const float* u, float* pooled, float* probs,
                             hipStream_t s) {
    // the dynamic-LDS limit is a per-device property of the function: set once per device of this process (see launch_gemm_cfg, vit_gemm.hip)
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    IBL_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        IBL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ibl_probe_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          PP_LDS_MAX));
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(ibl_probe_pool_kernel, dim3((unsigned)batch), dim3(PP_THREADS), (size_t)pp_lds_bytes(n_tokens, dim, heads), s, x, u,
                       pooled, probs, n_tokens, dim, heads);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

extern "C" int ibl_probe_pool_f32(const float* x, int batch, int n_tokens, int dim, int heads, const float* u, float* pooled, float* probs,
                                  void* stream) {
    if (!x || !u || !pooled) return ibl_set_error(IBL_ERR_ARG, "ibl_probe_pool_f32: null pointer");
    const int st = probe_pool_check("ibl_probe_pool_f32", batch, n_tokens, dim, heads);
    if (st) return st;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(u) & 15) || (reinterpret_cast<uintptr_t>(pooled) & 15) ||
        (reinterpret_cast<uintptr_t>(probs) & 3))
        return ibl_set_error(IBL_ERR_ARG, "ibl_probe_pool_f32: x, u and pooled must be 16-byte aligned");
    return launch_probe_pool(x, batch, n_tokens, dim, heads, u, pooled, probs, reinterpret_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------------------------------------
// out[z][r][n] = epi(b[z][n] + sum_k x[z][r][k] * W[z][n][k]), k ascending, one fmaf chain per output: 64 x 64 output tile, 4 x 4 outputs per
// thread (the tiling of dator.hip's linear), 32-deep K chunks through LDS, fetched as float4 one chunk ahead so that the global loads of
// chunk i + 1 fly under the arithmetic of chunk i (at batch <= 224 a linear of the head is 48 .. 192 workgroups: latency, not bandwidth,
// sets its time).  K, ldx and ldw are multiples of 4 and the rows 16-byte aligned.  blockIdx.z walks independent problems whose operands
// lie zx / zw / zb / zo elements apart (the per-head value projections).  epi: 0 none, 1 tanh GELU, 2 out = resid + (.)
// ------------------------------------------------------------------------------------------------
enum { PL_NONE = 0, PL_TANH_GELU = 1, PL_RESID = 2 };
#define PL_KC 32

__global__ __launch_bounds__(256) void ibl_probe_linear_kernel(const float* __restrict__ x, int64_t ldx, int64_t zx, const float* __restrict__ W,
                                                               int64_t ldw, int64_t zw, const float* __restrict__ bias, int64_t zb,
                                                               const float* __restrict__ resid, int64_t ldr, float* __restrict__ out,
                                                               int64_t ldo, int64_t zo, int R, int K, int N, int epi) {
    __shared__ float sx[PL_KC][65], sw[PL_KC][65];
    const int z = blockIdx.z;
    x += z * zx; W += z * zw; bias += z * zb; out += z * zo;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    // this thread's two float4 of a chunk: tile row (threadIdx.x >> 3) + 32 s, columns 4 (threadIdx.x & 7) .. + 3
    const int lrow = threadIdx.x >> 3, lk = (threadIdx.x & 7) * 4;
    float4 px[2], pw[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int r = r0 + lrow + 32 * s, n = n0 + lrow + 32 * s, k = k0 + lk;
            px[s] = (r < R && k < K) ? *reinterpret_cast<const float4*>(x + (int64_t)r * ldx + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            pw[s] = (n < N && k < K) ? *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float acc[4][4] = {{0}};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += PL_KC) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = lrow + 32 * s;
            sx[lk][row] = px[s].x; sx[lk + 1][row] = px[s].y; sx[lk + 2][row] = px[s].z; sx[lk + 3][row] = px[s].w;
            sw[lk][row] = pw[s].x; sw[lk + 1][row] = pw[s].y; sw[lk + 2][row] = pw[s].z; sw[lk + 3][row] = pw[s].w;
        }
        __syncthreads();
        if (k0 + PL_KC < K) fetch(k0 + PL_KC);
#pragma unroll
        for (int kk = 0; kk < PL_KC; ++kk) {
            float a[4], c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = sx[kk][ty * 4 + i]; c[i] = sw[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], c[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty * 4 + i;
        if (r >= R) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            float v = acc[i][j] + bias[n];
            if (epi == PL_TANH_GELU) {
                // 0.5 v (1 + tanh(z)) = v / (1 + exp(-2 z)): no cancellation for v << 0 (exp overflows to +inf there and the result is -0)
                const float zz = 0.7978845608028654f * (v + 0.044715f * v * v * v);
                v = v / (1.0f + expf(-2.0f * zz));
            } else if (epi == PL_RESID) {
                v = resid[(int64_t)r * ldr + n] + v;
            }
            out[(int64_t)r * ldo + n] = v;
        }
    }
}

static int launch_probe_linear(const float* x, int64_t ldx, int64_t zx, const float* W, int64_t ldw, int64_t zw, const float* bias, int64_t zb,
                               const float* resid, int64_t ldr, float* out, int64_t ldo, int64_t zo, int R, int K, int N, int nz, int epi,
                               hipStream_t s) {
    dim3 grid((N + 63) / 64, (R + 63) / 64, nz);
    hipLaunchKernelGGL(ibl_probe_linear_kernel, grid, dim3(256), 0, s, x, ldx, zx, W, ldw, zw, bias, zb, resid, ldr, out, ldo, zo, R, K, N, epi);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// LayerNorm over D <= 1024 columns, one wave per row: mean, then the biased variance of the centred row (torch.nn.LayerNorm)
__global__ __launch_bounds__(256) void ibl_probe_ln_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                           float eps, float* __restrict__ out, int R, int D) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* xr = x + (int64_t)r * D;
    float v[PP_MAXD / 64];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PP_MAXD / 64; ++i) {
        const int c = i * 64 + lane;
        v[i] = c < D ? xr[c] : 0.f;
        s += v[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PP_MAXD / 64; ++i) {
        const int c = i * 64 + lane;
        v[i] = c < D ? v[i] - mean : 0.f;
        q += v[i] * v[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = 1.0f / sqrtf(q / (float)D + eps);
#pragma unroll
    for (int i = 0; i < PP_MAXD / 64; ++i) {
        const int c = i * 64 + lane;
        if (c < D) out[(int64_t)r * D + c] = v[i] * rstd * g[c] + b[c];
    }
}

// ------------------------------------------------------------------------------------------------
// C-ABI of the head
// ------------------------------------------------------------------------------------------------
static int probe_head_check(const char* fn, const ibl_probe_head_desc* d, int batch) {
    if (!d) return ibl_set_error(IBL_ERR_ARG, "%s: null descriptor", fn);
    const int st = probe_pool_check(fn, batch, d->n_tokens, d->dim, d->heads);
    if (st) return st;
    if (d->mlp_dim < 4 || (d->mlp_dim & 3)) return ibl_set_error(IBL_ERR_ARG, "%s: mlp_dim (%d) must be a positive multiple of 4", fn, d->mlp_dim);
    if (!(d->ln_eps >= 0.f)) return ibl_set_error(IBL_ERR_ARG, "%s: ln_eps must be >= 0", fn);
    return IBL_OK;
}

// byte offsets of the IBL_PROBE_WS_* buffers from the 256-byte-aligned workspace base, each on a 256-byte boundary.  The forward pass and
// ibl_probe_head_workspace_layout both read this table.  Returns the end.
static int64_t probe_head_layout(const ibl_probe_head_desc* d, int batch, int64_t offs[IBL_PROBE_WS_COUNT]) {
    const int64_t B = batch, D = d->dim;
    int64_t floats[IBL_PROBE_WS_COUNT];
    floats[IBL_PROBE_WS_PROBS] = B * d->heads * d->n_tokens;
    floats[IBL_PROBE_WS_POOLED] = B * d->heads * D;
    floats[IBL_PROBE_WS_VCAT] = B * D; floats[IBL_PROBE_WS_ATT] = B * D; floats[IBL_PROBE_WS_LN] = B * D;
    floats[IBL_PROBE_WS_HID] = B * d->mlp_dim;
    int64_t p = 0;
    for (int i = 0; i < IBL_PROBE_WS_COUNT; ++i) {
        p = (p + 255) & ~(int64_t)255;
        offs[i] = p;
        p += floats[i] * 4;
    }
    return p;
}

extern "C" int64_t ibl_probe_head_workspace_bytes(const ibl_probe_head_desc* d, int batch) {
    if (probe_head_check("ibl_probe_head_workspace_bytes", d, batch)) return -1;
    int64_t offs[IBL_PROBE_WS_COUNT];
    return probe_head_layout(d, batch, offs) + 256;          // + the round-up of the workspace pointer
}

extern "C" int ibl_probe_head_workspace_layout(const ibl_probe_head_desc* d, int batch, int64_t* offsets, int n) {
    const int st = probe_head_check("ibl_probe_head_workspace_layout", d, batch);
    if (st) return st;
    if (!offsets || n < 0 || n > IBL_PROBE_WS_COUNT) return ibl_set_error(IBL_ERR_ARG, "ibl_probe_head_workspace_layout: bad offsets / n");
    int64_t offs[IBL_PROBE_WS_COUNT];
    probe_head_layout(d, batch, offs);
    for (int i = 0; i < n; ++i) offsets[i] = offs[i];
    return IBL_OK;
}

extern "C" int ibl_probe_head_forward(const ibl_probe_head_desc* d, const ibl_probe_head_weights* w, const float* tokens, int batch,
                                      float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!d || !w || !tokens || !out || !workspace) return ibl_set_error(IBL_ERR_ARG, "ibl_probe_head_forward: null pointer");
    int st = probe_head_check("ibl_probe_head_forward", d, batch);
    if (st) return st;
    if (!w->u || !w->w_v || !w->b_v || !w->w_o || !w->b_o || !w->ln_g || !w->ln_b || !w->w_fc1 || !w->b_fc1 || !w->w_fc2 || !w->b_fc2)
        return ibl_set_error(IBL_ERR_ARG, "ibl_probe_head_forward: null weight pointer");
    if ((reinterpret_cast<uintptr_t>(tokens) & 15) || (reinterpret_cast<uintptr_t>(w->u) & 15) || (reinterpret_cast<uintptr_t>(w->w_v) & 15) ||
        (reinterpret_cast<uintptr_t>(w->w_o) & 15) || (reinterpret_cast<uintptr_t>(w->w_fc1) & 15) || (reinterpret_cast<uintptr_t>(w->w_fc2) & 15))
        return ibl_set_error(IBL_ERR_ARG, "ibl_probe_head_forward: tokens, u and the weight matrices must be 16-byte aligned");
    int64_t offs[IBL_PROBE_WS_COUNT];
    const int64_t end = probe_head_layout(d, batch, offs);
    unsigned char* base = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    if (workspace_bytes < 0 || (base - reinterpret_cast<unsigned char*>(workspace)) + end > workspace_bytes)
        return ibl_set_error(IBL_ERR_ARG, "ibl_probe_head_forward: workspace too small");
    auto buf = [&](int i) { return reinterpret_cast<float*>(base + offs[i]); };
    float* probs = buf(IBL_PROBE_WS_PROBS); float* pooled = buf(IBL_PROBE_WS_POOLED); float* vcat = buf(IBL_PROBE_WS_VCAT);
    float* att = buf(IBL_PROBE_WS_ATT); float* ln = buf(IBL_PROBE_WS_LN); float* hid = buf(IBL_PROBE_WS_HID);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int D = d->dim, H = d->heads, hd = D / H, M = d->mlp_dim;
    st = launch_probe_pool(tokens, batch, d->n_tokens, D, H, w->u, pooled, probs, s);
    if (st) return st;
    // head h: vcat[b][h * hd ..] = W_v[h * hd ..] pooled[b][h] + b_v[h * hd ..]
    st = launch_probe_linear(pooled, (int64_t)H * D, D, w->w_v, D, (int64_t)hd * D, w->b_v, hd, nullptr, 0, vcat, D, hd, batch, D, hd, H, PL_NONE, s);
    if (st) return st;
    st = launch_probe_linear(vcat, D, 0, w->w_o, D, 0, w->b_o, 0, nullptr, 0, att, D, 0, batch, D, D, 1, PL_NONE, s);
    if (st) return st;
    hipLaunchKernelGGL(ibl_probe_ln_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, att, w->ln_g, w->ln_b, d->ln_eps, ln, batch, D);
    IBL_LAUNCH_CHECK();
    st = launch_probe_linear(ln, D, 0, w->w_fc1, D, 0, w->b_fc1, 0, nullptr, 0, hid, M, 0, batch, D, M, 1, PL_TANH_GELU, s);
    if (st) return st;
    return launch_probe_linear(hid, M, 0, w->w_fc2, M, 0, w->b_fc2, 0, att, D, out, D, 0, batch, M, D, 1, PL_RESID, s);
}
