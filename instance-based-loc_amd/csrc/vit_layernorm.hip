// vit_layernorm.hip -- the ViT encoder's LayerNorm on gfx950 (vit.hip says where it sits in the forward): the kernel, its launcher and the
// entry ibl_layernorm_f32.
#include "vit_kernels.h"

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
int launch_layernorm(const float* x, int64_t ld_x, int64_t n_rows, int dim, const float* g, const float* b, float eps, void* out,
                     int64_t ld_out, int terms, hipStream_t s) {
    const dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
    if (terms == 0) hipLaunchKernelGGL((ibl_layernorm_kernel<true>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else if (terms == 1) hipLaunchKernelGGL((ibl_layernorm_kernel<false, 1>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else if (terms == 2) hipLaunchKernelGGL((ibl_layernorm_kernel<false, 2>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    else hipLaunchKernelGGL((ibl_layernorm_kernel<false, 3>), grid, block, 0, s, x, ld_x, n_rows, dim, g, b, eps, out, ld_out);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
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
