// vit_attention.hip -- the ViT encoder's attention on gfx950 (vit.hip says where it sits in the forward): the rotation of q and k, the
// resident kernel (up to 272 tokens, K and V^T of a head in LDS), the streaming one beyond and its ragged twin (crops of different
// lengths packed back to back), their launchers, and the entries ibl_attention_f16, ibl_attention_stream_f16, ibl_attention_ragged_f16
// and ibl_rope_f16.
#include <type_traits>

#include "vit_kernels.h"

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
int run_rope(u16* qkv, const float* table, int B, int T, int n_prefix, int D, int heads, int k_only, hipStream_t s) {
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
// The body both streaming kernels share: query block qb of head h of the crop whose T rows start at row tok0 of qkv and out.
template <int TERMS>
__device__ __forceinline__ void attention_stream_body(const u16* __restrict__ qkv, u16* __restrict__ out, int T, int64_t tok0, int h, int qb,
                                                      int D, float scale, int cls_only) {
    constexpr int KV = ATT_S_KV, NT = KV / 16, NS = NT / 2;
    constexpr int KROW = 144;               // bytes per K row (64 fp16 + 16 B pad)
    constexpr int VROW = KV * 2 + 16;       // bytes per V^T row
    constexpr int KL = KV * 8 / ATT_S_THREADS;          // uint4 of K per thread and chunk
    constexpr int VL = (KV / 2) * 8 / ATT_S_THREADS;    // (key pair, 8-wide d chunk) tasks of V per thread and chunk
    __shared__ __attribute__((aligned(16))) unsigned char sK[KV * KROW];
    __shared__ __attribute__((aligned(16))) unsigned char sV[64 * VROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = cls_only ? 1 : T;                    // rows that are queries
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

// equal rows: crop b's T rows start at row b * T
template <int TERMS>
__global__ __launch_bounds__(ATT_S_THREADS, 3) void ibl_attention_stream_kernel(const u16* __restrict__ qkv, u16* __restrict__ out, int T,
                                                                                  int D, int heads, float scale, int cls_only) {
    const int nq = cls_only ? 1 : T;
    const int nqb = (nq + ATT_S_QB - 1) / ATT_S_QB;     // the query blocks of a (crop, head) are neighbours in the grid: they share K and V in L2
    const int bh = blockIdx.x / nqb, qb = blockIdx.x % nqb;
    attention_stream_body<TERMS>(qkv, out, T, (int64_t)(bh / heads) * T, bh % heads, qb, D, scale, cls_only);
}

// ragged rows: crop b's rows are seq_off[b] .. seq_off[b + 1] - 1 of the packed qkv and out.  Grid (query blocks of the longest crop,
// heads, batch): the query blocks of a (crop, head) stay neighbours.  A workgroup whose query block lies beyond its crop returns before
// the first barrier -- the whole workgroup does, and the key loop's trip count is the crop's, so every barrier is met by all or by none.
template <int TERMS>
__global__ __launch_bounds__(ATT_S_THREADS, 3) void ibl_attention_ragged_kernel(const u16* __restrict__ qkv, u16* __restrict__ out,
                                                                                  const int* __restrict__ seq_off, int D, float scale,
                                                                                  int cls_only) {
    const int b = blockIdx.z, qb = blockIdx.x;
    const int tok0 = seq_off[b], T = seq_off[b + 1] - tok0;
    if (qb * ATT_S_QB >= (cls_only ? 1 : T)) return;
    attention_stream_body<TERMS>(qkv, out, T, tok0, blockIdx.y, qb, D, scale, cls_only);
}

// terms (1..3; the entries and ibl_vit_forward validate it) -> the kernels' TERMS: f is called with std::integral_constant<int, TERMS>
template <class F>
static void with_terms(int terms, F f) {
    if (terms == 3) f(std::integral_constant<int, 3>{});
    else if (terms == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

// any 1 <= T <= IBL_ATT_STREAM_MAX_TOKENS; the caller has checked that the grid fits
static int run_attention_stream(const u16* qkv, u16* out, int B, int T, int D, int heads, int cls_only, hipStream_t s, int terms) {
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nqb = ((cls_only ? 1 : T) + ATT_S_QB - 1) / ATT_S_QB;
    const int64_t wgs = (int64_t)B * heads * nqb;
    if (wgs > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "attention: batch * heads * query blocks exceeds the grid");
    dim3 grid((unsigned)wgs), block(ATT_S_THREADS);
    with_terms(terms, [&](auto t) {
        hipLaunchKernelGGL((ibl_attention_stream_kernel<decltype(t)::value>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only);
    });
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// seq_off [dev] as ibl_attention_ragged_f16 takes it, max_tokens the longest segment (from the host copy); batch <= 65535 (grid.z)
int run_attention_ragged(const u16* qkv, u16* out, const int* seq_off, int B, int max_tokens, int D, int heads, int cls_only, hipStream_t s,
                         int terms) {
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nqb = ((cls_only ? 1 : max_tokens) + ATT_S_QB - 1) / ATT_S_QB;
    dim3 grid((unsigned)nqb, (unsigned)heads, (unsigned)B), block(ATT_S_THREADS);
    with_terms(terms, [&](auto t) {
        hipLaunchKernelGGL((ibl_attention_ragged_kernel<decltype(t)::value>), grid, block, 0, s, qkv, out, seq_off, D, scale, cls_only);
    });
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// the row offsets of a ragged batch, on the host: ascending from >= 0, every segment 1 .. IBL_ATT_STREAM_MAX_TOKENS rows, at most 65535
// segments (grid.z).  *max_tokens: the longest segment
int ragged_offsets_check(const char* fn, const int32_t* seq_off, int batch, int* max_tokens) {
    *max_tokens = 0;
    if (batch > 65535) return ibl_set_error(IBL_ERR_ARG, "%s: batch %d exceeds the grid (65535)", fn, batch);
    if (seq_off[0] < 0) return ibl_set_error(IBL_ERR_ARG, "%s: seq_off[0] = %d is negative", fn, seq_off[0]);
    for (int b = 0; b < batch; ++b) {
        const int64_t n = (int64_t)seq_off[b + 1] - seq_off[b];
        if (n < 1) return ibl_set_error(IBL_ERR_ARG, "%s: segment %d is empty or descending (%d .. %d)", fn, b, seq_off[b], seq_off[b + 1]);
        if (n > IBL_ATT_STREAM_MAX_TOKENS)
            return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: segment %d has %lld rows > %d", fn, b, (long long)n, IBL_ATT_STREAM_MAX_TOKENS);
        if (n > *max_tokens) *max_tokens = (int)n;
    }
    return IBL_OK;
}

extern "C" int ibl_attention_ragged_f16(const void* qkv, void* out, const int32_t* seq_off_dev, const int32_t* seq_off_host, int batch,
                                        int dim, int heads, int cls_only, int terms, void* stream) {
    const char* fn = "ibl_attention_ragged_f16";
    if (batch < 0) return ibl_set_error(IBL_ERR_ARG, "%s: negative batch (%d)", fn, batch);
    if (terms < 1 || terms > 3) return ibl_set_error(IBL_ERR_ARG, "%s: terms %d outside 1..3", fn, terms);
    if (cls_only != 0 && cls_only != 1) return ibl_set_error(IBL_ERR_ARG, "%s: cls_only must be 0 or 1", fn);
    if (heads <= 0 || heads > 65535 || dim != heads * 64)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: dim (%d) must be 64 * heads (%d): head_dim is 64", fn, dim, heads);
    if (batch == 0) return IBL_OK;
    if (!qkv || !out || !seq_off_dev || !seq_off_host) return ibl_set_error(IBL_ERR_ARG, "%s: null pointer", fn);
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(seq_off_dev) & 3))
        return ibl_set_error(IBL_ERR_ARG, "%s: qkv must be 16-byte, out 8-byte and seq_off 4-byte aligned", fn);
    int max_tokens;
    const int st = ragged_offsets_check(fn, seq_off_host, batch, &max_tokens);
    if (st) return st;
    return run_attention_ragged(reinterpret_cast<const u16*>(qkv), reinterpret_cast<u16*>(out), seq_off_dev, batch, max_tokens, dim, heads,
                                cls_only, reinterpret_cast<hipStream_t>(stream), terms);
}

int run_attention(const u16* qkv, u16* out, int B, int T, int D, int heads, int cls_only, hipStream_t s, int terms) {
    if (T > 272) {      // beyond the resident kernel's widest tier: keys and values stream through LDS
        if (T > IBL_ATT_STREAM_MAX_TOKENS)
            return ibl_set_error(IBL_ERR_UNSUPPORTED, "attention: n_tokens %d > %d not supported", T, IBL_ATT_STREAM_MAX_TOKENS);
        return run_attention_stream(qkv, out, B, T, D, heads, cls_only, s, terms);
    }
    const float scale = 0.125f;   // 1/sqrt(64)
    const int nt = (T + 15) / 16;
    dim3 grid(B * heads), block(ATT_THREADS);
#define IBL_ATT(NTV)                                                                                                                    \
    with_terms(terms, [&](auto t) {                                                                                                     \
        hipLaunchKernelGGL((ibl_attention_kernel<NTV, decltype(t)::value>), grid, block, 0, s, qkv, out, T, D, heads, scale, cls_only); \
    })
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

// ibl_attention_f16 and ibl_attention_stream_f16: one validation.  `fn` is the entry's name for the messages, `max_tokens` its token
// limit, `per_head` the workgroups its launch may take per (crop, head) and `grid` what their total is made of, for the message (the grid bound).
// *run: something is to launch
static int attention_check(const char* fn, int max_tokens, int64_t per_head, const char* grid, const void* qkv, const void* out, int batch,
                           int n_tokens, int dim, int heads, int cls_only, int terms, bool* run) {
    *run = false;
    if (batch < 0 || n_tokens < 0) return ibl_set_error(IBL_ERR_ARG, "%s: negative batch (%d) or n_tokens (%d)", fn, batch, n_tokens);
    if (terms < 1 || terms > 3) return ibl_set_error(IBL_ERR_ARG, "%s: terms %d outside 1..3", fn, terms);
    if (cls_only != 0 && cls_only != 1) return ibl_set_error(IBL_ERR_ARG, "%s: cls_only must be 0 or 1", fn);
    if (heads <= 0 || dim != heads * 64)
        return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: dim (%d) must be 64 * heads (%d): head_dim is 64", fn, dim, heads);
    if (n_tokens > max_tokens) return ibl_set_error(IBL_ERR_UNSUPPORTED, "%s: n_tokens %d > %d not supported", fn, n_tokens, max_tokens);
    if ((int64_t)batch * heads * per_head > 0x7fffffff) return ibl_set_error(IBL_ERR_ARG, "%s: %s exceeds the grid", fn, grid);
    if (batch == 0 || n_tokens == 0) return IBL_OK;
    if (!qkv || !out) return ibl_set_error(IBL_ERR_ARG, "%s: null pointer", fn);
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return ibl_set_error(IBL_ERR_ARG, "%s: qkv must be 16-byte and out 8-byte aligned", fn);
    *run = true;
    return IBL_OK;
}

extern "C" int ibl_attention_f16(const void* qkv, void* out, int batch, int n_tokens, int dim, int heads, int cls_only, int terms,
                                 void* stream) {
    bool run;
    const int st = attention_check("ibl_attention_f16", 272, 1, "batch * heads", qkv, out, batch, n_tokens, dim, heads,
                                   cls_only, terms, &run);
    if (st || !run) return st;
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
    bool run;
    const int st = attention_check("ibl_attention_stream_f16", IBL_ATT_STREAM_MAX_TOKENS,
                                   ((int64_t)n_tokens + ATT_S_QB - 1) / ATT_S_QB, "batch * heads * query blocks", qkv, out,
                                   batch, n_tokens, dim, heads, cls_only, terms, &run);
    if (st || !run) return st;
    return run_attention_stream(reinterpret_cast<const u16*>(qkv), reinterpret_cast<u16*>(out), batch, n_tokens, dim, heads, cls_only,
                                reinterpret_cast<hipStream_t>(stream), terms);
}
