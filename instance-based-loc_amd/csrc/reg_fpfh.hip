// reg_fpfh.hip -- SPFH / FPFH of every point of a batch from its <= max_nn nearest neighbours within a radius (Open3D
// compute_fpfh_feature, utils/fpfh_register.py:90-97), alone (SpfhConsumer, after a normals search) or fused with the normals: ONE
// neighbour search writes the lists and marks the normal's own neighbours (ListNormalConsumer), ibl_normals_from_mask_kernel solves the
// normals, ibl_spfh_lists_kernel / ibl_spfh_queue_kernel build the histograms, ibl_fpfh_kernel weights them.  The selection itself is
// knn_select.h, the normal's arithmetic knn_normal.h.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <vector>

#include "reg_common.h"
#include "knn_select.h"
#include "knn_normal.h"

__device__ inline void pair_features_d(const float4& p1, const float4& n1f, const float4& p2, const float4& n2f, double* f) {
    double d[3] = {(double)p2.x - (double)p1.x, (double)p2.y - (double)p1.y, (double)p2.z - (double)p1.z};
    double n1[3] = {n1f.x, n1f.y, n1f.z}, n2[3] = {n2f.x, n2f.y, n2f.z};
    const double r = sqrt(dot3d(d, d));
    f[0] = 5.0; f[1] = f[2] = 0;          // (all-zero features: theta = 0 lies in bin 5; f[0] is a bin index, see below)
    if (r == 0.0) return;
    const double a1 = dot3d(n1, d) / r, a2 = dot3d(n2, d) / r;
    double na[3], nb[3];
    // acos(|a1|) > acos(|a2|)  <=>  |a1| < |a2|  (false when either exceeds 1: acos -> NaN)
    if (fabs(a1) < fabs(a2) && fabs(a1) <= 1.0 && fabs(a2) <= 1.0) {
        for (int t = 0; t < 3; ++t) { na[t] = n2[t]; nb[t] = n1[t]; d[t] = -d[t]; }
        f[2] = -a2;
    } else {
        for (int t = 0; t < 3; ++t) { na[t] = n1[t]; nb[t] = n2[t]; }
        f[2] = a1;
    }
    double v[3], w[3];
    cross3d(d, na, v);
    const double vn = sqrt(dot3d(v, v));
    if (vn == 0.0) { f[0] = 5.0; f[1] = f[2] = 0; return; }
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    cross3d(na, v, w);
    f[1] = dot3d(v, nb);
    // f[0] carries the BIN of theta = atan2(w.nb, na.nb), floor(11 (theta + pi) / (2 pi)), found without the arctangent (~120 fp64
    // instructions): theta' = theta + pi is the angle of p = (-x, -y), and within a half plane "theta' >= 2 pi k / 11" is the sign of the
    // cross product with the boundary direction -- five tests.  The half plane follows atan2's sign-of-zero rule (y = +0, x < 0 is
    // +pi -> last bin; y = -0 is -pi -> bin 0: antiparallel normals on a plane land there).  It can differ from the arctangent only
    // for an angle within rounding of a boundary.
    {
        const double x = dot3d(na, nb), y = dot3d(w, nb);
        constexpr double CK[10] = {0.84125353283118121, 0.41541501300188644, -0.142314838273285, -0.65486073394528499, -0.95949297361449737, -0.95949297361449748, -0.65486073394528521, -0.14231483827328523, 0.41541501300188605, 0.84125353283118121};
        constexpr double SK[10] = {0.54064081745559756, 0.90963199535451833, 0.9898214418809328, 0.75574957435425827, 0.28173255684142967, -0.28173255684142939, -0.75574957435425816, -0.98982144188093268, -0.90963199535451855, -0.54064081745559744};
        const double px = -x, py = -y;
        int bin;
        if (!(__double_as_longlong(py) < 0)) {            // py = +0 or positive: theta' in [0, pi]
            bin = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) bin += (CK[k] * py - SK[k] * px >= 0.0) ? 1 : 0;
        } else {                                           // theta' in (pi, 2 pi]
            bin = 5;
#pragma unroll
            for (int k = 5; k < 10; ++k) bin += (CK[k] * py - SK[k] * px >= 0.0) ? 1 : 0;
        }
        if (x == 0.0 && y == 0.0) bin = (__double_as_longlong(x) < 0) ? ((__double_as_longlong(y) < 0) ? 0 : 10) : 5;   // atan2(+-0, +-0)
        f[0] = (double)bin;
    }
}

__device__ __forceinline__ int clamp_bin11(int h) { return h < 0 ? 0 : (h >= 11 ? 10 : h); }

// The three SPFH bins of a pair in fp32, or "undecided" (round 4).  pair_features_d spends ~150 fp64 operations (two square roots, five
// divisions) on a pair whose only output is three bin INDICES: the fp64 values matter where they sit next to a bin boundary, nowhere
// else.  This evaluates the same expressions in fp32 and calls a pair decided only when every decision on the way -- which normal carries
// the frame (|a1| < |a2|), the half plane and the five boundary tests of theta, the bins of v . nb and of a -- clears a guard band at least
// ten times the fp32 error of the value tested (u = 2^-24; inputs are fp32, normals unit to 1 ulp):
//   d = p2 - p1: one rounding (relative u).  a = (n . d) rsq(|d|^2): absolute error <= 8e-7 -> band 1e-5 on |a1| - |a2| and on 1 - |a|,
//     5e-5 on the bin fraction of a.
//   v = d x na: component error <= 6 u |d|; pairs with |v|^2 < 1e-2 |d|^2 (d within 5.7 degrees of the frame's normal) are undecided, for
//     the rest the normalised v is within 1.3e-5 of the fp64 one, and so are v . nb, w = na x v, y = w . nb and the boundary forms
//     CK y - SK x -> band SPFH_G = 2e-4 on y and the five forms, 11 / 2 SPFH_G on the bin fraction of v . nb.
// Undecided pairs (measured: see DESIGN.md) are evaluated by pair_features_d afterwards, so the histograms are those of the fp64 evaluation bit for bit
// (IBL_SPFH_F64=1 runs every pair in fp64: tests/test_gpu_features.py compares the two).
#define SPFH_G 2.0e-4f
__device__ __forceinline__ bool pair_bins_f32(const float4& p1, const float4& n1, const float4& p2, const float4& n2, int* b0, int* b1, int* b2) {
    float dx = p2.x - p1.x, dy = p2.y - p1.y, dz = p2.z - p1.z;
    *b0 = 5; *b1 = 5; *b2 = 5;
    if (dx == 0.0f && dy == 0.0f && dz == 0.0f) return true;                  // coincident points: the zero features' bins (d is exact there)
    const float r2 = dx * dx + dy * dy + dz * dz;
    if (r2 < 1.0e-20f) return false;
    const float rinv = __builtin_amdgcn_rsqf(r2);
    const float a1 = (n1.x * dx + n1.y * dy + n1.z * dz) * rinv, a2 = (n2.x * dx + n2.y * dy + n2.z * dz) * rinv;
    const float f1a = fabsf(a1), f2a = fabsf(a2);
    const bool same_n = n1.x == n2.x && n1.y == n2.y && n1.z == n2.z;          // (planes: a1 == a2 in fp64 as well -> no swap)
    bool sure = (same_n || fabsf(f1a - f2a) > 1.0e-5f) && fmaxf(f1a, f2a) < 1.0f - 1.0e-5f;
    const bool swap = f1a < f2a;
    float nax, nay, naz, nbx, nby, nbz, f3;
    if (swap) { nax = n2.x; nay = n2.y; naz = n2.z; nbx = n1.x; nby = n1.y; nbz = n1.z; dx = -dx; dy = -dy; dz = -dz; f3 = -a2; }
    else { nax = n1.x; nay = n1.y; naz = n1.z; nbx = n2.x; nby = n2.y; nbz = n2.z; f3 = a1; }
    float vx = dy * naz - dz * nay, vy = dz * nax - dx * naz, vz = dx * nay - dy * nax;
    const float vn2 = vx * vx + vy * vy + vz * vz;
    sure = sure && vn2 > 1.0e-2f * r2;                                         // sin^2 of the angle between d and the frame's normal
    const float vinv = __builtin_amdgcn_rsqf(fmaxf(vn2, 1e-30f));
    vx *= vinv; vy *= vinv; vz *= vinv;
    const float f2 = vx * nbx + vy * nby + vz * nbz;
    const float wx = nay * vz - naz * vy, wy = naz * vx - nax * vz, wz = nax * vy - nay * vx;
    const float x = nax * nbx + nay * nby + naz * nbz, y = wx * nbx + wy * nby + wz * nbz;
    const float px = -x, py = -y;
    sure = sure && fabsf(py) > SPFH_G;
    constexpr float CK[10] = {0.84125353283118121f, 0.41541501300188644f, -0.142314838273285f, -0.65486073394528499f, -0.95949297361449737f,
                              -0.95949297361449748f, -0.65486073394528521f, -0.14231483827328523f, 0.41541501300188605f, 0.84125353283118121f};
    constexpr float SK[10] = {0.54064081745559756f, 0.90963199535451833f, 0.9898214418809328f, 0.75574957435425827f, 0.28173255684142967f,
                              -0.28173255684142939f, -0.75574957435425816f, -0.98982144188093268f, -0.90963199535451855f, -0.54064081745559744f};
    int bin = py >= 0.0f ? 0 : 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float t = py >= 0.0f ? CK[k] * py - SK[k] * px : CK[k + 5] * py - SK[k + 5] * px;
        sure = sure && fabsf(t) > SPFH_G;
        bin += t >= 0.0f ? 1 : 0;
    }
    const float g1 = 11.0f * (f2 + 1.0f) * 0.5f, g2 = 11.0f * (f3 + 1.0f) * 0.5f;
    const float fl1 = floorf(g1), fl2 = floorf(g2);
    constexpr float GB1 = 5.5f * SPFH_G, GB2 = 5.0e-5f;
    sure = sure && (g1 - fl1) > GB1 && (g1 - fl1) < 1.0f - GB1 && (g2 - fl2) > GB2 && (g2 - fl2) < 1.0f - GB2;
    *b0 = bin; *b1 = clamp_bin11((int)fl1); *b2 = clamp_bin11((int)fl2);
    return sure;
}

template <class Acc>
struct SpfhConsumer {
    static constexpr bool WANTS_INNER = false;
    const float4* normals;   // original order
    Acc acc;
    unsigned char* spfh_cnt; // [N][36] integer SPFH histograms
    int* nbr_idx;            // [N][K]
    float* nbr_d2;           // [N][K]
    int* nbr_cnt;            // [N]
    int K;
    int qi;
    float4 q, qn;
    WaveLds* L;
    int ncount;
    __device__ void begin(int) {
        const int lane = threadIdx.x & 63;
        if (lane < 33) L->scratch[lane] = 0;
        ncount = 0;
        wave_lds_sync();
    }
    // selected candidates are only appended to the per-wave list here; the pair features (fp64, ~300 instructions)
    // are computed afterwards on densely packed lanes
    __device__ void accept(bool sel, int j, const float4&, float d2) {
        const int lane = threadIdx.x & 63;
        const unsigned long long m = __ballot(sel);
        if (sel) {
            const int pos = ncount + __popcll(m & ((1ull << lane) - 1ull));
            L->sel_j[pos] = j;
            L->sel_d2[pos] = d2;
        }
        ncount += __popcll(m);
    }
    __device__ void finish(int k) {
        const int lane = threadIdx.x & 63;
        int* hist = L->scratch;
        sort_selected_by_index<true>(L, acc, k);
        for (int t = lane; t < k; t += 64) {
            const int j = L->b_j[t];
            const int jo = acc.ord(j);
            nbr_idx[(int64_t)qi * K + t] = jo;
            nbr_d2[(int64_t)qi * K + t] = __uint_as_float(L->b_bits[t]);
            if (jo != qi) {
                double f[3];
                pair_features_d(q, qn, acc.pt(j), normals[jo], f);
                atomicAdd(&hist[clamp_bin11((int)f[0])], 1);
                atomicAdd(&hist[11 + clamp_bin11((int)floor(11 * (f[1] + 1.0) * 0.5))], 1);
                atomicAdd(&hist[22 + clamp_bin11((int)floor(11 * (f[2] + 1.0) * 0.5))], 1);
            }
        }
        wave_lds_sync();
        // SPFH(i)[b] = hist[b] * 100 / (k - 1): only the integer histogram (<= 255 per bin) is stored, 36 bytes per point,
        // so the FPFH pass gathers 36 B instead of 132 B per neighbour; the fp32 value is rebuilt on the fly
        if (lane < 36) spfh_cnt[(int64_t)qi * 36 + lane] = lane < 33 ? (unsigned char)hist[lane] : (unsigned char)0;
        if (lane == 0) nbr_cnt[qi] = k;
    }
};

// The 100-neighbour search and the normals in one pass (instance features: normal radius <= feature radius, <= 32 normal neighbours):
// the <= kn nearest of a point within the normal radius are among its k nearest within the feature radius, so the selected list
// serves both -- the neighbour lists are written for the SPFH / FPFH kernels that follow, and the normal's own neighbours are taken
// from the list (all entries inside the normal radius, or the kn smallest by (d2 bits, index) through a 64-bin histogram of the
// list) and parked for the batched solve, in the same ascending-index order as the stand-alone normals kernel: identical normals.
// This removes that kernel's whole search (2.9 of the 10.8 ms of the two searches per step).
template <class Acc>
struct ListNormalConsumer {
    // tile_select_guess marks the normal's own neighbours (the <= kn nearest inside rn2) while it selects the list: they fall out of the
    // same histogram, so finish() need not find them again (its 64-bin histogram and rank loops were 4 300 of a query's 24 000 clocks)
    static constexpr bool WANTS_INNER = true;
    bool flagged = false;    // accept_in() was used: bit 31 of the stored d2 marks an inner neighbour
    // Round 3: the consumer no longer solves the normal.  It records WHICH entries of the query's neighbour list are the normal's
    // neighbours as a 128-bit mask over the list slots (the list is in ascending original index: the order of the covariance sums);
    // ibl_normals_from_mask_kernel then solves every point of the batch with one lane per point.  In this kernel the solve ran on 8 of
    // 64 lanes, every eighth query, behind ~250 VGPRs of fp64 code (the tile kernel spilled), and kept 2.3 KB of LDS per workgroup.
    unsigned* nrm_mask;      // out [N][4]
    Acc acc;
    int* nbr_idx;            // [N][K]
    float* nbr_d2;           // [N][K]
    int* nbr_cnt;            // [N]
    int K;
    float rn2;               // squared normal radius
    int kn;                  // normal neighbours (<= NP_MAXK)
    int qi;
    WaveLds* L;
    int ncount;
    __device__ void begin(int) { ncount = 0; }
    __device__ void accept(bool sel, int j, const float4&, float d2) {
        const int lane = threadIdx.x & 63;
        const unsigned long long m = __ballot(sel);
        if (sel) {
            const int pos = ncount + __popcll(m & ((1ull << lane) - 1ull));
            L->sel_j[pos] = j;
            L->sel_d2[pos] = d2;
        }
        ncount += __popcll(m);
    }
    __device__ void accept_in(bool sel, int j, float d2, bool inner) {
        const int lane = threadIdx.x & 63;
        const unsigned long long m = __ballot(sel);
        if (sel) {
            const int pos = ncount + __popcll(m & ((1ull << lane) - 1ull));
            L->sel_j[pos] = j;
            L->sel_d2[pos] = __uint_as_float(__float_as_uint(d2) | (inner ? 0x80000000u : 0u));
        }
        ncount += __popcll(m);
        flagged = true;
    }
    __device__ void finish_flagged(int k) {
        const int lane = threadIdx.x & 63;
        sort_selected_by_index<true>(L, acc, k);                  // b_j: handles, b_bits: d2 bits | inner flag, ascending original index
        unsigned long long mm[2] = {0ull, 0ull};
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int t = 64 * c + lane;
            const bool v = t < k;
            const unsigned bits = v ? L->b_bits[t] : 0u;
            if (v) {
                nbr_idx[(int64_t)qi * K + t] = acc.ord(L->b_j[t]);
                nbr_d2[(int64_t)qi * K + t] = __uint_as_float(bits & 0x7FFFFFFFu);
            }
            mm[c] = __ballot(v && (bits >> 31) != 0u);
        }
        if (lane == 0) {
            nbr_cnt[qi] = k;
            *reinterpret_cast<uint4*>(nrm_mask + 4 * (int64_t)qi) =
                make_uint4((unsigned)mm[0], (unsigned)(mm[0] >> 32), (unsigned)mm[1], (unsigned)(mm[1] >> 32));
        }
    }
    __device__ void finish(int k) {
        if (flagged) { finish_flagged(k); return; }
        const int lane = threadIdx.x & 63;
        const unsigned long long lt_mask = (1ull << lane) - 1ull;
#ifdef KNN_LAB_CLK
        long long _clk_prev = (long long)__builtin_amdgcn_s_memtime();
#endif
        sort_selected_by_index<true>(L, acc, k);                  // b_j: handles, b_bits: d2 bits, ascending original index
        KNN_CLK(13);
        int n_in = 0;
        for (int t0 = 0; t0 < k; t0 += 64) {
            const int t = t0 + lane;
            const bool v = t < k;
            const unsigned bits = v ? L->b_bits[t] : 0x7F800000u;
            if (v) {
                nbr_idx[(int64_t)qi * K + t] = acc.ord(L->b_j[t]);
                nbr_d2[(int64_t)qi * K + t] = __uint_as_float(bits);
            }
            n_in += __popcll(__ballot(v && __uint_as_float(bits) < rn2));
        }
        if (lane == 0) nbr_cnt[qi] = k;
        KNN_CLK(14);
        // ---- the normal's neighbours
        int b30 = 64, need = 0, popb = 0;
        const float nscale = 64.0f / rn2;
        auto nbin = [&](float d2) { const int b = (int)(d2 * nscale); return b > 63 ? 63 : b; };
        if (n_in > kn) {
            int* nh = L->scratch;                                   // 64 bins over [0, rn2); free once the index sort is done
            nh[lane] = 0;
            wave_lds_sync();
            for (int t = lane; t < k; t += 64) {
                const float d2 = __uint_as_float(L->b_bits[t]);
                if (d2 < rn2) atomicAdd(&nh[nbin(d2)], 1);
            }
            wave_lds_sync();
            const int c = nh[lane];
            int incl = wave_incl_scan_i(c);
            const unsigned long long m = __ballot(incl >= kn);
            b30 = __ffsll((long long)m) - 1;
            need = kn - __shfl(incl - c, b30, 64);
            // the entries of the boundary bin, for the rank by (d2 bits, original index)
            for (int t0 = 0; t0 < k; t0 += 64) {
                const int t = t0 + lane;
                const float d2 = t < k ? __uint_as_float(L->b_bits[t]) : INFINITY;
                const bool bd = d2 < rn2 && nbin(d2) == b30;
                const unsigned long long mb = __ballot(bd);
                if (bd) {
                    const int pos = popb + __popcll(mb & lt_mask);
                    L->sel_d2[pos] = d2;
                    L->sel_j[pos] = t;                               // position in the index-sorted list = index order
                }
                popb += __popcll(mb);
            }
            wave_lds_sync();
        }
        unsigned long long mmk[2] = {0ull, 0ull};
        for (int t0 = 0; t0 < k; t0 += 64) {
            const int t = t0 + lane;
            const float d2 = t < k ? __uint_as_float(L->b_bits[t]) : INFINITY;
            bool member = d2 < rn2;
            if (member && n_in > kn) {
                const int b = nbin(d2);
                if (b > b30) member = false;
                else if (b == b30) {
                    const unsigned mb = __float_as_uint(d2);
                    int rank = 0;
                    for (int u = 0; u < popb; ++u) {
                        const unsigned ub = __float_as_uint(L->sel_d2[u]);
                        rank += (ub < mb || (ub == mb && L->sel_j[u] < t)) ? 1 : 0;
                    }
                    member = rank < need;
                }
            }
            mmk[t0 >> 6] = __ballot(member);
        }
        KNN_CLK(15);
        if (lane == 0)
            *reinterpret_cast<uint4*>(nrm_mask + 4 * (int64_t)qi) =
                make_uint4((unsigned)mmk[0], (unsigned)(mmk[0] >> 32), (unsigned)mmk[1], (unsigned)(mmk[1] >> 32));
    }
};

struct SpfhFactory {
    // its tile: 2^3 cells, geometry only: the packed tile (original index in the staged point's w), three workgroups per CU
    static constexpr int TILE_TS = KNN_TILE_FEATURE, TILE_CAP = KNN_TILE_CAP3, TILE_OCC = 3;
    static constexpr bool TILE_PACK = true;
    typedef NoPending Pending;
    const float4* normals; unsigned char* spfh_cnt; int* nbr_idx; float* nbr_d2; int* nbr_cnt; int K;
    template <class Acc> __device__ void flush(Pending*, const Acc&) const {}
    template <class Acc> __device__ void flush_block(Pending*, const Acc&) const {}
    template <class Acc> __device__ SpfhConsumer<Acc> make(int qi, const float4& q, WaveLds* L, const Acc& acc, Pending* = nullptr) const {
        SpfhConsumer<Acc> c;
        c.normals = normals; c.acc = acc; c.spfh_cnt = spfh_cnt; c.nbr_idx = nbr_idx; c.nbr_d2 = nbr_d2; c.nbr_cnt = nbr_cnt; c.K = K;
        c.qi = qi; c.q = q; c.qn = normals[qi]; c.L = L; c.ncount = 0;
        return c;
    }
};
struct ListNormalFactory {
    static constexpr int TILE_TS = KNN_TILE_FEATURE, TILE_CAP = KNN_TILE_CAP3, TILE_OCC = 3;      // (the packed tile of SpfhFactory)
    static constexpr bool TILE_PACK = true;
    typedef NoPending Pending;
    unsigned* nrm_mask; int* nbr_idx; float* nbr_d2; int* nbr_cnt; int K; float rn2; int kn;
    template <class Acc> __device__ void flush(Pending*, const Acc&) const {}
    template <class Acc> __device__ void flush_block(Pending*, const Acc&) const {}
    template <class Acc> __device__ ListNormalConsumer<Acc> make(int qi, const float4&, WaveLds* L, const Acc& acc, Pending* = nullptr) const {
        ListNormalConsumer<Acc> c;
        c.nrm_mask = nrm_mask; c.acc = acc; c.nbr_idx = nbr_idx; c.nbr_d2 = nbr_d2; c.nbr_cnt = nbr_cnt; c.K = K; c.rn2 = rn2; c.kn = kn;
        c.qi = qi; c.L = L; c.ncount = 0;
        return c;
    }
};

// Position of histogram bin b in the "matching order" of the feature search (reg_match.hip, oracle_reg.c FEAT_ORDER: the
// three histograms from their centre bins outwards, interleaved).  Instance features are stored in that order so that the
// search reads the terms of its early-abandon chain contiguously.
__constant__ int FEAT_POS[33] = {29, 23, 17, 11, 5, 2, 8, 14, 20, 26, 32, 27, 21, 15, 9, 3, 0, 6, 12, 18, 24, 30, 28, 22, 16, 10, 4, 1, 7, 13, 19, 25, 31};

// FPFH(i) = 100 * sum_k SPFH(k)/d2_k / blocksum + SPFH(i)   (one wave per point, lanes = bins)
__device__ __forceinline__ float spfh_value(const unsigned char* __restrict__ spfh_cnt, const int* __restrict__ nbr_cnt, int j, int b) {
    const int kj = nbr_cnt[j];
    if (kj <= 1) return 0.0f;
    return (float)((double)spfh_cnt[(int64_t)j * 36 + b] * (100.0 / (double)(kj - 1)));
}

// Neighbour rows are gathered 64 at a time (one per lane, all loads in flight together) into a per-wave LDS tile;
// the lanes then switch roles to "one histogram bin each" and walk the tile.  The sum over neighbours keeps the list order.
struct FpfhTile {
    unsigned char cnt[64][36];
    double w[64];         // (100 / (k_j - 1)) / d2: the weight of the neighbour's integer histogram; 0 for a skipped entry (the point
                          // itself, zero distance, a neighbour without SPFH)
};

// A workgroup serves FPFH_Q = 7 points: thread p < 231 owns (point p / 33, bin p % 33), so 231 of its 256 lanes work (one wave per
// point left 31 of 64 idle in the loop below, which is the whole kernel).  Neighbour rows are staged 64 per point at a time; each
// (point, bin) sum runs over the neighbour list in its stored order, exactly as before.
#define FPFH_Q 7
__global__ __launch_bounds__(256) void ibl_fpfh_kernel(const unsigned char* __restrict__ spfh_cnt, const int* __restrict__ nbr_idx,
                                                       const float* __restrict__ nbr_d2, const int* __restrict__ nbr_cnt, int K, int n,
                                                       int matching_order, float* __restrict__ fpfh) {
    __shared__ FpfhTile tiles[FPFH_Q];
    __shared__ double accs[FPFH_Q][33];
    __shared__ int kq[FPFH_Q];
    const int tid = threadIdx.x;
    const int q0 = IBL_XCD_BLOCK(blockIdx.x, gridDim.x) * FPFH_Q;
    if (tid < FPFH_Q) kq[tid] = q0 + tid < n ? nbr_cnt[q0 + tid] : 0;
    __syncthreads();
    int kmax = 0;
#pragma unroll
    for (int u = 0; u < FPFH_Q; ++u) kmax = max(kmax, kq[u]);
    const int qq = tid / 33, b = tid - qq * 33;            // tid >= 231: no work (qq == 7)
    const bool mine = qq < FPFH_Q && q0 + qq < n;
    const int qi = q0 + qq;
    const int k = mine ? kq[qq] : 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < kmax; t0 += 64) {
        for (int e = tid; e < FPFH_Q * 64; e += 256) {     // stage row t0 + r of point sq
            const int sq = e >> 6, r = e & 63, t = t0 + r, si = q0 + sq;
            if (si < n && t < kq[sq]) {
                FpfhTile& S = tiles[sq];
                const int j = nbr_idx[(int64_t)si * K + t];
                const double dist = (double)nbr_d2[(int64_t)si * K + t];
                const int kj = nbr_cnt[j];
                // a 36-byte row as 16 + 16 + 4 bytes (rows are 4-byte aligned: the 4-byte aligned struct makes these two
                // global_load_dwordx4 + one dword instead of nine dword gathers per row)
                const unsigned char* src = spfh_cnt + (int64_t)j * 36;
                const ibl_u4_a4 r0 = *reinterpret_cast<const ibl_u4_a4*>(src), r1 = *reinterpret_cast<const ibl_u4_a4*>(src + 16);
                const unsigned r2w = *reinterpret_cast<const unsigned*>(src + 32);
                unsigned int* dst = reinterpret_cast<unsigned int*>(S.cnt[r]);
                dst[0] = r0.x; dst[1] = r0.y; dst[2] = r0.z; dst[3] = r0.w; dst[4] = r1.x; dst[5] = r1.y; dst[6] = r1.z; dst[7] = r1.w; dst[8] = r2w;
                // SPFH(j)[b] / d2 = count x (increment / d2) in double (Open3D keeps its histograms in double; oracle_fpfh likewise): one
                // division per neighbour, one fma per (neighbour, bin); a zero weight or an empty bin adds an exact zero
                S.w[r] = (j == si || dist == 0.0 || kj <= 1) ? 0.0 : (100.0 / (double)(kj - 1)) / dist;
            }
        }
        __syncthreads();
        if (mine && k > 1) {
            const FpfhTile& T = tiles[qq];
            const int m = min(64, k - t0);
            // (count as a double without v_cvt_f64_u32, a quarter-rate instruction that was the hottest of this loop: 2^52 + c has c in its
            // low mantissa bits, and subtracting 2^52 leaves c exactly)
            for (int r = 0; r < m; ++r)
                acc = fma(__hiloint2double(0x43300000, (int)T.cnt[r][b]) - 4503599627370496.0, T.w[r], acc);
        }
        __syncthreads();
    }
    if (mine) accs[qq][b] = acc;
    __syncthreads();
    if (mine) {
        // block sums over bins 0-10, 11-21, 22-32
        double sum = 0.0;
        const int blk = b / 11;
        for (int t = 0; t < 11; ++t) sum += accs[qq][blk * 11 + t];
        float out = 0.0f;
        if (k > 1) {
            const double sc = sum != 0.0 ? 100.0 / sum : 0.0;
            out = (float)(acc * sc + (double)spfh_value(spfh_cnt, nbr_cnt, qi, b));
        }
        fpfh[(int64_t)qi * 33 + (matching_order ? FEAT_POS[b] : b)] = out;
    }
}

int ibl_launch_fpfh(ibl_reg_ctx* ctx, const BatchGrid& g, const float4* pts, const float4* normals, const int* seg_off, int n, double radius, int max_nn,
                    unsigned char* spfh, int* nbr_idx, float* nbr_d2, int* nbr_cnt, float* fpfh, int matching_order, int* status,
                    hipStream_t s) {
    if (n <= 0) return IBL_OK;
    if (max_nn > 256) return ibl_set_error(IBL_ERR_UNSUPPORTED, "fpfh: max_nn %d > 256 (SPFH histograms are stored as bytes)", max_nn);
    void* tok;
    ibl_prof_begin(IBL_PROF_SPFH, 156.0 * (double)n, s, &tok);
    const int st = launch_knn(ctx, g, seg_off, n, 0, n, radius, max_nn, SpfhFactory{normals, spfh, nbr_idx, nbr_d2, nbr_cnt, max_nn}, status, s);
    ibl_prof_end(tok, s);
    if (st) return st;
    hipLaunchKernelGGL(ibl_fpfh_kernel, dim3((n + FPFH_Q - 1) / FPFH_Q), dim3(256), 0, s, spfh, nbr_idx, nbr_d2, nbr_cnt, max_nn, n, matching_order, fpfh);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// Normals of every point from its neighbour list and the 128-bit mask of the list slots that are the normal's own neighbours (written by
// ListNormalConsumer): one lane per point, the moment sums in list order = ascending original index, exactly the arithmetic of
// normal_solve -- a point's normal does not depend on which kernel found its neighbours.
__global__ __launch_bounds__(256) void ibl_normals_from_mask_kernel(const float4* __restrict__ pts, const int* __restrict__ nbr_idx, int K,
                                                                    const unsigned* __restrict__ nrm_mask, int n, float4* __restrict__ normals) {
    const int qi = IBL_XCD_BLOCK(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (qi >= n) return;
    const uint4 m4 = *reinterpret_cast<const uint4*>(nrm_mask + 4 * (int64_t)qi);
    const unsigned w[4] = {m4.x, m4.y, m4.z, m4.w};
    double c[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) c[t] = 0.0;
    int k = 0;
    // eight neighbours per step: their list entries are read together, then their points (a lane's walk was two dependent loads per
    // neighbour, one neighbour after the other -- the kernel waited 76 % of its wave time); the sums keep the list order
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        unsigned bits = w[u];
        while (bits) {
            int t[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                t[v] = -1;
                if (bits) { t[v] = 32 * u + __ffs((int)bits) - 1; bits &= bits - 1u; }
            }
            int j[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) j[v] = nbr_idx[(int64_t)qi * K + (t[v] >= 0 ? t[v] : 0)];
            float4 p[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) p[v] = pts[j[v]];
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                if (t[v] < 0) continue;
                const double x = p[v].x, y = p[v].y, z = p[v].z;
                c[0] += x; c[1] += y; c[2] += z;
                c[3] += x * x; c[4] += x * y; c[5] += x * z; c[6] += y * y; c[7] += y * z; c[8] += z * z;
                ++k;
            }
        }
    }
    normal_from_moments(c, k, qi, normals);
}

// SPFH histograms from stored neighbour lists (after the fused search above has written lists and normals): wave per point.
// FAST: the bins of a pair come from pair_bins_f32; the pairs it cannot decide are collected per point and appended, with ONE atomic per
// point that has any, to one of SPFH_NQ queues (consecutive workgroups use different queues: a single counter serialises ~10^6 returning
// atomics per batch at the L2 -- measured, it doubled the stage), then evaluated in fp64 by ibl_spfh_queue_kernel, which adds their three
// counts to the stored byte histograms.
#define SPFH_NQ 256
#define SPFH_QSTRIDE 64                 // ints between two queue counters (256 B: different L2 channels)
template <bool FAST>
__global__ __launch_bounds__(256) void ibl_spfh_lists_kernel(const float4* __restrict__ pts, const float4* __restrict__ normals,
                                                             const int* __restrict__ nbr_idx, const int* __restrict__ nbr_cnt, int K, int n,
                                                             unsigned char* __restrict__ spfh_cnt, int2* __restrict__ queue, int* __restrict__ q_count,
                                                             int q_cap) {
    __shared__ int hists[4][36];
    __shared__ int stash[4][FAST ? 128 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the fp64 form doubles as the fast form's overflow path: launched behind it with the queues' overflow flag (the word after the last
    // counter), it returns at once unless a queue overflowed, and then rewrites every histogram (grid-stride over the points)
    if (!FAST && q_count != nullptr && q_count[SPFH_NQ * SPFH_QSTRIDE] == 0) return;
    int* hist = hists[wave];
  for (int qi = IBL_XCD_BLOCK(blockIdx.x, gridDim.x) * 4 + wave; qi < n; qi += gridDim.x * 4) {
    if (lane < 36) hist[lane] = 0;
    wave_lds_sync();
    const int k = nbr_cnt[qi];
    const float4 q = pts[qi], qn = normals[qi];
    int n_unsure = 0;
    for (int t0 = 0; t0 < k; t0 += 64) {
        const int t = t0 + lane;
        const int jo = t < k ? nbr_idx[(int64_t)qi * K + t] : qi;
        bool unsure = false;
        if (jo != qi) {
            if (FAST) {
                int b0, b1, b2;
                if (pair_bins_f32(q, qn, pts[jo], normals[jo], &b0, &b1, &b2)) {
                    atomicAdd(&hist[b0], 1);
                    atomicAdd(&hist[11 + b1], 1);
                    atomicAdd(&hist[22 + b2], 1);
                } else {
                    unsure = true;
                }
            } else {
                double f[3];
                pair_features_d(q, qn, pts[jo], normals[jo], f);
                atomicAdd(&hist[clamp_bin11((int)f[0])], 1);
                atomicAdd(&hist[11 + clamp_bin11((int)floor(11 * (f[1] + 1.0) * 0.5))], 1);
                atomicAdd(&hist[22 + clamp_bin11((int)floor(11 * (f[2] + 1.0) * 0.5))], 1);
            }
        }
        if (FAST) {
            const unsigned long long m = __ballot(unsure);
            if (unsure) stash[wave][(n_unsure + __popcll(m & ((1ull << lane) - 1ull))) & 127] = jo;      // (K <= 128: ibl_normals_fpfh_fusable)
            n_unsure += __popcll(m);
        }
    }
    wave_lds_sync();
    if (lane < 36) spfh_cnt[(int64_t)qi * 36 + lane] = lane < 33 ? (unsigned char)hist[lane] : (unsigned char)0;
    if (FAST && n_unsure > 0) {
        const int qsel = blockIdx.x & (SPFH_NQ - 1);
        int base = 0;
        if (lane == 0) base = atomicAdd(&q_count[qsel * SPFH_QSTRIDE], n_unsure);
        base = __shfl(base, 0, 64);
        if (base + n_unsure <= q_cap) {
            for (int e = lane; e < n_unsure; e += 64) queue[(int64_t)qsel * q_cap + base + e] = make_int2(qi, stash[wave][e]);
        } else if (lane == 0) {
            q_count[SPFH_NQ * SPFH_QSTRIDE] = 1;           // this queue is full: the gated fp64 launch redoes the batch
        }
    }
    wave_lds_sync();
  }
}

// the undecided pairs of the fast kernel, in fp64: three byte counters of the point's stored histogram go up by one each (a 32-bit atomic on
// the word that holds the byte: a counter never exceeds the 100 neighbours of a point, so no carry crosses into the next byte).
// Grid: SPFH_NQ x 4 workgroups, four per queue.
__global__ __launch_bounds__(256) void ibl_spfh_queue_kernel(const float4* __restrict__ pts, const float4* __restrict__ normals,
                                                             const int2* __restrict__ queue, const int* __restrict__ q_count, int q_cap,
                                                             unsigned char* __restrict__ spfh_cnt) {
    if (q_count[SPFH_NQ * SPFH_QSTRIDE] != 0) return;            // (overflow: everything is redone)
    const int qsel = blockIdx.x & (SPFH_NQ - 1), part = blockIdx.x / SPFH_NQ, parts = gridDim.x / SPFH_NQ;
    const int total = min(q_count[qsel * SPFH_QSTRIDE], q_cap);
    for (int e = part * 256 + threadIdx.x; e < total; e += parts * 256) {
        const int2 pr = queue[(int64_t)qsel * q_cap + e];
        double f[3];
        pair_features_d(pts[pr.x], normals[pr.x], pts[pr.y], normals[pr.y], f);
        const int b[3] = {clamp_bin11((int)f[0]), 11 + clamp_bin11((int)floor(11 * (f[1] + 1.0) * 0.5)), 22 + clamp_bin11((int)floor(11 * (f[2] + 1.0) * 0.5))};
        unsigned* words = reinterpret_cast<unsigned*>(spfh_cnt + (int64_t)pr.x * 36);
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(&words[b[c] >> 2], 1u << (8 * (b[c] & 3)));
    }
}

// normals + FPFH from ONE neighbour search (requires radius_normal <= radius_feature, max_nn_normal <= max_nn_feature and <= NP_MAXK)
// (diag.feat_unfused keeps the two separate searches: the tests compare both)
bool ibl_normals_fpfh_fusable(const ibl_reg_ctx* ctx, double radius_normal, int max_nn_normal, double radius_feature, int max_nn_feature) {
    return !ctx->diag.feat_unfused && radius_normal <= radius_feature && max_nn_normal <= max_nn_feature && max_nn_normal <= NP_MAXK && max_nn_feature <= 128;   // (128-slot mask)
}
int ibl_launch_normals_fpfh(ibl_reg_ctx* ctx, const BatchGrid& g, const float4* pts, const int* seg_off, int n, double radius_normal,
                            int max_nn_normal, double radius_feature, int max_nn_feature, float4* normals, unsigned char* spfh, int* nbr_idx,
                            float* nbr_d2, int* nbr_cnt, float* fpfh, int matching_order, int* status, hipStream_t s) {
    if (n <= 0) return IBL_OK;
    ArenaMark mk(ctx);                  // (the mask is read by the kernel launched below, on the same stream)
    unsigned* nrm_mask;
    IBL_ARENA(nrm_mask, unsigned, 4 * (int64_t)n + 64);
    void* tok;
    ibl_prof_begin(IBL_PROF_SPFH, 156.0 * (double)n, s, &tok);
    const int st = launch_knn(ctx, g, seg_off, n, 0, n, radius_feature, max_nn_feature,
                              ListNormalFactory{nrm_mask, nbr_idx, nbr_d2, nbr_cnt, max_nn_feature, (float)(radius_normal * radius_normal), max_nn_normal},
                              status, s);
    ibl_prof_end(tok, s);
    if (st) return st;
    hipLaunchKernelGGL(ibl_normals_from_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pts, nbr_idx, max_nn_feature, nrm_mask, n, normals);
    IBL_LAUNCH_CHECK();
    {
        // fp32 bins + fp64 for the pairs next to a bin boundary (pair_bins_f32); the SPFH_NQ queues together hold 1 / 16 of all pairs
        // (measured: 0.8 % are undecided) -- a batch that overflows one is redone in fp64 by the gated third launch; diag.spfh_f64 runs
        // every pair in fp64 (the tests compare both), diag.spfh_qcap = <entries per queue> shrinks the queues (the overflow test)
        if (!ctx->diag.spfh_f64) {
            int64_t cap64 = std::min<int64_t>((int64_t)n * max_nn_feature / (16 * SPFH_NQ) + 256, (int64_t)1 << 20);
            if (ctx->diag.spfh_qcap) cap64 = ctx->diag.spfh_qcap;
            int2* queue; int* q_count;
            IBL_ARENA(queue, int2, cap64 * SPFH_NQ);
            IBL_ARENA(q_count, int, SPFH_NQ * SPFH_QSTRIDE + 64);
            IBL_HIP_CHECK(hipMemsetAsync(q_count, 0, sizeof(int) * (SPFH_NQ * SPFH_QSTRIDE + 1), s));
            hipLaunchKernelGGL(ibl_spfh_lists_kernel<true>, dim3((n + 3) / 4), dim3(256), 0, s, pts, normals, nbr_idx, nbr_cnt, max_nn_feature, n, spfh,
                               queue, q_count, (int)cap64);
            IBL_LAUNCH_CHECK();
            hipLaunchKernelGGL(ibl_spfh_queue_kernel, dim3(SPFH_NQ * 4), dim3(256), 0, s, pts, normals, queue, q_count, (int)cap64, spfh);
            IBL_LAUNCH_CHECK();
            hipLaunchKernelGGL(ibl_spfh_lists_kernel<false>, dim3(2048), dim3(256), 0, s, pts, normals, nbr_idx, nbr_cnt, max_nn_feature, n, spfh,
                               (int2*)nullptr, q_count, (int)cap64);
            IBL_LAUNCH_CHECK();
            if (ctx->diag.spfh_stats) {              // diagnostics: undecided pairs of this batch (synchronises)
                std::vector<int> cnt(SPFH_NQ * SPFH_QSTRIDE + 1);
                IBL_HIP_CHECK(hipMemcpyAsync(cnt.data(), q_count, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost, s));
                IBL_HIP_CHECK(hipStreamSynchronize(s));
                long long tot = 0; int mx = 0;
                for (int i = 0; i < SPFH_NQ; ++i) { tot += cnt[i * SPFH_QSTRIDE]; mx = std::max(mx, cnt[i * SPFH_QSTRIDE]); }
                fprintf(stderr, "[ibloc] spfh: %lld undecided pairs of at most %lld; fullest queue %d of %lld; overflow %d\n", tot,
                        (long long)n * max_nn_feature, mx, (long long)cap64, cnt.back());
            }
        } else {
            hipLaunchKernelGGL(ibl_spfh_lists_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, s, pts, normals, nbr_idx, nbr_cnt, max_nn_feature, n, spfh,
                               (int2*)nullptr, (int*)nullptr, 0);
            IBL_LAUNCH_CHECK();
        }
    }
    if (fpfh) {
        hipLaunchKernelGGL(ibl_fpfh_kernel, dim3((n + FPFH_Q - 1) / FPFH_Q), dim3(256), 0, s, spfh, nbr_idx, nbr_d2, nbr_cnt, max_nn_feature, n, matching_order, fpfh);
        IBL_LAUNCH_CHECK();
    }
    return IBL_OK;
}
