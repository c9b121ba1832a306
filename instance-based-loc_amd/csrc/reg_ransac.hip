// reg_ransac.hip -- RANSAC stage of a registration pass: transform hypotheses from the feature correspondences.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once, the RANSAC loop of
//   utils/fpfh_register.py:100-143            register_point_clouds (Open3D RegistrationRANSACBasedOnFeatureMatching)
// RANSAC follows the index-ordered, Philox-driven semantics of oracle/oracle_reg.c (Open3D's own loop is
// unseeded and OpenMP-racy): hypotheses are generated and scored in parallel rounds, then folded by a
// sequential scan that reproduces the "better result / confidence-based early exit" bookkeeping exactly.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_stages.h"

// ------------------------------------------------------------------------------------------------
// RANSAC
//
// Rounds of up to RANSAC_MAX_ROUND hypotheses per job.  Per round:
//   flag    thread per hypothesis: Philox draw, edge-length check, 3-point Kabsch, distance check -> 1 byte,
//           plus the count of survivors of every 256-hypothesis block
//   scan    exclusive sum of the block counts (hipcub) -> ordered offsets
//   scatter ordered list of surviving (job, hypothesis) ids
//   score   thread per survivor: its transform (once); then one wavefront per survivor: validate it on the correspondence set
//   fold    one wavefront per job: walk the survivors in hypothesis order and reproduce the sequential
//           "better result -> tighten est_k" bookkeeping of the reference loop exactly
// Correspondences are packed as (source xyz, target xyz) pairs so that a draw costs two 16-byte loads.
// ------------------------------------------------------------------------------------------------
#define RANSAC_MAX_ROUND 262144
#define RANSAC_FIRST_ROUND 4096
#ifndef RANSAC_WIDE_MIN_BLOCKS
#define RANSAC_WIDE_MIN_BLOCKS 1024       // fewer 16 k-hypothesis blocks than this in a round: 4 k blocks instead (run_round)
#endif
#define RANSAC_TAIL_JOBS 8                 // with at most this many jobs left ...
#define RANSAC_TAIL_ROUND (1 << 20)        // ... a round walks this many hypotheses per job

__global__ void ibl_ransac_init_kernel(RansacState* __restrict__ st, const int* __restrict__ n_corr, int J, long long max_iter,
                                       double max_dist, int* __restrict__ active, unsigned job_id_base,
                                       const unsigned* __restrict__ job_ids) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    RansacState s;
    for (int i = 0; i < 16; ++i) s.best_T[i] = (i % 5) == 0 ? 1.0 : 0.0;
    s.best_fit = 0; s.best_rmse = 0; s.est_k = max_iter; s.next_i = 0; s.walked = 0; s.validated = 0; s.best_inl = 0; s.last_update = -1;
    s.done = (n_corr[j] < 3 || max_dist <= 0) ? 1 : 0;
    s.job_id = job_ids ? job_ids[j] : job_id_base + (unsigned)j;
    s.pad_ = 0;
    st[j] = s;
    active[j] = j;           // the first rounds run every job slot (a finished job's blocks leave at once); the host compacts later
}

// done flags for the host's read-back between groups of rounds
__global__ void ibl_ransac_done_kernel(const RansacState* __restrict__ st, int J, int* __restrict__ done) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < J) done[j] = st[j].done;
}

// packed correspondences: cp[2c] = source point, cp[2c + 1] = target point
__global__ __launch_bounds__(256) void ibl_pack_corr_kernel(const float4* __restrict__ pts, const int* __restrict__ job_off, int J,
                                                            const int2* __restrict__ corr, const int* __restrict__ n_corr,
                                                            float4* __restrict__ cp) {
    const int j = blockIdx.y;
    const int sb = job_off[j], tb = job_off[J + j], nc = n_corr[j];
    for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += gridDim.x * 256) {
        const int2 cc = corr[sb + c];
        cp[2 * (int64_t)(sb + c)] = pts[sb + cc.x];
        cp[2 * (int64_t)(sb + c) + 1] = pts[tb + cc.y];
    }
}

// hypothesis i: Philox draw of three packed correspondences
__device__ __forceinline__ void ransac_draw(long long i, unsigned job_id, unsigned seed_lo, unsigned seed_hi, const float4* __restrict__ cp,
                                            int nc, double* s, double* d) {
    unsigned r[4];
    philox4x32((unsigned)i, job_id, (unsigned)((unsigned long long)i >> 32), 0u, seed_lo, seed_hi, r);
    for (int t = 0; t < 3; ++t) {
        const int pick = (int)(((unsigned long long)r[t] * (unsigned long long)nc) >> 32);
        const float4 ps = cp[2 * pick], pd = cp[2 * pick + 1];
        s[3 * t] = ps.x; s[3 * t + 1] = ps.y; s[3 * t + 2] = ps.z;
        d[3 * t] = pd.x; d[3 * t + 1] = pd.y; d[3 * t + 2] = pd.z;
    }
}

// CorrespondenceCheckerBasedOnEdgeLength
__device__ __forceinline__ bool ransac_edge_ok(const double* s, const double* d, double edge_sim) {
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) {
            const double ds = sqrt((s[3 * a] - s[3 * b]) * (s[3 * a] - s[3 * b]) + (s[3 * a + 1] - s[3 * b + 1]) * (s[3 * a + 1] - s[3 * b + 1]) +
                                   (s[3 * a + 2] - s[3 * b + 2]) * (s[3 * a + 2] - s[3 * b + 2]));
            const double dt = sqrt((d[3 * a] - d[3 * b]) * (d[3 * a] - d[3 * b]) + (d[3 * a + 1] - d[3 * b + 1]) * (d[3 * a + 1] - d[3 * b + 1]) +
                                   (d[3 * a + 2] - d[3 * b + 2]) * (d[3 * a + 2] - d[3 * b + 2]));
            if (ds < dt * edge_sim || dt < ds * edge_sim) return false;
        }
    return true;
}

// The same check for the flag kernel's first pass (every hypothesis, ~99 % rejected): squared edge lengths in fp32 against
// edge_sim^2 with a 3e-6 guard band (the fp32 ratio is good to ~5e-7), no square roots.  Only a hypothesis with an edge
// ratio inside the band -- or a zero-length edge -- falls back to the exact double-precision form above, so the verdict
// is always the exact one.
__device__ __forceinline__ bool ransac_edge_ok_draw(long long i, unsigned job_id, unsigned seed_lo, unsigned seed_hi,
                                                    const float4* __restrict__ cp, int nc, double edge_sim, float e2_lo, float e2_hi) {
    unsigned r[4];
    philox4x32((unsigned)i, job_id, (unsigned)((unsigned long long)i >> 32), 0u, seed_lo, seed_hi, r);
    float4 ps[3], pd[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int pick = (int)(((unsigned long long)r[t] * (unsigned long long)nc) >> 32);
        ps[t] = cp[2 * pick]; pd[t] = cp[2 * pick + 1];
    }
    bool borderline = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a + 1; b < 3; ++b) {
            const float sx = ps[a].x - ps[b].x, sy = ps[a].y - ps[b].y, sz = ps[a].z - ps[b].z;
            const float tx = pd[a].x - pd[b].x, ty = pd[a].y - pd[b].y, tz = pd[a].z - pd[b].z;
            const float ds2 = sx * sx + sy * sy + sz * sz, dt2 = tx * tx + ty * ty + tz * tz;
            if (ds2 < dt2 * e2_lo || dt2 < ds2 * e2_lo) return false;
            if (!(ds2 > dt2 * e2_hi && dt2 > ds2 * e2_hi)) borderline = true;
        }
    if (!borderline) return true;
    double s[9], d[9];
    for (int t = 0; t < 3; ++t) {
        s[3 * t] = ps[t].x; s[3 * t + 1] = ps[t].y; s[3 * t + 2] = ps[t].z;
        d[3 * t] = pd[t].x; d[3 * t + 1] = pd[t].y; d[3 * t + 2] = pd[t].z;
    }
    return ransac_edge_ok(s, d, edge_sim);
}

// 3-point Kabsch + CorrespondenceCheckerBasedOnDistance
__device__ inline bool ransac_fit_ok(const double* s, const double* d, double max_dist, double* T) {
    double sm[3] = {0, 0, 0}, dm[3] = {0, 0, 0};
    for (int t = 0; t < 3; ++t) for (int a = 0; a < 3; ++a) { sm[a] += s[3 * t + a]; dm[a] += d[3 * t + a]; }
    for (int a = 0; a < 3; ++a) { sm[a] /= 3; dm[a] /= 3; }
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int t = 0; t < 3; ++t)
        for (int rr = 0; rr < 3; ++rr) for (int cc = 0; cc < 3; ++cc) H[rr][cc] += (d[3 * t + rr] - dm[rr]) * (s[3 * t + cc] - sm[cc]);
    kabsch_from_moments(sm, dm, H, T);
    for (int t = 0; t < 3; ++t) {
        double p[3];
        xform_d(T, s[3 * t], s[3 * t + 1], s[3 * t + 2], p);
        const double dx = p[0] - d[3 * t], dy = p[1] - d[3 * t + 1], dz = p[2] - d[3 * t + 2];
        if (sqrt(dx * dx + dy * dy + dz * dz) > max_dist) return false;
    }
    return true;
}

__device__ inline bool ransac_hypothesis(long long i, unsigned job_id, unsigned seed_lo, unsigned seed_hi, const float4* __restrict__ cp,
                                         int nc, double max_dist, double edge_sim, double* T) {
    double s[9], d[9];
    ransac_draw(i, job_id, seed_lo, seed_hi, cp, nc, s, d);
    if (!ransac_edge_ok(s, d, edge_sim)) return false;
    return ransac_fit_ok(s, d, max_dist, T);
}

// grid (round / (1024 RANSAC_SUBS), active jobs): each block walks 1024 RANSAC_SUBS consecutive hypotheses.  The cheap part (draw + edge-length
// check, ~99 % rejected) runs on every lane; the survivors of the whole chunk are compacted through LDS so that the
// expensive part (fp64 Kabsch + distance check) runs once, on densely packed lanes.  `flags` is zeroed by the host before the launch.
constexpr int RANSAC_LDS_CORR = 1024;    // correspondences staged in LDS (32 KiB)
// Blocks of the well-filled rounds (run_round): 8 k hypotheses.  16 k amortise the dense Kabsch pass over more survivors, but their 32 KB
// survivor table + the 32 KB of staged correspondences leave two workgroups per CU; 8 k blocks (48 KB, registers bound to 168) run three:
// 653 -> 554 us for the 262 144-hypothesis round of a bench step.
#ifndef RANSAC_BIG_SUBS
#define RANSAC_BIG_SUBS 8
#endif
#ifndef RANSAC_BIG_OCC
#define RANSAC_BIG_OCC 3                 // its workgroups per CU the registers must allow
#endif
template <int RANSAC_SUBS>               // 1024-hypothesis passes per block (one Kabsch pass over all their survivors)
__global__ __launch_bounds__(256, RANSAC_SUBS == RANSAC_BIG_SUBS ? RANSAC_BIG_OCC : 1) void ibl_ransac_flag_kernel(const RansacState* __restrict__ st, const float4* __restrict__ cp,
                                                              const int* __restrict__ job_off, const int* __restrict__ n_corr,
                                                              long long max_iter, double max_dist, double edge_sim, unsigned seed_lo,
                                                              unsigned seed_hi, unsigned job_id_base, int round_size,
                                                              unsigned char* __restrict__ flags /* [J][round] */,
                                                              int* __restrict__ blk_cnt /* [J][round/256] */,
                                                              const int* __restrict__ active /* job ids still running */) {
    constexpr int RANSAC_CHUNK = 1024 * RANSAC_SUBS;
    const int a = blockIdx.y, j = active[a];        // per-round tables are indexed by the job's slot in the active list
    const int nblk = round_size / 256;
    const RansacState& S = st[j];
    const long long next_i = S.next_i, est_k = S.est_k;
    const bool job_on = !S.done;
    const float4* c = cp + 2 * (int64_t)job_off[j];
    const int nc = n_corr[j];
    const unsigned job_id = S.job_id;
    __shared__ unsigned short surv[RANSAC_CHUNK];     // slot within the chunk
    __shared__ int nsurv;
    __shared__ int cnt16[4 * RANSAC_SUBS];
    // The packed correspondences of the job (32 B each) are drawn 3 at a time by every hypothesis: random 16-byte gathers that sat on
    // L2 latency with two waves per SIMD to hide it.  Up to RANSAC_LDS_CORR of them are staged in LDS once per block (a block draws
    // from them 6 x 4096 ... 16384 times); larger jobs keep reading global memory.  Same values either way.
    __shared__ float4 sc[2 * RANSAC_LDS_CORR];
    if (!job_on) {            // uniform per block: nothing survives, the counts of this block's 256-hypothesis groups are zero
        if (threadIdx.x < 4 * RANSAC_SUBS) blk_cnt[a * nblk + blockIdx.x * (4 * RANSAC_SUBS) + threadIdx.x] = 0;
        return;
    }
    const bool in_lds = nc <= RANSAC_LDS_CORR;
    if (in_lds && job_on)
        for (int t = threadIdx.x; t < 2 * nc; t += 256) sc[t] = c[t];
    if (threadIdx.x < 4 * RANSAC_SUBS) cnt16[threadIdx.x] = 0;
    if (threadIdx.x == 0) nsurv = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const float e2 = (float)(edge_sim * edge_sim), e2_lo = e2 * (1.0f - 3e-6f), e2_hi = e2 * (1.0f + 3e-6f);
    for (int r = 0; r < 4 * RANSAC_SUBS; ++r) {
        const int slot = blockIdx.x * RANSAC_CHUNK + r * 256 + threadIdx.x;
        const long long i = next_i + slot;
        bool ok = false;
        if (job_on && i < est_k && i < max_iter)
            ok = in_lds ? ransac_edge_ok_draw(i, job_id, seed_lo, seed_hi, sc, nc, edge_sim, e2_lo, e2_hi)
                        : ransac_edge_ok_draw(i, job_id, seed_lo, seed_hi, c, nc, edge_sim, e2_lo, e2_hi);
        const unsigned long long m = __ballot(ok);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(&nsurv, __popcll(m));
        base = __shfl(base, 0, 64);
        if (ok) surv[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(r * 256 + threadIdx.x);
    }
    __syncthreads();
    // the survivors of the whole chunk (~1 %) go through the fp64 Kabsch together: a single, densely packed pass
    const int ns = nsurv;
    for (int t = threadIdx.x; t < ns; t += 256) {
        const int slot = blockIdx.x * RANSAC_CHUNK + (int)surv[t];
        double sp[9], dp[9], T[16];
        if (in_lds) ransac_draw(next_i + slot, job_id, seed_lo, seed_hi, sc, nc, sp, dp);
        else ransac_draw(next_i + slot, job_id, seed_lo, seed_hi, c, nc, sp, dp);
        if (ransac_fit_ok(sp, dp, max_dist, T)) {
            flags[(int64_t)a * round_size + slot] = 1;
            atomicAdd(&cnt16[(slot - blockIdx.x * RANSAC_CHUNK) >> 8], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 * RANSAC_SUBS) blk_cnt[a * nblk + blockIdx.x * (4 * RANSAC_SUBS) + threadIdx.x] = cnt16[threadIdx.x];
}

__global__ __launch_bounds__(256) void ibl_ransac_scatter_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ blk_off,
                                                                 int round_size, int* __restrict__ list /* slot ids, ordered */, int list_cap) {
    const int a = blockIdx.y;
    const int nblk = round_size / 256;
    const int slot = blockIdx.x * 256 + threadIdx.x;
    const bool ok = flags[(int64_t)a * round_size + slot] != 0;
    __shared__ int wc[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wc[wave] = __popcll(m);
    __syncthreads();
    if (ok) {
        int pre = blk_off[a * nblk + blockIdx.x];
        for (int w = 0; w < wave; ++w) pre += wc[w];
        const int pos = pre + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < list_cap) list[pos] = slot;              // an overflowing round is reported by the transform kernel
    }
}

// thread per survivor e in [0, total): its transform, once (job = the active slot whose offset range contains e)
__global__ __launch_bounds__(256) void ibl_ransac_transform_kernel(const RansacState* __restrict__ st, const float4* __restrict__ cp,
                                                                   const int* __restrict__ job_off, const int* __restrict__ n_corr,
                                                                   const int* __restrict__ active, int n_active, double max_dist, double edge_sim,
                                                                   unsigned seed_lo, unsigned seed_hi, unsigned job_id_base, int round_size,
                                                                   const int* __restrict__ blk_off, const int* __restrict__ list,
                                                                   const int* __restrict__ total_ptr, int list_cap, int* __restrict__ status,
                                                                   int* __restrict__ e_job, double* __restrict__ e_T) {
    int total = *total_ptr;                    // the round's survivors: the last entry of the block-count scan
    if (total > list_cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, IBL_ST_RANSAC_OVERFLOW);
        total = list_cap;
    }
    const int nblk = round_size / 256;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    int lo = 0, hi = n_active;                // largest active slot a with blk_off[a * nblk] <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk_off[mid * nblk] <= e) lo = mid; else hi = mid;
    }
    const int j = active[lo];
    const long long i = st[j].next_i + list[e];
    double T[16];
    ransac_hypothesis(i, st[j].job_id, seed_lo, seed_hi, cp + 2 * (int64_t)job_off[j], n_corr[j], max_dist, edge_sim, T);
    e_job[e] = j;
#pragma unroll
    for (int t = 0; t < 12; ++t) e_T[(int64_t)e * 12 + t] = T[t];
    }
}

// wave per survivor: inliers and squared error of its transform over the job's correspondences
__global__ __launch_bounds__(256) void ibl_ransac_score_kernel(const float4* __restrict__ cp, const int* __restrict__ job_off,
                                                               const int* __restrict__ n_corr, double max_dist,
                                                               const int* __restrict__ total_ptr, int list_cap,
                                                               const int* __restrict__ e_job, const double* __restrict__ e_T,
                                                               int* __restrict__ e_inl, double* __restrict__ e_err2) {
    const int total = min(*total_ptr, list_cap);
    const int lane = threadIdx.x & 63;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < total; e += gridDim.x * 4) {
    const int j = e_job[e];
    const float4* c = cp + 2 * (int64_t)job_off[j];
    const int nc = n_corr[j];
    double T[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) T[t] = e_T[(int64_t)e * 12 + t];
    int inl = 0;
    double err2 = 0;
    const double md2_hi = max_dist * max_dist * (1.0 + 1e-12);      // d2 >= this => sqrt(d2) >= max_dist for certain
    for (int k = lane; k < nc; k += 64) {
        const float4 ps = c[2 * k], q = c[2 * k + 1];
        double p[3];
        xform_d(T, ps.x, ps.y, ps.z, p);
        const double dx = p[0] - q.x, dy = p[1] - q.y, dz = p[2] - q.z;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 < md2_hi) {          // most correspondences of most hypotheses are far outliers: no square root for them
            const double dd = sqrt(d2);
            if (dd < max_dist) { ++inl; err2 += dd * dd; }
        }
    }
    inl = wave_sum_i(inl);
    err2 = wave_sum_d(err2);
    if (lane == 0) { e_inl[e] = inl; e_err2[e] = err2; }
    }
}

// wave per job: fold the round's survivors in hypothesis order
__global__ __launch_bounds__(64) void ibl_ransac_fold_kernel(RansacState* __restrict__ st, int J, const int* __restrict__ n_corr,
                                                             long long max_iter, double confidence, int round_size,
                                                             const int* __restrict__ blk_off, const int* __restrict__ list,
                                                             const int* __restrict__ e_inl, const double* __restrict__ e_err2,
                                                             const double* __restrict__ e_T, const int* __restrict__ active) {
    const int a = blockIdx.x, j = active[a];
    const int lane = threadIdx.x;
    RansacState S = st[j];
    if (S.done) return;
    const int nblk = round_size / 256;
    const int b = blk_off[a * nblk], e = blk_off[(a + 1) * nblk];      // the scan has one entry past the last slot (= total)
    const int nc = n_corr[j];
    bool stop = false;
    long long n_before_stop = 0;          // survivors with index < the stopping index in this round
    for (int c0 = b; c0 < e && !stop; c0 += 64) {
        const int k = c0 + lane;
        const bool v = k < e;
        const int inl = v ? e_inl[k] : -1;
        const long long idx = v ? S.next_i + list[k] : 0x7FFFFFFFFFFFFFFFll;
        unsigned long long cand = __ballot(v && inl > 0 && inl >= S.best_inl);
        while (cand) {
            const int t = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const long long ci = __shfl(idx, t, 64);
            if (ci >= S.est_k) { stop = true; break; }
            const int cinl = __shfl(inl, t, 64);
            if (cinl < S.best_inl) continue;                    // best_inl may have grown inside this chunk
            const double cerr2 = e_err2[c0 + t];
            const double fit = (double)cinl / (double)nc, rmse = sqrt(cerr2 / cinl);
            if (fit > S.best_fit || (fit == S.best_fit && rmse < S.best_rmse)) {
                S.best_fit = fit; S.best_rmse = rmse; S.best_inl = cinl; S.last_update = ci;
                if (lane < 12) S.best_T[lane] = e_T[(int64_t)(c0 + t) * 12 + lane];
                if (confidence > 0.0) {          // (<= 0: fixed budget, IBL_REG_FIXED_BUDGET)
                    const double ek = log(1.0 - confidence) / log(1.0 - pow(fit, 3.0));
                    if (ek < (double)S.est_k) S.est_k = (long long)ceil(ek);
                }
            }
        }
        // survivors of this chunk that the reference loop walks: it stands at max(last update + 1, est_k)
        long long lim = S.last_update + 1 > S.est_k ? S.last_update + 1 : S.est_k;
        if (lim > max_iter) lim = max_iter;
        n_before_stop += __popcll(__ballot(v && idx < lim));
        if (!stop) { const unsigned long long beyond = __ballot(v && idx >= lim); if (beyond) stop = true; }
    }
    const long long end = S.next_i + round_size;
    const long long lim = S.est_k < max_iter ? S.est_k : max_iter;
    S.validated += n_before_stop;
    S.next_i = end;
    if (stop || end >= lim) {
        S.done = 1;
        long long w = S.last_update + 1 > lim ? S.last_update + 1 : lim;   // the reference loop stands at max(i0 + 1, est_k)
        if (w > max_iter) w = max_iter;
        S.walked = w;
    } else {
        S.walked = end;
    }
    // best_T lanes 0..11 were written by the owning lanes: gather them to lane 0's copy
    double bt = lane < 12 ? S.best_T[lane] : 0.0;
    for (int t = 0; t < 12; ++t) { const double v = __shfl(bt, t, 64); if (lane == 0) S.best_T[t] = v; }
    if (lane == 0) st[j] = S;
}

// ------------------------------------------------------------------------------------------------
// the round scheduler
// ------------------------------------------------------------------------------------------------
// per-round tables; they hold (active jobs) x (round size) hypotheses
struct RansacScratch {
    float4* cp;                    // packed correspondences
    unsigned char* hyp_flags;      // [active][round]: the hypothesis passed both checkers
    int *blk_cnt, *blk_off;        // survivors per 256-hypothesis block and their exclusive scan
    int* list; int list_cap;       // ordered survivor slots of the round
    int *e_inl, *e_job; double *e_err2, *e_T;       // per survivor
    unsigned char* tmp; size_t tmp_bytes;           // hipcub scan
    int* active;                   // job ids still running
    double max_dist;
};

static int ransac_round(ibl_reg_ctx* ctx, const RegPass& ps, const RansacScratch& r, int n_act, int round_size) {
    const RegCall& c = *ps.call;
    hipStream_t s = ps.s;
    const unsigned seed_lo = (unsigned)c.params.seed, seed_hi = (unsigned)(c.params.seed >> 32);
    const long long max_iter = (long long)c.params.ransac_max_iter;
    const int nblk = round_size / 256;
    const int n_tab = n_act * nblk;           // tables are indexed by (slot in the active list, block)
    IBL_HIP_CHECK(hipMemsetAsync(r.hyp_flags, 0, (size_t)n_act * round_size, s));
    // large blocks amortise the dense Kabsch pass best, but a round of few jobs (or the 32 k round of all of them) is a few
    // hundred of them -- under two per CU, each ~120 us long: those rounds run as 4 k blocks (same flags: a hypothesis does not
    // know its block)
    constexpr int BIG = 1024 * RANSAC_BIG_SUBS;
    if (round_size >= BIG && (int64_t)(round_size / 16384) * n_act >= RANSAC_WIDE_MIN_BLOCKS)
        hipLaunchKernelGGL(ibl_ransac_flag_kernel<RANSAC_BIG_SUBS>, dim3(round_size / BIG, n_act), dim3(256), 0, s, ps.rs, r.cp, ps.d_job_off, ps.n_corr,
                           max_iter, r.max_dist, 0.9, seed_lo, seed_hi, c.params.job_id_base, round_size, r.hyp_flags, r.blk_cnt, r.active);
    else
        hipLaunchKernelGGL(ibl_ransac_flag_kernel<4>, dim3(round_size / 4096, n_act), dim3(256), 0, s, ps.rs, r.cp, ps.d_job_off, ps.n_corr,
                           max_iter, r.max_dist, 0.9, seed_lo, seed_hi, c.params.job_id_base, round_size, r.hyp_flags, r.blk_cnt, r.active);
    IBL_LAUNCH_CHECK();
    IBL_HIP_CHECK(hipMemsetAsync(r.blk_cnt + n_tab, 0, sizeof(int), s));
    size_t tmp_bytes = r.tmp_bytes;
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(r.tmp, tmp_bytes, r.blk_cnt, r.blk_off, n_tab + 1, s));
    const int* total_ptr = r.blk_off + n_tab;
    hipLaunchKernelGGL(ibl_ransac_scatter_kernel, dim3(nblk, n_act), dim3(256), 0, s, r.hyp_flags, r.blk_off, round_size, r.list, r.list_cap);
    IBL_LAUNCH_CHECK();
    const int sweep = (int)std::min<int64_t>(2048, ((int64_t)r.list_cap + 255) / 256);
    hipLaunchKernelGGL(ibl_ransac_transform_kernel, dim3(sweep), dim3(256), 0, s, ps.rs, r.cp, ps.d_job_off, ps.n_corr, r.active, n_act, r.max_dist, 0.9,
                       seed_lo, seed_hi, c.params.job_id_base, round_size, r.blk_off, r.list, total_ptr, r.list_cap, ctx->d_status, r.e_job, r.e_T);
    IBL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ibl_ransac_score_kernel, dim3(4096), dim3(256), 0, s, r.cp, ps.d_job_off, ps.n_corr, r.max_dist, total_ptr, r.list_cap, r.e_job,
                       r.e_T, r.e_inl, r.e_err2);
    IBL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ibl_ransac_fold_kernel, dim3(n_act), dim3(64), 0, s, ps.rs, ps.J, ps.n_corr, max_iter,
                       (c.params.flags & IBL_REG_FIXED_BUDGET) ? -1.0 : 0.99, round_size, r.blk_off, r.list, r.e_inl, r.e_err2, r.e_T, r.active);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}

// Rounds are enqueued without asking the device anything: every per-round kernel finds the round's survivor count in
// device memory (the last entry of the block-count scan), and the blocks of a job that has met its confidence bound
// leave at once.  The host only looks between GROUPS of rounds -- after the first three (4 k + 32 k + 256 k hypotheses,
// where most jobs stop) and then after every two -- to compact the list of running jobs and to stop.
static int ransac_schedule(ibl_reg_ctx* ctx, const RegPass& ps, const RansacScratch& r, int* done_flags) {
    const int J = ps.J;
    const int64_t ransac_max_iter = ps.call->params.ransac_max_iter;
    hipStream_t s = ps.s;
    const int max_round = RANSAC_MAX_ROUND;
    std::vector<int> h_done(J, 0), h_list;
    long long walked = 0;
    int round_size = RANSAC_FIRST_ROUND;
    int n_act = J;
    int group = 3;
    while (walked < ransac_max_iter && n_act > 0) {
        for (int k = 0; k < group && walked < ransac_max_iter; ++k) {
            if (n_act <= RANSAC_TAIL_JOBS && round_size == max_round) round_size = RANSAC_TAIL_ROUND;
            const int st = ransac_round(ctx, ps, r, n_act, round_size);
            if (st) return st;
            walked += round_size;
            if (round_size < max_round) round_size = std::min(max_round, round_size * 8);
        }
        if (walked >= ransac_max_iter) break;
        hipLaunchKernelGGL(ibl_ransac_done_kernel, dim3((J + 63) / 64), dim3(64), 0, s, ps.rs, J, done_flags);
        IBL_LAUNCH_CHECK();
        IBL_HIP_CHECK(hipMemcpyAsync(h_done.data(), done_flags, sizeof(int) * J, hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipStreamSynchronize(s));
        h_list.clear();
        for (int j = 0; j < J; ++j) if (!h_done[j]) h_list.push_back(j);
        n_act = (int)h_list.size();
        if (n_act > 0) {
            const int st = ibl_stage_upload(ctx, r.active, h_list.data(), sizeof(int) * (int64_t)n_act, s);
            if (st) return st;
        }
        group = n_act <= RANSAC_TAIL_JOBS ? 1 : 2;
    }
    return IBL_OK;
}

int ibl_reg_ransac_stage(ibl_reg_ctx* ctx, RegPass& ps) {
    const RegCall& c = *ps.call;
    const int J = ps.J;
    hipStream_t s = ps.s;
    ArenaMark m3(ctx);
    ibl_prof_begin(IBL_PROF_ST_RANSAC, 0.0, s, &ps.tok_ransac);
    RansacScratch r = {};
    r.max_dist = c.params.voxel_size * c.params.global_dist_factor;
    // a round's tables hold (active jobs) x (round size) hypotheses; when only a few jobs are left (wrong assignments
    // that never reach the confidence exit walk all 4 M), rounds grow to RANSAC_TAIL_ROUND so that they still fill the GPU
    const int64_t cap_slots = std::max<int64_t>((int64_t)J * RANSAC_MAX_ROUND, (int64_t)RANSAC_TAIL_JOBS * RANSAC_TAIL_ROUND);
    const int64_t cap_blk = cap_slots / 256;
    IBL_ARENA(r.cp, float4, 2 * (int64_t)ps.Ns + 2);
    IBL_ARENA(r.hyp_flags, unsigned char, cap_slots);
    IBL_ARENA(r.blk_cnt, int, cap_blk + 1);
    IBL_ARENA(r.blk_off, int, cap_blk + 1);
    // survivors of the edge-length test of one round: ~1 % of the hypotheses on real clouds; a batch whose round exceeds the list is
    // redone once with a list that holds every hypothesis (RegPassOpts::ransac_full_list)
    r.list_cap = (int)std::min<int64_t>(ps.opt.ransac_full_list ? cap_slots + 65536 : cap_slots / 16 + 65536, (int64_t)1 << 27);
    IBL_ARENA(r.list, int, r.list_cap);
    IBL_ARENA(r.e_inl, int, r.list_cap);
    IBL_ARENA(r.e_job, int, r.list_cap);
    IBL_ARENA(r.e_err2, double, r.list_cap);
    IBL_ARENA(r.e_T, double, (int64_t)r.list_cap * 12);
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, r.tmp_bytes, r.blk_cnt, r.blk_off, (int)(cap_blk + 1), s));
    IBL_ARENA(r.tmp, unsigned char, (int64_t)r.tmp_bytes + 256);
    hipLaunchKernelGGL(ibl_pack_corr_kernel, dim3(16, J), dim3(256), 0, s, ps.P, ps.d_job_off, J, ps.corr, ps.n_corr, r.cp);
    IBL_LAUNCH_CHECK();
    int* done_flags;
    IBL_ARENA(r.active, int, J + 1);
    IBL_ARENA(done_flags, int, J + 1);
    unsigned* d_job_ids = nullptr;
    if (c.job_ids) {
        IBL_ARENA(d_job_ids, unsigned, J + 1);
        const int st = ibl_stage_upload(ctx, d_job_ids, c.job_ids, sizeof(unsigned) * (int64_t)J, s);
        if (st) return st;
    }
    hipLaunchKernelGGL(ibl_ransac_init_kernel, dim3((J + 63) / 64), dim3(64), 0, s, ps.rs, ps.n_corr, J, (long long)c.params.ransac_max_iter, r.max_dist,
                       r.active, c.params.job_id_base, d_job_ids);
    IBL_LAUNCH_CHECK();
    return ransac_schedule(ctx, ps, r, done_flags);
}
