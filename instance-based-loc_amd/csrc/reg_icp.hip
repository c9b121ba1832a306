// reg_icp.hip -- ICP stage of a registration pass: coloured ICP from the RANSAC transforms, point-to-point ICP from the identity
// for clouds without colours.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once, the refinement of
//   utils/fpfh_register.py:100-143            register_point_clouds (Open3D registration_colored_icp, p2p fallback)
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_stages.h"

// ICP iteration from which a source point is searched by 8 lanes (ibl_icp_nn_group_kernel).  Measured per-launch times of the T
// workload (us): thread per point 446 376 351 347 342 324 229 136 115 100 ... 85 (floor); eight lanes 411 186 106 80 65 ... 41 (floor)
#ifndef ICP_GROUP_FROM
#define ICP_GROUP_FROM 8
#endif
// (32 lanes per point from iteration 11 on measured 100 us per launch: the grid of 32x the blocks, nearly all of finished jobs, costs
// more to schedule than the shorter walk saves)
#ifndef ICP_LPQ
#define ICP_LPQ 8            // lanes per source point of ibl_icp_nn_group_kernel
#endif
#define ICP_ACT_Y 32      // block rows of the ICP kernels once they walk the active-job list (iterations >= ICP_GROUP_FROM >= 1)
static_assert(ICP_GROUP_FROM >= 1, "the first active-job list is written by the update of iteration ICP_GROUP_FROM - 1");
#define ICP_NACC 29      // 21 (JTJ upper) + 6 (JTr) + count + err2  |  p2p: 3 + 3 + 9, [15, 21) second moments, count + err2

// ------------------------------------------------------------------------------------------------
// ICP (coloured / point-to-point)
// ------------------------------------------------------------------------------------------------
__global__ void ibl_icp_init_kernel(IcpState* __restrict__ st, int J, const RansacState* __restrict__ rs, int from_identity) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    IcpState s;
    for (int i = 0; i < 16; ++i) s.T[i] = (from_identity || !rs) ? ((i % 5) == 0 ? 1.0 : 0.0) : rs[j].best_T[i];
    s.T[12] = s.T[13] = s.T[14] = 0.0; s.T[15] = 1.0;
    s.fitness = 0; s.rmse = 0; s.iter = 0; s.done = 0; s.started = 0;
    st[j] = s;
}

// nearest target point with d2 < r2 (fp32 distance on the float-rounded query); (d2, index) lexicographic minimum.
// The row of cells through the query's own cell is scanned first: it nearly always holds the neighbour (or one almost as
// close), after which the other rows are skipped unless their distance lower bound can still reach the best -- a row is
// only skipped when the bound is strictly larger, so equal distances are always compared by index and the result does
// not depend on the scan order.
// `pos` / `*d2out` carry the minimum so far in and out (-1 / r2 to start): a target side is searched piece by piece.  The minimum is
// carried as a POSITION in the cell-sorted arrays (the caller reads g.order[pos] once, at the end).
// Inner loop (round 3): eight candidates per step, their loads issued together (one thread's walk is a chain of dependent latencies);
// the comparisons are branch-free selects -- the branchy form (`if (d2 < bd) ... else if (d2 == bd) ...` per candidate) compiled to ~10
// exec-mask / branch instructions per candidate, more than the arithmetic.  An exact tie with the running best (equal fp32 distances of
// two different points: duplicate points, symmetric configurations) is only DETECTED there; the step is then redone from its saved
// state with the sequential rule (lowest original index wins), so the result is the sequential scan's, bit for bit.  Candidates past
// the end of a row are clamped to its last point: a repeat of a candidate changes neither the minimum nor a tie.
// (Round 3 also measured: pruning the row cell by cell -- own cell first, the others by their x gap -- 30 % slower: more dependent
// cell-table loads than points saved.)
__device__ __forceinline__ int nn_within(const BatchGrid& g, const SegGrid& sg, float qx, float qy, float qz, float radius, int pos,
                                         float* d2out) {
    int reach = (int)ceilf(radius * sg.inv);
    if (reach < 1) reach = 1;
    const int cx = (int)floorf((qx - sg.minx) * sg.inv), cy = (int)floorf((qy - sg.miny) * sg.inv), cz = (int)floorf((qz - sg.minz) * sg.inv);
    float bd = *d2out;
    const int x0 = max(cx - reach, 0), x1 = min(cx + reach, sg.nx - 1);
    const float csz = 1.0f / sg.inv, slack = 1e-4f * csz + 1e-6f;
    auto scan_row = [&](int z, int y) {
        const int row = sg.cell_base + (z * sg.ny + y) * sg.nx;
        const int b = g.cell_start[row + x0], e = g.cell_start[row + x1 + 1];
        for (int jj = b; jj < e; jj += 8) {
            int c[8];
            float4 p[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { c[u] = min(jj + u, e - 1); p[u] = g.sorted_pts[c[u]]; }
            const float bd0 = bd;
            const int pos0 = pos;
            unsigned long long tie = 0ull;          // (wave masks OR-ed on the scalar unit: a per-lane flag got packed bit by bit)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float d2 = dist2f(qx, qy, qz, p[u].x, p[u].y, p[u].z);
                const bool lt = d2 < bd;
                tie |= __builtin_amdgcn_ballot_w64((d2 == bd) & (c[u] != pos));          // (pos < 0: a d2 equal to r2 -- the redo rejects it)
                bd = lt ? d2 : bd;
                pos = lt ? c[u] : pos;
            }
            if (tie != 0ull) {          // rare: the sequential rule from the saved state
                bd = bd0;
                pos = pos0;
#pragma unroll
                for (int u = 0; u < 8; ++u) {          // (unrolled: a loop would index p[] dynamically and put it in scratch)
                    const float d2 = dist2f(qx, qy, qz, p[u].x, p[u].y, p[u].z);
                    if (d2 < bd) { bd = d2; pos = c[u]; }
                    else if (d2 == bd && pos >= 0 && c[u] != pos) { if (g.order[c[u]] < g.order[pos]) pos = c[u]; }
                }
            }
        }
    };
    if (x1 >= x0) {
        const bool centre = cz >= 0 && cz < sg.nz && cy >= 0 && cy < sg.ny;
        if (centre) scan_row(cz, cy);
        for (int z = max(cz - reach, 0); z <= min(cz + reach, sg.nz - 1); ++z) {
            // lower bound of the distance to any point of the row: skip what cannot reach the current best
            const float zlo = sg.minz + (float)z * csz;
            const float gz = fmaxf((qz < zlo ? zlo - qz : (qz > zlo + csz ? qz - zlo - csz : 0.0f)) - slack, 0.0f);
            for (int y = max(cy - reach, 0); y <= min(cy + reach, sg.ny - 1); ++y) {
                if (centre && z == cz && y == cy) continue;
                const float ylo = sg.miny + (float)y * csz;
                const float gy = fmaxf((qy < ylo ? ylo - qy : (qy > ylo + csz ? qy - ylo - csz : 0.0f)) - slack, 0.0f);
                if (gz * gz + gy * gy > bd) continue;
                scan_row(z, y);
            }
        }
    }
    *d2out = bd;
    return pos;
}

// The same search by a GROUP of LPQ lanes per query (tail iterations of the ICP, below): a lane takes four consecutive candidates of
// every 4 * LPQ, so a row of n candidates costs n / (4 LPQ) dependent load rounds instead of n / 8, and the lanes of a group share
// their best distance after every row for the pruning.  The group's result is the (d2, index) lexicographic minimum over its lanes:
// the same neighbour as nn_within, whatever the order.  A lane's minimum is a position here too.
template <int LPQ>
__device__ __forceinline__ int nn_within_group(const BatchGrid& g, const SegGrid& sg, float qx, float qy, float qz, float radius, int sub, int pos,
                                               float* d2out) {
    int reach = (int)ceilf(radius * sg.inv);
    if (reach < 1) reach = 1;
    const int cx = (int)floorf((qx - sg.minx) * sg.inv), cy = (int)floorf((qy - sg.miny) * sg.inv), cz = (int)floorf((qz - sg.minz) * sg.inv);
    float bd = *d2out;            // this lane's best
    float gbd = bd;               // the group's best distance (pruning bound)
#pragma unroll
    for (int off = 1; off < LPQ; off <<= 1) gbd = fminf(gbd, __shfl_xor(gbd, off, 64));
    const int x0 = max(cx - reach, 0), x1 = min(cx + reach, sg.nx - 1);
    const float csz = 1.0f / sg.inv, slack = 1e-4f * csz + 1e-6f;
    auto scan_row = [&](int z, int y) {
        const int row = sg.cell_base + (z * sg.ny + y) * sg.nx;
        const int b = g.cell_start[row + x0], e = g.cell_start[row + x1 + 1];
        for (int jj = b + 4 * sub; jj < e; jj += 4 * LPQ) {
            int c[4];
            float4 p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { c[u] = min(jj + u, e - 1); p[u] = g.sorted_pts[c[u]]; }
            const float bd0 = bd;
            const int pos0 = pos;
            unsigned long long tie = 0ull;          // (wave masks OR-ed on the scalar unit: a per-lane flag got packed bit by bit)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d2 = dist2f(qx, qy, qz, p[u].x, p[u].y, p[u].z);
                const bool lt = d2 < bd;
                tie |= __builtin_amdgcn_ballot_w64((d2 == bd) & (c[u] != pos));          // (pos < 0: a d2 equal to r2 -- the redo rejects it)
                bd = lt ? d2 : bd;
                pos = lt ? c[u] : pos;
            }
            if (tie != 0ull) {
                bd = bd0;
                pos = pos0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {          // (unrolled: a loop would index p[] dynamically and put it in scratch)
                    const float d2 = dist2f(qx, qy, qz, p[u].x, p[u].y, p[u].z);
                    if (d2 < bd) { bd = d2; pos = c[u]; }
                    else if (d2 == bd && pos >= 0 && c[u] != pos) { if (g.order[c[u]] < g.order[pos]) pos = c[u]; }
                }
            }
        }
        gbd = fminf(gbd, bd);
#pragma unroll
        for (int off = 1; off < LPQ; off <<= 1) gbd = fminf(gbd, __shfl_xor(gbd, off, 64));
    };
    if (x1 >= x0) {
        const bool centre = cz >= 0 && cz < sg.nz && cy >= 0 && cy < sg.ny;
        if (centre) scan_row(cz, cy);
        for (int z = max(cz - reach, 0); z <= min(cz + reach, sg.nz - 1); ++z) {
            const float zlo = sg.minz + (float)z * csz;
            const float gz = fmaxf((qz < zlo ? zlo - qz : (qz > zlo + csz ? qz - zlo - csz : 0.0f)) - slack, 0.0f);
            for (int y = max(cy - reach, 0); y <= min(cy + reach, sg.ny - 1); ++y) {
                if (centre && z == cz && y == cy) continue;
                const float ylo = sg.miny + (float)y * csz;
                const float gy = fmaxf((qy < ylo ? ylo - qy : (qy > ylo + csz ? qy - ylo - csz : 0.0f)) - slack, 0.0f);
                if (gz * gz + gy * gy > gbd) continue;          // (strictly larger than the group's best: ties are still compared)
                scan_row(z, y);
            }
        }
    }
    *d2out = bd;
    return pos;
}

// Late ICP iterations: the jobs still running are the ones that do not converge (wrong assignments: sources with no target inside the
// correspondence distance scan their whole 5 x 5 x 5 neighbourhood, ~1 000 candidates in ~125 dependent rounds), and with few jobs
// left a launch is as long as one thread's walk (~90 us, 22 launches per batch).  Here LPQ lanes share a query.
template <int LPQ>
__global__ __launch_bounds__(256) void ibl_icp_nn_group_kernel(BatchGrid g, const float4* __restrict__ pts, const int* __restrict__ job_off, int J,
                                                               const int* __restrict__ piece_off, const IcpState* __restrict__ st, float radius,
                                                               float r2, int* __restrict__ nn_idx, float* __restrict__ nn_d2,
                                                               const int* __restrict__ act_list, const int* __restrict__ act_cnt) {
    // grid (chunks of the largest source side, ICP_ACT_Y): block row y walks the ACTIVE jobs y, y + ICP_ACT_Y, ... of the list the previous
    // iteration's update kernel wrote -- a (chunks, J) grid spent 40 us per launch on dispatching the ~90 000 blocks of finished jobs
    const int n_act = *act_cnt;
    const int sub = threadIdx.x % LPQ;
    for (int a = blockIdx.y; a < n_act; a += gridDim.y) {
        const int j = act_list[a];
        const IcpState& S = st[j];
        const int p = job_off[j] + blockIdx.x * (256 / LPQ) + threadIdx.x / LPQ;
        if (p >= job_off[j + 1]) continue;               // (whole groups leave together)
        const int i = g.order[p];
        const float4 s4 = pts[i];
        double T[12], vs[3];
        for (int t = 0; t < 12; ++t) T[t] = S.T[t];
        xform_d(T, s4.x, s4.y, s4.z, vs);
        float d2 = r2;
        int pos = -1;
#pragma unroll 1
        for (int t = 0; t < 3; ++t) {
            const int k = J + 3 * j + t;
            if (piece_off[k + 1] > piece_off[k])      // (a lane keeps its own best from piece to piece; the group's best prunes)
                pos = nn_within_group<LPQ>(g, g.seg[k], (float)vs[0], (float)vs[1], (float)vs[2], radius, sub, pos, &d2);
        }
        int best = pos >= 0 ? g.order[pos] : -1;
        // (d2, index) minimum over the group; best = -1 (with d2 = r2) marks a lane that found nothing
#pragma unroll
        for (int off = 1; off < LPQ; off <<= 1) {
            const float od = __shfl_xor(d2, off, 64);
            const int ob = __shfl_xor(best, off, 64);
            if (od < d2 || (od == d2 && ob >= 0 && (best < 0 || ob < best))) { d2 = od; best = ob; }
        }
        if (sub == 0) {
            nn_idx[i] = best;
            nn_d2[i] = d2;
        }
    }
}

// Thread per source point of every job: nearest target point under the job's current T.  Split from the accumulation so
// that this latency-bound neighbour walk runs with few registers (many waves per SIMD hide the dependent cell / point
// loads) while the fp64 normal equations run in their own kernel on coalesced inputs.
// The grid has one segment per source side (0 .. J) and one per target INSTANCE (J + 3 j + t, `piece_off`): a side made of instances far
// apart would otherwise get one coarse grid over their union (>= extent / 128 per cell, hundreds of points per cell: one such job
// quadrupled the ICP time of its batch).
__global__ __launch_bounds__(256) void ibl_icp_nn_kernel(BatchGrid g, const float4* __restrict__ pts, const int* __restrict__ job_off, int J,
                                                         const int* __restrict__ piece_off, const IcpState* __restrict__ st, float radius,
                                                         float r2, int* __restrict__ nn_idx, float* __restrict__ nn_d2) {
    // grid (chunks of the largest source side, J): the job is the block's y index -- a finished job's blocks leave on their first load,
    // and a thread does not find its job by a binary search over the offsets (eight dependent loads before the walk could start)
    const int j = blockIdx.y;
    const IcpState& S = st[j];
    if (S.done) return;
    const int p = job_off[j] + blockIdx.x * 256 + threadIdx.x;
    if (p >= job_off[j + 1]) return;
    // walk the sources in the cell order of their own grid (segment j of the batch grid = the job's source side, so its sorted positions
    // are [job_off[j], job_off[j + 1]) too): neighbouring lanes then query neighbouring cells of the target grid (a rigid transform
    // keeps them together) and share cache lines
    const int i = g.order[p];
    const float4 s4 = pts[i];
    double T[12], vs[3];
    for (int t = 0; t < 12; ++t) T[t] = S.T[t];
    xform_d(T, s4.x, s4.y, s4.z, vs);
    float d2 = r2;
    int pos = -1;
#pragma unroll 1
    for (int t = 0; t < 3; ++t) {
        const int k = J + 3 * j + t;
        if (piece_off[k + 1] > piece_off[k]) pos = nn_within(g, g.seg[k], (float)vs[0], (float)vs[1], (float)vs[2], radius, pos, &d2);
    }
    nn_idx[i] = pos >= 0 ? g.order[pos] : -1;
    nn_d2[i] = d2;
}

// grid (ICP_BPJ, J), or (ICP_BPJ, ICP_ACT_Y) over the active-job list (act_list != null): the normal-equation / Kabsch moments of the
// correspondences found by ibl_icp_nn_kernel
__global__ __launch_bounds__(256) void ibl_icp_step_kernel(const float4* __restrict__ pts, const float4* __restrict__ normals,
                                                           const float4* __restrict__ grad, const int* __restrict__ job_off, int J,
                                                           const IcpState* __restrict__ st, const int* __restrict__ nn_idx,
                                                           const float* __restrict__ nn_d2, int colored,
                                                           double sl_g, double sl_p, double* __restrict__ partial /* [J][BPJ][NACC] */,
                                                           const int* __restrict__ act_list, const int* __restrict__ act_cnt) {
    const int n_act = act_list ? *act_cnt : J;
    for (int a = blockIdx.y; a < n_act; a += gridDim.y) {
    const int j = act_list ? act_list[a] : a;
    const IcpState& S = st[j];
    if (S.done) continue;
    const int sb = job_off[j], se = job_off[j + 1];
    double T[12];
    for (int t = 0; t < 12; ++t) T[t] = S.T[t];
    double acc[ICP_NACC];
    for (int t = 0; t < ICP_NACC; ++t) acc[t] = 0.0;
    for (int i = sb + blockIdx.x * 256 + threadIdx.x; i < se; i += ICP_BPJ * 256) {
        const int tj = nn_idx[i];
        if (tj < 0) continue;
        const float d2 = nn_d2[i];
        const float4 s4 = pts[i];
        double vs[3];
        xform_d(T, s4.x, s4.y, s4.z, vs);
        acc[27] += 1.0;
        acc[28] += (double)d2;
        const float4 t4 = pts[tj];
        const double vt[3] = {t4.x, t4.y, t4.z};
        if (colored) {
            const float4 n4 = normals[tj], g4 = grad[tj];
            const double nt[3] = {n4.x, n4.y, n4.z};
            double Jr[6], r, c[3];
            const double dv[3] = {vs[0] - vt[0], vs[1] - vt[1], vs[2] - vt[2]};
            cross3d(vs, nt, c);
            Jr[0] = sl_g * c[0]; Jr[1] = sl_g * c[1]; Jr[2] = sl_g * c[2]; Jr[3] = sl_g * nt[0]; Jr[4] = sl_g * nt[1]; Jr[5] = sl_g * nt[2];
            r = sl_g * dot3d(dv, nt);
            int q = 0;
            for (int a = 0; a < 6; ++a) { for (int b = a; b < 6; ++b) acc[q++] += Jr[a] * Jr[b]; }
            for (int a = 0; a < 6; ++a) acc[21 + a] += Jr[a] * r;
            const double pr = dot3d(dv, nt);
            const double vp[3] = {vs[0] - pr * nt[0], vs[1] - pr * nt[1], vs[2] - pr * nt[2]};
            const double is = s4.w, itg = t4.w;
            const double dit[3] = {g4.x, g4.y, g4.z};
            const double dp[3] = {vp[0] - vt[0], vp[1] - vt[1], vp[2] - vt[2]};
            const double is0 = dot3d(dit, dp) + itg;
            const double dn = dot3d(dit, nt);
            const double ditM[3] = {-(dit[0] - dn * nt[0]), -(dit[1] - dn * nt[1]), -(dit[2] - dn * nt[2])};
            cross3d(vs, ditM, c);
            Jr[0] = sl_p * c[0]; Jr[1] = sl_p * c[1]; Jr[2] = sl_p * c[2]; Jr[3] = sl_p * ditM[0]; Jr[4] = sl_p * ditM[1]; Jr[5] = sl_p * ditM[2];
            r = sl_p * (is - is0);
            q = 0;
            for (int a = 0; a < 6; ++a) { for (int b = a; b < 6; ++b) acc[q++] += Jr[a] * Jr[b]; }
            for (int a = 0; a < 6; ++a) acc[21 + a] += Jr[a] * r;
        } else {
            for (int a = 0; a < 3; ++a) { acc[a] += vs[a]; acc[3 + a] += vt[a]; acc[15 + a] += vs[a] * vs[a]; acc[18 + a] += vt[a] * vt[a]; }
            for (int rr = 0; rr < 3; ++rr) for (int cc = 0; cc < 3; ++cc) acc[6 + 3 * rr + cc] += vt[rr] * vs[cc];
        }
    }
    __shared__ double sh[4][ICP_NACC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = 0; t < ICP_NACC; ++t) {
        const double v = wave_sum_d(acc[t]);
        if (lane == 0) sh[wave][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < ICP_NACC)
        partial[((int64_t)j * ICP_BPJ + blockIdx.x) * ICP_NACC + threadIdx.x] =
            ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
    __syncthreads();          // (sh is reused by the next job of this block row)
    }
}

__device__ inline bool solve6_d(double A[6][6], double* b, double* x) {
    double M[6][7];
    for (int i = 0; i < 6; ++i) { for (int j = 0; j < 6; ++j) M[i][j] = A[i][j]; M[i][6] = b[i]; }
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        double mx = fabs(M[c][c]);
        for (int r = c + 1; r < 6; ++r) if (fabs(M[r][c]) > mx) { mx = fabs(M[r][c]); piv = r; }
        if (mx == 0.0 || !isfinite(mx)) return false;
        if (piv != c) for (int jj = 0; jj <= 6; ++jj) { const double t = M[c][jj]; M[c][jj] = M[piv][jj]; M[piv][jj] = t; }
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] / M[c][c];
            for (int jj = c; jj <= 6; ++jj) M[r][jj] -= f * M[c][jj];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double s = M[i][6];
        for (int jj = i + 1; jj < 6; ++jj) s -= M[i][jj] * x[jj];
        x[i] = s / M[i][i];
    }
    return true;
}

// wave per job: finish the reduction, convergence test, Gauss-Newton / Kabsch update
// act_list / act_cnt: the active jobs of this iteration (null: all J, one block each); next_list / next_cnt (may be null): the jobs
// still running after this update are appended for the next iteration (in any order: jobs are independent)
__device__ __forceinline__ void icp_update_job(IcpState* __restrict__ st, int j, const int* __restrict__ job_off, const double* __restrict__ partial,
                                               int colored, int max_iter, double rel_fitness, double rel_rmse, int* __restrict__ next_list,
                                               int* __restrict__ next_cnt);
__global__ __launch_bounds__(64) void ibl_icp_update_kernel(IcpState* __restrict__ st, int J, const int* __restrict__ job_off, const double* __restrict__ partial,
                                      int colored, int max_iter, double rel_fitness, double rel_rmse, const int* __restrict__ act_list,
                                      const int* __restrict__ act_cnt, int* __restrict__ next_list, int* __restrict__ next_cnt) {
    const int n_act = act_list ? *act_cnt : J;
    for (int a = blockIdx.x; a < n_act; a += gridDim.x)
        icp_update_job(st, act_list ? act_list[a] : a, job_off, partial, colored, max_iter, rel_fitness, rel_rmse, next_list, next_cnt);
}
__device__ __forceinline__ void icp_update_job(IcpState* __restrict__ st, int j, const int* __restrict__ job_off, const double* __restrict__ partial,
                                               int colored, int max_iter, double rel_fitness, double rel_rmse, int* __restrict__ next_list,
                                               int* __restrict__ next_cnt) {
    // one wavefront per job: lane t folds moment t over the blocks (in block order), lane 0 solves
    if (st[j].done) return;
    double mine = 0.0;
    if (threadIdx.x < ICP_NACC)
        for (int b = 0; b < ICP_BPJ; ++b) mine += partial[((int64_t)j * ICP_BPJ + b) * ICP_NACC + threadIdx.x];
    double a[ICP_NACC];
    for (int t = 0; t < ICP_NACC; ++t) a[t] = __shfl(mine, t, 64);
    if (threadIdx.x != 0) return;
    IcpState S = st[j];
    const int ns = job_off[j + 1] - job_off[j];
    const double cnt = a[27], err2 = a[28];
    const double nf = ns > 0 ? cnt / (double)ns : 0.0, nr = cnt > 0 ? sqrt(err2 / cnt) : 0.0;
    if (S.started && fabs(S.fitness - nf) < rel_fitness && fabs(S.rmse - nr) < rel_rmse) {
        S.fitness = nf; S.rmse = nr; S.done = 1;
        st[j] = S;
        return;
    }
    S.fitness = nf; S.rmse = nr; S.started = 1;
    if (S.iter >= max_iter) { S.done = 1; st[j] = S; return; }
    double U[16];
    for (int i = 0; i < 16; ++i) U[i] = (i % 5) == 0 ? 1.0 : 0.0;
    if (cnt > 0) {
        if (colored) {
            double A[6][6], nb[6], x[6];
            int q = 0;
            for (int r = 0; r < 6; ++r) for (int c = r; c < 6; ++c) { A[r][c] = a[q]; A[c][r] = a[q]; ++q; }
            for (int r = 0; r < 6; ++r) nb[r] = -a[21 + r];
            if (solve6_d(A, nb, x)) {
                const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
                U[0] = cg * cb; U[1] = cg * sb * sa - sg * ca; U[2] = cg * sb * ca + sg * sa; U[3] = x[3];
                U[4] = sg * cb; U[5] = sg * sb * sa + cg * ca; U[6] = sg * sb * ca - cg * sa; U[7] = x[4];
                U[8] = -sb;     U[9] = cb * sa;                U[10] = cb * ca;               U[11] = x[5];
            }
        } else {
            double sm[3], dm[3], H[3][3];
            for (int t = 0; t < 3; ++t) { sm[t] = a[t] / cnt; dm[t] = a[3 + t] / cnt; }
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r][c] = a[6 + 3 * r + c] - cnt * dm[r] * sm[c];
            // Every correspondence on ONE target point (a single point within reach), or from one source point: H is zero but for the
            // rounding of the two moments it is the difference of, and the rank test of the Kabsch step is relative to the largest
            // singular value, so it would read a rotation out of that noise (the centred sum gives exact zeros and the identity).
            // The roundings (~24 of them along the fold, each relative to a partial sum) are bounded by
            // |sum vt_r vs_c| <= sqrt(sum vt_r^2 * sum vs_c^2); an H that is below 2^-46 of that bound in all nine entries is zero.
            // (A genuine cloud cannot fall under it: its H is ~ cnt * extent^2 against a bound of ~ cnt * distance^2 from the origin, so a
            // 1 cm cluster 1 km away still sits at 1e-10 of the bound, four orders above the threshold.)
            bool zero = true;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) zero = zero && fabs(H[r][c]) <= 0x1p-46 * sqrt(a[18 + r] * a[15 + c]);
            if (zero) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r][c] = 0.0;
            kabsch_from_moments(sm, dm, H, U);
        }
    }
    double R[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) {
        double s = 0;
        for (int k = 0; k < 4; ++k) s += U[4 * r + k] * S.T[4 * k + c];
        R[4 * r + c] = s;
    }
    for (int i = 0; i < 16; ++i) S.T[i] = R[i];
    S.iter++;
    st[j] = S;
    if (next_list) next_list[atomicAdd(next_cnt, 1)] = j;        // still running
}

// ------------------------------------------------------------------------------------------------
// the iteration loop: 31 x (neighbours, moments, update) from the RANSAC transforms (coloured) or the identity (point-to-point)
// ------------------------------------------------------------------------------------------------
int ibl_reg_icp_stage(ibl_reg_ctx* ctx, RegPass& ps) {
    const int J = ps.J, colored = ps.colored ? 1 : 0;
    hipStream_t s = ps.s;
    const float radius = (float)ps.max_dist_icp, r2 = (float)(ps.max_dist_icp * ps.max_dist_icp);
    double* partial; int* icp_nn; float* icp_d2;
    IBL_ARENA(partial, double, (int64_t)J * ICP_BPJ * ICP_NACC);
    IBL_ARENA(icp_nn, int, ps.Ns + 64);
    IBL_ARENA(icp_d2, float, ps.Ns + 64);
    hipLaunchKernelGGL(ibl_icp_init_kernel, dim3((J + 63) / 64), dim3(64), 0, s, ps.is, J, ps.rs, colored ? 0 : 1);
    IBL_LAUNCH_CHECK();
    const double lambda_geometric = 0.968;
    const int max_iter = 30;
    int max_side = 0;
    for (int j = 0; j < J; ++j) max_side = std::max(max_side, ps.job_off[j + 1] - ps.job_off[j]);
    const unsigned chunks = (unsigned)std::max(1, (max_side + 255) / 256);
    // from ICP_GROUP_FROM on the kernels walk the list of jobs still running (written by the previous update: list it & 1, count
    // act_cnt[it]) on a grid of ICP_ACT_Y block rows instead of one row per job
    int *act_list, *act_cnt;
    IBL_ARENA(act_list, int, 2 * (int64_t)J + 64);
    IBL_ARENA(act_cnt, int, max_iter + 8);
    IBL_HIP_CHECK(hipMemsetAsync(act_cnt, 0, sizeof(int) * (max_iter + 8), s));
    const unsigned act_y = (unsigned)std::min(J, ICP_ACT_Y);
    for (int it = 0; it <= max_iter; ++it) {
        const bool listed = it >= ICP_GROUP_FROM;
        const int* cur_list = listed ? act_list + (size_t)(it & 1) * J : nullptr;
        const int* cur_cnt = listed ? act_cnt + it : nullptr;
        int* nxt_list = it + 1 >= ICP_GROUP_FROM ? act_list + (size_t)((it + 1) & 1) * J : nullptr;
        int* nxt_cnt = it + 1 >= ICP_GROUP_FROM ? act_cnt + it + 1 : nullptr;
        if (!listed)
            hipLaunchKernelGGL(ibl_icp_nn_kernel, dim3(chunks, J), dim3(256), 0, s, ps.gC, ps.P, ps.d_job_off, J, ps.d_piece_off, ps.is, radius,
                               r2, icp_nn, icp_d2);
        else
            hipLaunchKernelGGL(ibl_icp_nn_group_kernel<ICP_LPQ>, dim3(chunks * ICP_LPQ, act_y), dim3(256), 0, s, ps.gC, ps.P, ps.d_job_off, J,
                               ps.d_piece_off, ps.is, radius, r2, icp_nn, icp_d2, cur_list, cur_cnt);
        IBL_LAUNCH_CHECK();
        hipLaunchKernelGGL(ibl_icp_step_kernel, dim3(ICP_BPJ, listed ? act_y : (unsigned)J), dim3(256), 0, s, ps.P, ps.normals, ps.grad, ps.d_job_off, J,
                           ps.is, icp_nn, icp_d2, colored, sqrt(lambda_geometric), sqrt(1.0 - lambda_geometric), partial, cur_list, cur_cnt);
        IBL_LAUNCH_CHECK();
        hipLaunchKernelGGL(ibl_icp_update_kernel, dim3(listed ? act_y : (unsigned)J), dim3(64), 0, s, ps.is, J, ps.d_job_off, partial, colored, max_iter,
                           1e-6, 1e-6, cur_list, cur_cnt, nxt_list, nxt_cnt);
        IBL_LAUNCH_CHECK();
    }
    return IBL_OK;
}
