// reg_eval.hip -- scoring of registration results against the whole memory (the hash grid of reg_memgrid.hip): the fitness / rmse of
// every job's transformed detected points against it, and the information matrix of a pose from the same correspondences.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once,
//   utils/fpfh_register.py:145-150            evaluate_transform against the concatenation of all memory clouds
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_memgrid.h"
#include "reg_stages.h"

struct EvalJob {
    double T[12];
    int begin, end;      // detected point range (all cleaned detected clouds of the job's frame)
    long long out;       // offset of this job's per-point outputs (d2_out of ibl_evaluate_batch, nn_out of ibl_evaluate_information)
};

// The jobs of a call, assembled in `jobs` (which must live until the stream has been synchronised) and copied to the arena, next to
// room for the K sums per job and block that the kernel leaves.
static int eval_upload_jobs(ibl_reg_ctx* ctx, const int32_t* job_begin, const int32_t* job_end, const double* T_global, int J, int K,
                            const char* who, hipStream_t s, std::vector<EvalJob>& jobs, EvalJob** d_jobs, double** partial) {
    jobs.resize(J);
    for (int j = 0; j < J; ++j) {
        for (int t = 0; t < 12; ++t) jobs[j].T[t] = T_global[16 * j + t];
        jobs[j].begin = job_begin[j]; jobs[j].end = job_end[j];
        if (job_end[j] < job_begin[j]) return ibl_set_error(IBL_ERR_ARG, "%s: bad point range", who);
        jobs[j].out = j == 0 ? 0 : jobs[j - 1].out + (jobs[j - 1].end - jobs[j - 1].begin);
    }
    IBL_ARENA(*d_jobs, EvalJob, J);
    IBL_ARENA(*partial, double, (int64_t)J * ICP_BPJ * K);
    IBL_HIP_CHECK(hipMemcpyAsync(*d_jobs, jobs.data(), sizeof(EvalJob) * J, hipMemcpyHostToDevice, s));
    return IBL_OK;
}

// gridDim.y holds at most 65 535 rows: more jobs go in several launches, launch(first job, rows).  A launch numbers its jobs from 0,
// so it is given its part of the jobs and of the partials; job.out stays an offset into the whole of the per-point output.
template <class Launch>
static void eval_launch_rows(int J, Launch launch) {
    const int max_rows = 65535;
    for (int j0 = 0; j0 < J; j0 += max_rows) launch(j0, std::min(J - j0, max_rows));
}

// sum t of job j over its ICP_BPJ block partials (h: [J][ICP_BPJ][K]), in block order
static double eval_partial_sum(const std::vector<double>& h, int j, int K, int t) {
    double v = 0.0;
    for (int b = 0; b < ICP_BPJ; ++b) v += h[((size_t)j * ICP_BPJ + b) * K + t];
    return v;
}

// grid (ICP_BPJ, J): fitness / rmse partials of evaluate_registration against the whole memory
__global__ __launch_bounds__(256) void ibl_evaluate_kernel(MemGridView g, const float4* __restrict__ det, const EvalJob* __restrict__ jobs,
                                                           float thr, float thr2, double* __restrict__ partial /* [J][BPJ][2] */,
                                                           float* __restrict__ d2_out /* per (job, point) or null */, int prune) {
    const int j = blockIdx.y;
    const EvalJob job = jobs[j];
    double cnt = 0, err2 = 0;
    for (int i = job.begin + blockIdx.x * 256 + threadIdx.x; i < job.end; i += ICP_BPJ * 256) {
        const float4 s4 = det[i];
        double p[3];
        xform_d(job.T, s4.x, s4.y, s4.z, p);
        const float qx = (float)p[0], qy = (float)p[1], qz = (float)p[2];
        float best = thr2;
        bool found = false;
        const MgBox box = mg_query_box(g.inv, qx, qy, qz, thr);
        // The query's own cell first, then the (up to seven) others of its +-thr box only while they can still hold a closer point:
        // a neighbouring cell lies behind the face it shares with the own cell, so the distance to that face (per axis that differs) bounds
        // every point of it from below (mg_face_gap).  Round 4: an inlier's nearest point is millimetres away and the faces are
        // centimetres away, so ~1.5 instead of 8 cells are looked up and read (1.6 of the 1.9 GB a launch moved were the points of those
        // cells).  The bound is conservative, and a cell is skipped only when its bound already reaches the best: the minimum is that
        // of the full scan.
        const int hx = (int)floorf(qx * g.inv), hy = (int)floorf(qy * g.inv), hz = (int)floorf(qz * g.inv);
        auto scan_cell = [&](int ix, int iy, int iz) {
            // The probe is mg_find_cell's without its bound, on purpose: bounded by a counter or by the wrap-around, this kernel
            // measured 11 % slower (0.59 against 0.53 ms for 32 jobs of 34 000 points on a 50 M-point memory; the information kernel
            // costs the same either way).  The table is at most a third full, so the walk ends at an empty slot.
            const unsigned long long k = mg_key(ix, iy, iz);
            unsigned long long h = mg_hash(k) & g.hmask;
            int c = -1;
            while (true) {
                const unsigned long long tk = g.tkeys[h];
                if (tk == k) { c = g.tvals[h]; break; }
                if (tk == MG_EMPTY) break;
                h = (h + 1) & g.hmask;
            }
            if (c < 0) return;
            const int b = g.ustart[c], e = g.ustart[c + 1];
            for (int t = b; t < e; t += 4) {           // four points in flight (past the end: the last point again -- a repeat changes no minimum)
                float4 m[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) m[u] = g.sorted[min(t + u, e - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d2 = dist2f(qx, qy, qz, m[u].x, m[u].y, m[u].z);
                    if (d2 < best) { best = d2; found = true; }
                }
            }
        };
        scan_cell(hx, hy, hz);
        for (int ix = box.x0; ix <= box.x1; ++ix) {
            const float gx = mg_face_gap(ix, hx, qx, g.cell);
            for (int iy = box.y0; iy <= box.y1; ++iy) {
                const float gy = mg_face_gap(iy, hy, qy, g.cell);
                for (int iz = box.z0; iz <= box.z1; ++iz) {
                    if (ix == hx && iy == hy && iz == hz) continue;
                    const float gz = mg_face_gap(iz, hz, qz, g.cell);
                    if (prune && gx * gx + gy * gy + gz * gz >= best) continue;
                    scan_cell(ix, iy, iz);
                }
            }
        }
        if (found) { cnt += 1.0; err2 += (double)best; }
        if (d2_out) d2_out[job.out + (i - job.begin)] = found ? best : INFINITY;
    }
    __shared__ double sh[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cnt = wave_sum_d(cnt); err2 = wave_sum_d(err2);
    if (lane == 0) { sh[0][wave] = cnt; sh[1][wave] = err2; }
    __syncthreads();
    if (threadIdx.x < 2)
        partial[((int64_t)j * ICP_BPJ + blockIdx.x) * 2 + threadIdx.x] =
            ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

extern "C" int ibl_evaluate_batch(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const float* det_pts4, const int32_t* job_begin,
                                  const int32_t* job_end, const double* T_global, int n_jobs, double threshold, float* d2_out,
                                  double* rmse_out, double* fitness_out, void* stream) {
    if (!ctx || !grid || !det_pts4 || !job_begin || !job_end || !T_global || !rmse_out || !fitness_out || n_jobs <= 0 || threshold <= 0)
        return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_batch: bad argument");
    hipStream_t s = (hipStream_t)stream;
    ArenaMark mark(ctx);
    const int J = n_jobs;
    std::vector<EvalJob> jobs;
    EvalJob* d_jobs; double* partial;
    const int st = eval_upload_jobs(ctx, job_begin, job_end, T_global, J, 2, "ibl_evaluate_batch", s, jobs, &d_jobs, &partial);
    if (st != IBL_OK) return st;
    const int prune = !ctx->diag.eval_fullscan;          // diagnostics: full scan = every cell of the query's box (the tests compare both)
    void* tok;
    ibl_prof_begin(IBL_PROF_ST_EVAL, 24.0 * (double)(jobs[J - 1].out + (jobs[J - 1].end - jobs[J - 1].begin)), s, &tok);
    eval_launch_rows(J, [&](int j0, int rows) {
        hipLaunchKernelGGL(ibl_evaluate_kernel, dim3(ICP_BPJ, rows), dim3(256), 0, s, grid->v, reinterpret_cast<const float4*>(det_pts4),
                           d_jobs + j0, (float)threshold, (float)(threshold * threshold), partial + (int64_t)j0 * ICP_BPJ * 2, d2_out, prune);
    });
    ibl_prof_end(tok, s);
    IBL_LAUNCH_CHECK();
    std::vector<double> h((size_t)J * ICP_BPJ * 2);
    IBL_HIP_CHECK(hipMemcpyAsync(h.data(), partial, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    for (int j = 0; j < J; ++j) {
        const double cnt = eval_partial_sum(h, j, 2, 0), err2 = eval_partial_sum(h, j, 2, 1);
        const int ns = job_end[j] - job_begin[j];
        fitness_out[j] = ns > 0 ? cnt / (double)ns : 0.0;
        rmse_out[j] = cnt > 0 ? std::sqrt(err2 / cnt) : 0.0;
    }
    return IBL_OK;
}

// ------------------------------------------------------------------------------------------------
// information matrix of a pose from its whole-memory correspondences (ibl_evaluate_information)
// ------------------------------------------------------------------------------------------------
// Open3D's get_information_matrix_from_point_clouds: sum over the correspondences of G^T G, G = [-[m]x | I] of the matched MEMORY
// point m (taken about `about`).  The 36 entries depend on ten sums only -- n, the first and the second moments of m -- which is what
// the kernel reduces; the host assembles the matrix.
#define INFO_SUMS 10       // n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz

// (x, y, z) of a before that of b, compared as floats
__device__ __forceinline__ bool mg_lex_less(float ax, float ay, float az, float bx, float by, float bz) {
    return ax < bx || (ax == bx && (ay < by || (ay == by && az < bz)));
}

// grid (ICP_BPJ, J).  The walk of ibl_evaluate_kernel -- the same transformed point, padded box, own cell first, face bounds -- that
// keeps the matched point next to its distance.  Which of several memory points at the same minimal fp32 d2 is the match must not
// depend on the order they are met in (cell order, live edits, pruning): it is the one with the lexicographically smallest
// (x, y, z).  So a cell is skipped only when its bound lies strictly ABOVE the best distance (a cell that can only tie is read), and
// the table probe is bounded (mg_find_cell).  The two walks stay two bodies: one shared walk would need a second compile-time
// switch for the probe next to the one for the skip rule.  The ten sums are reduced in the evaluation kernel's fixed order: no atomics.
__global__ __launch_bounds__(256) void ibl_information_kernel(MemGridView g, const float4* __restrict__ det, const EvalJob* __restrict__ jobs,
                                                              float thr, float thr2, double ox, double oy, double oz,
                                                              double* __restrict__ partial /* [J][BPJ][INFO_SUMS] */,
                                                              float4* __restrict__ nn_out /* per (job, point) or null */, int prune) {
    const int j = blockIdx.y;
    const EvalJob job = jobs[j];
    double acc[INFO_SUMS];
#pragma unroll
    for (int t = 0; t < INFO_SUMS; ++t) acc[t] = 0.0;
    for (int i = job.begin + blockIdx.x * 256 + threadIdx.x; i < job.end; i += ICP_BPJ * 256) {
        const float4 s4 = det[i];
        double p[3];
        xform_d(job.T, s4.x, s4.y, s4.z, p);
        const float qx = (float)p[0], qy = (float)p[1], qz = (float)p[2];
        float best = thr2, bx = 0.0f, by = 0.0f, bz = 0.0f;
        bool found = false;
        const MgBox box = mg_query_box(g.inv, qx, qy, qz, thr);
        const int hx = (int)floorf(qx * g.inv), hy = (int)floorf(qy * g.inv), hz = (int)floorf(qz * g.inv);
        auto scan_cell = [&](int ix, int iy, int iz) {
            const int c = mg_find_cell(g, mg_key(ix, iy, iz));
            if (c < 0) return;
            const int b = g.ustart[c], e = g.ustart[c + 1];
            for (int t = b; t < e; t += 4) {           // four points in flight (past the end: the last point again -- it neither beats nor precedes itself)
                float4 m[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) m[u] = g.sorted[min(t + u, e - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d2 = dist2f(qx, qy, qz, m[u].x, m[u].y, m[u].z);
                    if (d2 < best || (found && d2 == best && mg_lex_less(m[u].x, m[u].y, m[u].z, bx, by, bz))) {
                        best = d2; bx = m[u].x; by = m[u].y; bz = m[u].z; found = true;
                    }
                }
            }
        };
        scan_cell(hx, hy, hz);
        for (int ix = box.x0; ix <= box.x1; ++ix) {
            const float gx = mg_face_gap(ix, hx, qx, g.cell);
            for (int iy = box.y0; iy <= box.y1; ++iy) {
                const float gy = mg_face_gap(iy, hy, qy, g.cell);
                for (int iz = box.z0; iz <= box.z1; ++iz) {
                    if (ix == hx && iy == hy && iz == hz) continue;
                    const float gz = mg_face_gap(iz, hz, qz, g.cell);
                    if (prune && gx * gx + gy * gy + gz * gz > best) continue;      // strictly above: a cell that can tie is read
                    scan_cell(ix, iy, iz);
                }
            }
        }
        if (found) {
            const double x = (double)bx - ox, y = (double)by - oy, z = (double)bz - oz;
            acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += z;
            acc[4] += x * x; acc[5] += y * y; acc[6] += z * z;
            acc[7] += x * y; acc[8] += x * z; acc[9] += y * z;
        }
        if (nn_out) nn_out[job.out + (i - job.begin)] = found ? make_float4(bx, by, bz, best) : make_float4(0.0f, 0.0f, 0.0f, INFINITY);
    }
    __shared__ double sh[INFO_SUMS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < INFO_SUMS; ++t) {
        const double v = wave_sum_d(acc[t]);
        if (lane == 0) sh[t][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < INFO_SUMS)
        partial[((int64_t)j * ICP_BPJ + blockIdx.x) * INFO_SUMS + threadIdx.x] =
            ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

extern "C" int ibl_evaluate_information(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const float* det_pts4, const int32_t* job_begin,
                                        const int32_t* job_end, const double* T_global, int n_jobs, double threshold, const double* about,
                                        float* nn_out, double* info_out, int64_t* n_corr_out, void* stream) {
    if (!ctx || !grid || !det_pts4 || !job_begin || !job_end || !T_global || !info_out || !n_corr_out || n_jobs <= 0 || !(threshold > 0))
        return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_information: bad argument");
    if (((uintptr_t)det_pts4 | (uintptr_t)nn_out) & 15) return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_information: det_pts4 / nn_out not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ArenaMark mark(ctx);
    const int J = n_jobs;
    for (int j = 0; j < J; ++j)
        if (job_begin[j] < 0) return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_information: bad point range");
    std::vector<EvalJob> jobs;
    EvalJob* d_jobs; double* partial;
    int st = eval_upload_jobs(ctx, job_begin, job_end, T_global, J, INFO_SUMS, "ibl_evaluate_information", s, jobs, &d_jobs, &partial);
    if (st != IBL_OK) return st;
    const double ox = about ? about[0] : 0.0, oy = about ? about[1] : 0.0, oz = about ? about[2] : 0.0;
    const int prune = !ctx->diag.eval_fullscan;
    std::vector<double> h((size_t)J * ICP_BPJ * INFO_SUMS);
    auto run = [&]() -> int {
        eval_launch_rows(J, [&](int j0, int rows) {
            hipLaunchKernelGGL(ibl_information_kernel, dim3(ICP_BPJ, rows), dim3(256), 0, s, grid->v, reinterpret_cast<const float4*>(det_pts4),
                               d_jobs + j0, (float)threshold, (float)(threshold * threshold), ox, oy, oz,
                               partial + (int64_t)j0 * ICP_BPJ * INFO_SUMS, reinterpret_cast<float4*>(nn_out), prune);
        });
        IBL_LAUNCH_CHECK();
        IBL_HIP_CHECK(hipMemcpyAsync(h.data(), partial, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipStreamSynchronize(s));
        return IBL_OK;
    };
    st = run();
    if (st != IBL_OK) { (void)hipStreamSynchronize(s); return st; }      // (nothing queued may outlive the scratch or `jobs`)
    for (int j = 0; j < J; ++j) {
        double S[INFO_SUMS];
        for (int t = 0; t < INFO_SUMS; ++t) S[t] = eval_partial_sum(h, j, INFO_SUMS, t);
        const double n = S[0], sx = S[1], sy = S[2], sz = S[3], sxx = S[4], syy = S[5], szz = S[6], sxy = S[7], sxz = S[8], syz = S[9];
        double* A = info_out + 36 * (size_t)j;
        const double upper[6][6] = {{syy + szz, 0.0 - sxy, 0.0 - sxz, 0.0, 0.0 - sz, sy},
                                    {0.0, sxx + szz, 0.0 - syz, sz, 0.0, 0.0 - sx},
                                    {0.0, 0.0, sxx + syy, 0.0 - sy, sx, 0.0},
                                    {0.0, 0.0, 0.0, n, 0.0, 0.0},
                                    {0.0, 0.0, 0.0, 0.0, n, 0.0},
                                    {0.0, 0.0, 0.0, 0.0, 0.0, n}};
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) A[6 * r + c] = r <= c ? upper[r][c] : upper[c][r];
        n_corr_out[j] = (int64_t)n;
    }
    return IBL_OK;
}
