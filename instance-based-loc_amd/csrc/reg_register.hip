// reg_register.hip -- batched registration of (detected, memory) cloud pairs: the entry point, the retry loop and one pass
//   assemble jobs (concatenate + centre) -> grid C -> features + 33-d matching with mutual filter (reg_match.hip)
//   -> RANSAC on correspondences (reg_ransac.hip) -> coloured / point-to-point ICP (reg_icp.hip) -> read back
// Scoring against the whole memory is reg_eval.hip.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once,
//   object_memory/object_memory.py:1023-1034   concatenate the chosen clouds, subtract each side's mean
//   utils/fpfh_register.py:100-143            register_point_clouds (Open3D RANSAC + coloured ICP, p2p fallback)
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_stages.h"

#ifndef ICP_CELL_DIV
#define ICP_CELL_DIV 2.0     // cells of the ICP neighbour grid per correspondence distance (finer cells: fewer candidates per walk)
#endif

// ------------------------------------------------------------------------------------------------
// job assembly
// ------------------------------------------------------------------------------------------------

// grid (J, 2): mean of the concatenated clouds in double
__global__ __launch_bounds__(256) void ibl_job_mean_kernel(const JobDesc* __restrict__ jobs, const float4* __restrict__ det,
                                                           const int* __restrict__ det_off, const float4* __restrict__ mem,
                                                           const int* __restrict__ mem_off, int center, double* __restrict__ means /* [J][2][3] */) {
    const int j = blockIdx.x, side = blockIdx.y;
    const float4* pool = side == 0 ? det : mem;
    const int* off = side == 0 ? det_off : mem_off;
    double sx = 0, sy = 0, sz = 0;
    long long cnt = 0;
    for (int t = 0; t < 3; ++t) {
        const int sg = side == 0 ? jobs[j].src_seg[t] : jobs[j].tgt_seg[t];
        if (sg < 0) continue;
        const int b = off[sg], e = off[sg + 1];
        cnt += e - b;
        for (int i = b + threadIdx.x; i < e; i += 256) { const float4 p = pool[i]; sx += p.x; sy += p.y; sz += p.z; }
    }
    __shared__ double sh[3][256];
    sh[0][threadIdx.x] = sx; sh[1][threadIdx.x] = sy; sh[2][threadIdx.x] = sz;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (threadIdx.x < st) for (int a = 0; a < 3; ++a) sh[a][threadIdx.x] += sh[a][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int a = 0; a < 3; ++a) means[(j * 2 + side) * 3 + a] = (center && cnt > 0) ? sh[a][0] / (double)cnt : 0.0;
}

// writes the centred job clouds: segments [0, J) = sources, [J, 2J) = targets
__global__ __launch_bounds__(256) void ibl_job_gather_kernel(const JobDesc* __restrict__ jobs, int J, const float4* __restrict__ det,
                                                             const int* __restrict__ det_off, const float4* __restrict__ mem,
                                                             const int* __restrict__ mem_off, const int* __restrict__ job_off /* [2J+1] */,
                                                             const double* __restrict__ means, float4* __restrict__ out) {
    const int n = job_off[2 * J];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int sgi = seg_of(job_off, 2 * J, i);
    const int side = sgi >= J ? 1 : 0, j = side ? sgi - J : sgi;
    int local = i - job_off[sgi];
    const float4* pool = side == 0 ? det : mem;
    const int* off = side == 0 ? det_off : mem_off;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < 3; ++t) {
        const int sg = side == 0 ? jobs[j].src_seg[t] : jobs[j].tgt_seg[t];
        if (sg < 0) continue;
        const int len = off[sg + 1] - off[sg];
        if (local < len) { p = pool[off[sg] + local]; break; }
        local -= len;
    }
    const double* m = means + (j * 2 + side) * 3;
    out[i] = make_float4((float)((double)p.x - m[0]), (float)((double)p.y - m[1]), (float)((double)p.z - m[2]), p.w);
}

__global__ void ibl_status_clear_kernel(int* __restrict__ status, int mask) { atomicAnd(status, ~mask); }
__global__ void ibl_status_set_kernel(int* __restrict__ status, int mask) { atomicOr(status, mask); }

// ------------------------------------------------------------------------------------------------
// one pass
// ------------------------------------------------------------------------------------------------
static double now_ms() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

void RegPass::phase(const char* what) {
    if (timing < 1) return;
    (void)hipStreamSynchronize(s);
    const double t = now_ms();
    fprintf(stderr, "[reg] %-28s %7.3f ms\n", what, t - t_prev);
    t_prev = t;
}

void RegPass::dbg(const char* what) const {
    if (timing < 2) return;
    const hipError_t e = hipStreamSynchronize(s);
    fprintf(stderr, "[reg-dbg] %-36s %s\n", what, hipGetErrorString(e));
}

// host: job table + job cloud offsets; device: means and the centred job clouds -> ps.P
static int assemble_jobs(ibl_reg_ctx* ctx, RegPass& ps) {
    const RegCall& c = *ps.call;
    const int J = ps.J;
    hipStream_t s = ps.s;
    ps.jobs.resize(J);
    ps.job_off.assign(2 * J + 1, 0);
    for (int j = 0; j < J; ++j) {
        int ns = 0, nt = 0;
        for (int t = 0; t < 3; ++t) {
            const int a = c.job_src_seg[3 * j + t], b = c.job_tgt_seg[3 * j + t];
            if (a >= c.det.n_seg || b >= c.mem.n_seg) return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: segment index out of range");
            ps.jobs[j].src_seg[t] = a; ps.jobs[j].tgt_seg[t] = b;
            if (a >= 0) ns += c.det.off_host[a + 1] - c.det.off_host[a];
            if (b >= 0) nt += c.mem.off_host[b + 1] - c.mem.off_host[b];
        }
        ps.job_off[j + 1] = ns;          // sizes first, prefix below
        ps.job_off[J + j + 1] = nt;
    }
    for (int i = 0; i < 2 * J; ++i) ps.job_off[i + 1] += ps.job_off[i];
    const int N = ps.N = ps.job_off[2 * J];
    ps.Ns = ps.job_off[J];

    IBL_ARENA(ps.d_jobs, JobDesc, J);
    IBL_ARENA(ps.d_job_off, int, 2 * J + 1);
    IBL_ARENA(ps.d_means, double, (int64_t)J * 6);
    IBL_ARENA(ps.P, float4, N + 1);
    IBL_ARENA(ps.normals, float4, N + 1);
    int st = ibl_stage_upload(ctx, ps.d_jobs, ps.jobs.data(), sizeof(JobDesc) * (int64_t)J, s);
    if (st) return st;
    st = ibl_stage_upload(ctx, ps.d_job_off, ps.job_off.data(), sizeof(int) * (int64_t)(2 * J + 1), s);
    if (st) return st;
    hipLaunchKernelGGL(ibl_job_mean_kernel, dim3(J, 2), dim3(256), 0, s, ps.d_jobs, ps.det, c.det.off_dev, ps.mem, c.mem.off_dev,
                       (c.params.flags & IBL_REG_CENTER) ? 1 : 0, ps.d_means);
    IBL_LAUNCH_CHECK();
    if (N > 0) {
        hipLaunchKernelGGL(ibl_job_gather_kernel, dim3((N + 255) / 256), dim3(256), 0, s, ps.d_jobs, J, ps.det, c.det.off_dev, ps.mem, c.mem.off_dev,
                           ps.d_job_off, ps.d_means, ps.P);
        IBL_LAUNCH_CHECK();
    }
    return IBL_OK;
}

// upper bound of the cells of grid C at cell size cell0, from the instance boxes: a side's extent is at most the union of its boxes
static int64_t grid_c_cell_bound(const RegPass& ps, float cell0) {
    const RegCall& c = *ps.call;
    const int J = ps.J;
    int64_t bound = 0;
    for (int sgi = 0; sgi < 4 * J; ++sgi) {
        const int pl = sgi >= J ? 1 : 0, j = pl ? (sgi - J) / 3 : sgi, only = pl ? (sgi - J) % 3 : -1;
        float lo[3], hi[3];
        union_of_boxes(pl ? ps.jobs[j].tgt_seg : ps.jobs[j].src_seg, only, pl ? c.mem.off_host : c.det.off_host,
                       pl ? c.mem.features->bbox : c.det.features->bbox, lo, hi);
        double cells = 1;
        float cell = cell0;
        const float emax = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        if (emax * 1.0001f / 128.0f > cell) cell = emax / 128.0f;
        for (int a = 0; a < 3; ++a) cells *= std::floor((double)(hi[a] - lo[a]) * 1.0001 / cell) + 2.0;
        bound += (int64_t)cells;
    }
    return bound;
}

// Grid C (cell = ICP correspondence distance) lives until the end of the pass: ICP neighbours (reach 1) and colour gradients
// (radius 2 * max_dist, reach 2).  Its segments: the J source sides, then every target side instance by instance.
static int build_grid_c(ibl_reg_ctx* ctx, RegPass& ps) {
    const RegCall& c = *ps.call;
    const int J = ps.J;
    hipStream_t s = ps.s;
    // With the instance boxes on the host (instance features carry them) the table is sized from an upper bound of every job
    // side's extent -- centring moves a side, it does not stretch it beyond rounding -- and the build needs no read-back.
    // A batch with many spread-out job sides (assignments to instances far apart) would not fit the cell budget at the nominal cell
    // size: the cell grows until it does.  The neighbour walk derives its reach from the cell size, so only the work changes.
    const bool have = c.det.features && c.mem.features && c.det.features->bbox && c.mem.features->bbox;
    const int64_t budget = (int64_t)128 << 20;
    float cellC = (float)(ps.max_dist_icp / ICP_CELL_DIV);
    std::vector<int> piece_off(4 * (size_t)J + 1, 0);
    for (int j = 0; j <= J; ++j) piece_off[j] = ps.job_off[j];
    for (int j = 0; j < J; ++j)
        for (int t = 0; t < 3; ++t) {
            const int b = ps.jobs[j].tgt_seg[t];
            piece_off[J + 3 * j + t + 1] = piece_off[J + 3 * j + t] + (b >= 0 ? c.mem.off_host[b + 1] - c.mem.off_host[b] : 0);
        }
    IBL_ARENA(ps.d_piece_off, int, 4 * (int64_t)J + 1);
    int st = ibl_stage_upload(ctx, ps.d_piece_off, piece_off.data(), sizeof(int) * (4 * (int64_t)J + 1), s);
    if (st) return st;
    int64_t bound = have ? grid_c_cell_bound(ps, cellC) : 0;
    for (int tries = 0; have && bound >= budget && tries < 12; ++tries) { cellC *= 1.5f; bound = grid_c_cell_bound(ps, cellC); }
    if (have && bound < budget) return ibl_build_batch_grid_bounded(ctx, ps.P, ps.d_piece_off, piece_off.data(), 4 * J, cellC, bound, &ps.gC, s);
    for (int tries = 0; tries < 8; ++tries) {
        st = ibl_build_batch_grid(ctx, ps.P, ps.d_piece_off, piece_off.data(), 4 * J, cellC, budget, false, &ps.gC, s);
        if (st != IBL_ERR_OVERFLOW) break;
        cellC *= 2.0f;
    }
    return st;
}

enum { REDO_RANSAC_FULL_LIST = 1, REDO_FEAT_VALU = 2 };

// reads the states back, decides whether the pass has to be redone (*redo), writes the outputs if not
static int read_back(ibl_reg_ctx* ctx, RegPass& ps, int* redo) {
    const RegCall& c = *ps.call;
    const int J = ps.J;
    hipStream_t s = ps.s;
    const RansacState* rs = ps.rs;
    std::vector<IcpState> h_is(J);
    IBL_HIP_CHECK(hipMemcpyAsync(h_is.data(), ps.is, sizeof(IcpState) * J, hipMemcpyDeviceToHost, s));
    std::vector<RansacState> h_rs;
    if (rs && (c.out.T_ransac || c.out.ransac_stats)) {
        h_rs.resize(J);
        IBL_HIP_CHECK(hipMemcpyAsync(h_rs.data(), rs, sizeof(RansacState) * J, hipMemcpyDeviceToHost, s));
    }
    std::vector<double> h_means((size_t)J * 6);
    IBL_HIP_CHECK(hipMemcpyAsync(h_means.data(), ps.d_means, sizeof(double) * J * 6, hipMemcpyDeviceToHost, s));
    int h_status = 0;
    IBL_HIP_CHECK(hipMemcpyAsync(&h_status, ctx->d_status, sizeof(int), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    ibl_stage_reset(ctx);
    if (ps.tok_icp || ps.tok_ransac) {                 // stage units known now: iterations run per job, hypotheses walked
        double icp_b = 0, hyp = 0;
        for (int j = 0; j < J; ++j) {
            icp_b += 56.0 * (double)(ps.job_off[j + 1] - ps.job_off[j]) * (double)std::max(1, h_is[j].iter);
            if (!h_rs.empty()) hyp += (double)h_rs[j].walked;
        }
        ibl_prof_set_units(ps.tok_icp, icp_b);
        ibl_prof_set_units(ps.tok_ransac, hyp);
    }
    // Overflowed lists make the results of this pass unusable.  Both are decided here, in one place: a pass that overflowed the RANSAC
    // survivor list (near-identical clouds, a loose edge criterion) is redone with a list that holds every hypothesis of a round (same
    // hypotheses, same fold order: the result of a pass whose list never overflowed); one whose matrix-core feature search overflowed
    // its candidate list is redone with the VALU search, which has none; a pass that hit both asks for both at once.
    if ((h_status & IBL_ST_RANSAC_OVERFLOW) && ps.opt.ransac_full_list)
        return ibl_set_error(IBL_ERR_OVERFLOW, "ransac: the surviving hypotheses of one round exceed the list capacity");
    if (h_status & IBL_ST_RANSAC_OVERFLOW) *redo |= REDO_RANSAC_FULL_LIST;
    if ((h_status & IBL_ST_FEAT_OVERFLOW) && !ps.opt.force_valu) *redo |= REDO_FEAT_VALU;
    if (*redo) return IBL_OK;
    for (int j = 0; j < J; ++j) {
        for (int i = 0; i < 16; ++i) c.out.T[16 * j + i] = h_is[j].T[i];
        c.out.rmse[j] = h_is[j].rmse;
        c.out.fitness[j] = h_is[j].fitness;
        if (c.out.means) for (int i = 0; i < 6; ++i) c.out.means[6 * j + i] = h_means[6 * j + i];
        if (c.out.T_ransac) for (int i = 0; i < 16; ++i) c.out.T_ransac[16 * j + i] = rs ? h_rs[j].best_T[i] : ((i % 5) == 0 ? 1.0 : 0.0);
        if (c.out.ransac_stats) {
            c.out.ransac_stats[3 * j] = rs ? h_rs[j].walked : 0;
            c.out.ransac_stats[3 * j + 1] = rs ? h_rs[j].validated : 0;
            c.out.ransac_stats[3 * j + 2] = rs ? h_rs[j].best_inl : 0;
        }
    }
    return IBL_OK;
}

// One pass of the registration call.  *redo (bits REDO_*) tells the caller that the results of this pass are unusable and which
// of the two overflowing lists to avoid in the next one; the pass has released its arena allocations by then (the redo used
// to recurse from inside the pass, with the first pass's allocations still stacked under the second's).
static int register_pass(ibl_reg_ctx* ctx, const RegCall& c, RegPassOpts opt, int* redo) {
    *redo = 0;
    RegPass ps = {};
    ps.call = &c; ps.opt = opt; ps.s = c.stream; ps.J = c.n_jobs;
    ps.colored = (c.params.flags & IBL_REG_HAVE_COLORS) != 0;
    ps.max_dist_icp = c.params.voxel_size * c.params.local_dist_factor;
    ps.det = reinterpret_cast<const float4*>(c.det.pts4);
    ps.mem = reinterpret_cast<const float4*>(c.mem.pts4);
    hipStream_t s = ps.s;
    ArenaMark mark(ctx);
    hipLaunchKernelGGL(ibl_status_clear_kernel, dim3(1), dim3(1), 0, s, ctx->d_status, IBL_ST_FEAT_OVERFLOW | IBL_ST_RANSAC_OVERFLOW);
    IBL_LAUNCH_CHECK();
    ps.timing = ctx->diag.timing;
    ps.t_prev = now_ms();

    int st = assemble_jobs(ctx, ps);
    if (st) return st;
    IBL_ARENA(ps.is, IcpState, ps.J);
    ps.phase("job assembly");
    st = build_grid_c(ctx, ps);
    if (st) return st;
    ps.phase("grid C");
    if (ps.colored) {
        // made here, not by the stages: they outlive the stages' arena marks
        IBL_ARENA(ps.grad, float4, ps.N + 1);
        IBL_ARENA(ps.rs, RansacState, ps.J);
        IBL_ARENA(ps.corr, int2, ps.Ns + 1);
        IBL_ARENA(ps.n_corr, int, ps.J + 1);
        st = ibl_reg_match_stage(ctx, ps);
        if (st) return st;
        st = ibl_reg_ransac_stage(ctx, ps);
        if (st) return st;
    }
    ibl_prof_end(ps.tok_ransac, s);
    ps.phase("ransac");
    ibl_prof_begin(IBL_PROF_ST_ICP, 0.0, s, &ps.tok_icp);
    st = ibl_reg_icp_stage(ctx, ps);
    if (st) return st;
    ibl_prof_end(ps.tok_icp, s);
    ps.phase("icp");
    return read_back(ctx, ps, redo);
}

// at most three passes: the first, one with the lists it asked to avoid, and one more if that pass overflowed the OTHER list
static int register_call(ibl_reg_ctx* ctx, const RegCall& c) {
    RegPassOpts opt;
    int st = IBL_OK;
    for (int pass = 0; pass < 3; ++pass) {
        int redo = 0;
        st = register_pass(ctx, c, opt, &redo);
        if (st != IBL_OK || !redo) break;
        if (redo & REDO_RANSAC_FULL_LIST) opt.ransac_full_list = true;
        if (redo & REDO_FEAT_VALU) opt.force_valu = true;
        hipLaunchKernelGGL(ibl_status_set_kernel, dim3(1), dim3(1), 0, c.stream, ctx->d_status,
                           ((redo & REDO_RANSAC_FULL_LIST) ? IBL_ST_RANSAC_REDONE : 0) | ((redo & REDO_FEAT_VALU) ? IBL_ST_FEAT_REDONE : 0));
    }
    return st;
}

// ------------------------------------------------------------------------------------------------
// the entry point (include/ibloc.h): the argument checks, then the call with the public structs copied into a RegCall
// ------------------------------------------------------------------------------------------------
extern "C" int ibl_register_jobs(ibl_reg_ctx* ctx, const ibl_cloud_pool* det, const ibl_cloud_pool* mem, const int32_t* job_src_seg,
                                 const int32_t* job_tgt_seg, const uint32_t* job_ids, int n_jobs, const ibl_register_params* params,
                                 const ibl_register_out* out, void* stream) {
    if (!ctx || !det || !mem || !params || !out || !det->pts4 || !mem->pts4 || !det->off_dev || !mem->off_dev || !det->off_host ||
        !mem->off_host || !job_src_seg || !job_tgt_seg || !out->T || !out->rmse || !out->fitness)
        return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: null pointer");
    if (n_jobs <= 0 || params->voxel_size <= 0) return ibl_set_error(IBL_ERR_ARG, "ibl_register_jobs: bad sizes");
    const RegCall c = {*det, *mem, job_src_seg, job_tgt_seg, job_ids, n_jobs, *params, *out, (hipStream_t)stream};
    return register_call(ctx, c);
}
