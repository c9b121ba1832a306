// reg_assoc.hip -- association of detections with the resident instances of a live memory (ibl_memgrid_overlap): which instances
// does a detection cloud overlap, counted on the whole-memory hash grid (reg_memgrid.hip) and ranked per detection.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_memgrid.h"

// ------------------------------------------------------------------------------------------------
// association: which resident instances does a detection cloud overlap (ibl_memgrid_overlap)
// ------------------------------------------------------------------------------------------------
// hits(D, m) = #{ p in D : some point q of instance m has dist2f(p, q) < r2 }.  "Some point within r", not "the owner of the
// nearest point": a point that is near several instances counts for each of them, so no tie between instances decides a count.
#define AS_SEEN 8          // distinct instances a thread remembers in registers; further ones are deduplicated by a re-scan (exact)

// does cell c hold a point of the original-index range [ib, ie) within r2 of q?  (sidx ascends inside a cell: the range is a run)
__device__ __forceinline__ bool as_cell_hits_run(const MemGridView& g, const int* __restrict__ sidx, int c, int ib, int ie, float qx, float qy,
                                                 float qz, float r2) {
    const int b = g.ustart[c], e = g.ustart[c + 1];
    for (int t = mg_bound_int(sidx, b, e, ib); t < e && sidx[t] < ie; ++t) {
        const float4 m = g.sorted[t];
        if (dist2f(qx, qy, qz, m.x, m.y, m.z) < r2) return true;
    }
    return false;
}

// One thread per detection point.  The cells of the point's +-r box (at most 27 for r <= cell, one more layer where the padded box
// edge crosses a face) are looked up in the table; inside a cell the points of one instance are a run of ascending original
// indices: the first point of a run within r names the instance (a bounded search of its index in inst_off) and the rest of the
// run is skipped (a bounded search of inst_off[m + 1] in the cell's indices).  An instance met in several cells counts once: the
// first AS_SEEN distinct instances of a point are remembered in registers; for every further one the cells walked before the
// current one are searched again for a point of that instance within r -- exact for any number of instances.
__global__ __launch_bounds__(256) void ibl_overlap_count_kernel(MemGridView g, const int* __restrict__ sidx, const int* __restrict__ inst_off,
                                                                int n_inst, const float4* __restrict__ det, const int* __restrict__ det_off,
                                                                int n_det, float thr, float r2, int* __restrict__ counts /* [n_det][n_inst] */) {
    const int first = det_off[0], last = det_off[n_det];
    for (int64_t i64 = (int64_t)first + (int64_t)blockIdx.x * 256 + threadIdx.x; i64 < last; i64 += (int64_t)gridDim.x * 256) {
        const int i = (int)i64;
        const int d = seg_of(det_off, n_det, i);
        const float4 q4 = det[i];
        const float qx = q4.x, qy = q4.y, qz = q4.z;
        const MgBox box = mg_query_box(g.inv, qx, qy, qz, thr);
        int seen[AS_SEEN];
        int n_seen = 0;
        int* row = counts + (int64_t)d * n_inst;
        for (int ix = box.x0; ix <= box.x1; ++ix)
            for (int iy = box.y0; iy <= box.y1; ++iy)
                for (int iz = box.z0; iz <= box.z1; ++iz) {
                    const int c = mg_find_cell(g, mg_key(ix, iy, iz));
                    if (c < 0) continue;
                    const int b = g.ustart[c], e = g.ustart[c + 1];
                    int t = b;
                    while (t < e) {
                        const float4 m4 = g.sorted[t];
                        if (!(dist2f(qx, qy, qz, m4.x, m4.y, m4.z) < r2)) { ++t; continue; }
                        const int m = seg_of(inst_off, n_inst, sidx[t]);
                        const int ib = inst_off[m], ie = inst_off[m + 1];
                        t = mg_bound_int(sidx, t + 1, e, ie);            // (ie > sidx[t]: the run ends behind t)
                        bool dup = false;
#pragma unroll
                        for (int u = 0; u < AS_SEEN; ++u) dup |= (u < n_seen && seen[u] == m);
                        if (!dup && n_seen == AS_SEEN) {                 // more instances than the registers hold: the cells before this one again
                            for (int jx = box.x0; jx <= ix && !dup; ++jx)
                                for (int jy = box.y0; jy <= (jx < ix ? box.y1 : iy) && !dup; ++jy)
                                    for (int jz = box.z0; jz <= ((jx < ix || jy < iy) ? box.z1 : iz - 1) && !dup; ++jz) {
                                        const int c2 = mg_find_cell(g, mg_key(jx, jy, jz));
                                        if (c2 >= 0) dup = as_cell_hits_run(g, sidx, c2, ib, ie, qx, qy, qz, r2);
                                    }
                        }
                        if (dup) continue;
#pragma unroll
                        for (int u = 0; u < AS_SEEN; ++u) if (u == n_seen) seen[u] = m;
                        if (n_seen < AS_SEEN) ++n_seen;
                        atomicAdd(row + m, 1);                           // integer adds: the totals do not depend on the order
                    }
                }
    }
}

// (hits, instance) as one key that orders by hits descending, then instance ascending, when the larger key comes first
__device__ __forceinline__ unsigned long long as_rank_key(int hits, int inst) {
    return ((unsigned long long)(unsigned)hits << 32) | (unsigned long long)(unsigned)(0x7FFFFFFF - inst);
}

// One workgroup per detection: counts the instances with hits > 0 and writes the first k of them in rank order, one selection
// round per output (the largest key below the one before; keys are distinct): min(k, n_hit) sweeps of the row, then the padding.
__global__ __launch_bounds__(256) void ibl_overlap_rank_kernel(const int* __restrict__ counts, int n_inst, int k, int* __restrict__ pair_inst,
                                                               int* __restrict__ pair_hits, int* __restrict__ n_hit_inst) {
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* row = counts + (int64_t)d * n_inst;
    int* oi = pair_inst + (int64_t)d * k;
    int* oh = pair_hits + (int64_t)d * k;
    __shared__ unsigned long long sh_key[4];
    __shared__ int sh_cnt[4];
    int nz = 0;
    for (int m = tid; m < n_inst; m += 256) nz += row[m] > 0 ? 1 : 0;
    nz = wave_sum_i(nz);
    if (lane == 0) sh_cnt[wave] = nz;
    __syncthreads();
    const int n_hit = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
    if (tid == 0) n_hit_inst[d] = n_hit;
    const int n_out = n_hit < k ? n_hit : k;
    unsigned long long prev = ~0ull;
    for (int r = 0; r < n_out; ++r) {
        unsigned long long best = 0;                                     // (a key with hits > 0 is never 0)
        for (int m = tid; m < n_inst; m += 256) {
            const int h = row[m];
            const unsigned long long key = as_rank_key(h, m);
            if (h > 0 && key < prev && key > best) best = key;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        __syncthreads();                                                 // (the round before has read sh_key)
        if (lane == 0) sh_key[wave] = best;
        __syncthreads();
        best = sh_key[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) best = sh_key[w] > best ? sh_key[w] : best;
        if (tid == 0) { oi[r] = 0x7FFFFFFF - (int)(unsigned)(best & 0xFFFFFFFFull); oh[r] = (int)(best >> 32); }
        prev = best;
    }
    for (int r = n_out + tid; r < k; r += 256) { oi[r] = -1; oh[r] = 0; }
}

extern "C" int ibl_memgrid_overlap(ibl_reg_ctx* ctx, const ibl_memgrid* grid, const int32_t* inst_off, int32_t n_inst, int32_t inst_off_end,
                                   const float* det_pts4, const int32_t* det_off_host, int32_t n_det, double radius, int32_t k,
                                   int32_t* pair_inst, int32_t* pair_hits, int32_t* n_hit_inst, void* stream) {
    if (!ctx || !grid || !inst_off || !det_off_host || !pair_inst || !pair_hits || !n_hit_inst || n_inst < 1 || n_det < 0)
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: bad argument (a null pointer, n_inst < 1 or n_det < 0)");
    if (grid->fixed) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: a grid built with live = 0 keeps no point indices (build it with live = 1)");
    if (!(radius > 0)) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: radius %g is not positive", radius);
    if ((float)radius > grid->v.cell)                        // (in fp32, as the grid keeps its cell: radius == cell passes)
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: radius %g exceeds the grid's cell %g (a query's box would pass 27 cells)", radius,
                             (double)grid->v.cell);
    if (k < 1) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: k = %d, at least 1 expected", (int)k);
    if ((int64_t)inst_off_end != grid->v.n)
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: the instance offsets end at %d, the grid holds %lld points", (int)inst_off_end,
                             (long long)grid->v.n);
    if (det_off_host[0] < 0) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: det_off_host begins below 0");
    for (int d = 0; d < n_det; ++d)
        if (det_off_host[d + 1] < det_off_host[d]) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: det_off_host descends at detection %d", d);
    if (n_det == 0) return IBL_OK;
    const int64_t n_pts = (int64_t)det_off_host[n_det] - det_off_host[0];
    if (n_pts > 0 && !det_pts4) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_overlap: det_pts4 is null");
    hipStream_t s = (hipStream_t)stream;
    ArenaMark scratch(ctx);
    int *counts, *d_off, *o_inst, *o_hits, *o_n;
    const int64_t n_counts = (int64_t)n_det * n_inst, n_pairs = (int64_t)n_det * k;
    IBL_ARENA(counts, int, n_counts);
    IBL_ARENA(d_off, int, (int64_t)n_det + 1);
    IBL_ARENA(o_inst, int, n_pairs);
    IBL_ARENA(o_hits, int, n_pairs);
    IBL_ARENA(o_n, int, n_det);
    auto run = [&]() -> int {
        int st = ibl_stage_upload(ctx, d_off, det_off_host, (int64_t)sizeof(int) * (n_det + 1), s);
        if (st != IBL_OK) return st;
        IBL_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)n_counts, s));
        void* tok;
        ibl_prof_begin(IBL_PROF_ST_ASSOC, 16.0 * (double)n_pts, s, &tok);
        if (n_pts > 0) {
            const unsigned nb = (unsigned)std::min<int64_t>((n_pts + 255) / 256, 1 << 20);
            hipLaunchKernelGGL(ibl_overlap_count_kernel, dim3(nb), dim3(256), 0, s, grid->v, grid->sidx[grid->cur], inst_off, (int)n_inst,
                               reinterpret_cast<const float4*>(det_pts4), d_off, (int)n_det, (float)radius, (float)(radius * radius), counts);
        }
        hipLaunchKernelGGL(ibl_overlap_rank_kernel, dim3(n_det), dim3(256), 0, s, counts, (int)n_inst, (int)k, o_inst, o_hits, o_n);
        ibl_prof_end(tok, s);
        IBL_LAUNCH_CHECK();
        // into vectors first: a failed copy leaves the caller's arrays as they were
        std::vector<int> h_inst((size_t)n_pairs), h_hits((size_t)n_pairs), h_n((size_t)n_det);
        IBL_HIP_CHECK(hipMemcpyAsync(h_inst.data(), o_inst, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipMemcpyAsync(h_hits.data(), o_hits, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipMemcpyAsync(h_n.data(), o_n, sizeof(int) * (size_t)n_det, hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipStreamSynchronize(s));
        std::copy(h_inst.begin(), h_inst.end(), pair_inst);
        std::copy(h_hits.begin(), h_hits.end(), pair_hits);
        std::copy(h_n.begin(), h_n.end(), n_hit_inst);
        return IBL_OK;
    };
    const int st = run();
    if (st != IBL_OK) (void)hipStreamSynchronize(s);         // (nothing queued may outlive the scratch)
    ibl_stage_reset(ctx);                                    // the pinned staging of the offsets is recycled by the next call
    return st;
}
