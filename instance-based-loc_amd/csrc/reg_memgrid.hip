// reg_memgrid.hip -- the whole-memory hash grid (ibl_memgrid): a hash grid over the concatenation of all memory clouds, built once
// (ibl_memgrid_build) and, when live, edited where it stands: ibl_memgrid_append merges points in, ibl_memgrid_remove and
// ibl_memgrid_replace splice them out and in.  reg_eval.hip and reg_assoc.hip hold the kernels that read it (reg_memgrid.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <memory>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_memgrid.h"

__global__ __launch_bounds__(256) void ibl_mg_key_kernel(const float4* __restrict__ pts, int64_t n, float inv, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    keys[i] = mg_key((int)floorf(p.x * inv), (int)floorf(p.y * inv), (int)floorf(p.z * inv));
    vals[i] = (int)i;
}

__global__ __launch_bounds__(256) void ibl_mg_heads_kernel(const unsigned long long* __restrict__ skeys, int64_t n, int* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}

// Stable merge, old side: point i of the cell-ordered old points moves up by the number of new points in cells before its own (new
// points of its own cell follow it: they have the higher original indices).  One thread per point, 16-byte load and store; the new
// keys are a few thousand and stay in cache.  The merged keys go along for the cell boundaries, and a live grid's original indices
// (sidx_src / sidx_dst, null for an immutable grid) with their points.
__global__ __launch_bounds__(256) void ibl_mg_merge_old_kernel(const float4* __restrict__ src, const int* __restrict__ sidx_src, int64_t n_old,
                                                               float inv, const unsigned long long* __restrict__ nkeys, int n_new,
                                                               float4* __restrict__ dst, int* __restrict__ sidx_dst,
                                                               unsigned long long* __restrict__ mkeys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_old) return;
    const float4 p = src[i];
    const unsigned long long k = mg_key((int)floorf(p.x * inv), (int)floorf(p.y * inv), (int)floorf(p.z * inv));
    const int64_t d = i + mg_bound(nkeys, n_new, k, 0);
    dst[d] = p;
    mkeys[d] = k;
    if (sidx_dst) sidx_dst[d] = sidx_src[i];
}

// new side: sorted new point j moves up by the number of old points in cells up to and including its own, read from the old cell arrays
// (none for an empty grid: ustart[0] = 0, and the sorted new points are the grid's points)
__global__ __launch_bounds__(256) void ibl_mg_merge_new_kernel(const float4* __restrict__ pts, const int* __restrict__ order,
                                                               const unsigned long long* __restrict__ nkeys, int n_new,
                                                               const unsigned long long* __restrict__ ukeys, const int* __restrict__ ustart,
                                                               int n_cells, int n_old, float4* __restrict__ dst, int* __restrict__ sidx_dst,
                                                               unsigned long long* __restrict__ mkeys) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_new) return;
    const unsigned long long k = nkeys[j];
    const int64_t d = (int64_t)j + ustart[mg_bound(ukeys, n_cells, k, 1)];
    const int src = order[j];
    dst[d] = pts[src];
    mkeys[d] = k;
    if (sidx_dst) sidx_dst[d] = n_old + src;        // the new points count as the points behind all earlier ones
}

// ---- splice: points taken out of and put into the middle of the index space (ibl_memgrid_remove, ibl_memgrid_replace) --------------
// The edit is given as R ascending, disjoint ranges of original indices: rbeg / rend, rcum[r] = the resident points in the ranges
// 0 .. r, which go, and ncum[r] = the new points of the ranges 0 .. r, which take their place: the new points, in the order they are
// given, carry the concatenation indices c = 0 .. n_new - 1, those of range r are ncum[r - 1] <= c < ncum[r].  A range may be empty
// (an insertion) or get no points (a removal).  In the spliced sequence an old point with original index idx stands behind the new
// points of every range that begins at or below idx, a new point of range r behind the old points below rbeg[r] -- and that order,
// within a cell, is the build's.
//
// For original index `idx`: is it kept, and *nr = the number of ranges that begin at or below it -- rcum[*nr - 1] removed points lie
// below a kept point.  One binary search, bounded by R (a few thousand entries at most: they stay in cache).
__device__ __forceinline__ bool mg_kept(const int* __restrict__ rbeg, const int* __restrict__ rend, int R, int idx, int* nr) {
    int lo = 0, hi = R;                             // lo = number of ranges that begin at or below idx
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rbeg[mid] <= idx) lo = mid + 1; else hi = mid;
    }
    *nr = lo;
    return lo == 0 || idx >= rend[lo - 1];          // (of a kept point: every range that begins at or below it ends at or below it)
}

// one thread per resident slot: 1 for a point that stays
__global__ __launch_bounds__(256) void ibl_mg_remove_flag_kernel(const int* __restrict__ sidx, int64_t n, const int* __restrict__ rbeg,
                                                                 const int* __restrict__ rend, int R, int* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int nr;
    keep[i] = mg_kept(rbeg, rend, R, sidx[i], &nr) ? 1 : 0;
}

// Old side: kept slot i moves to keep_scan[i] (the exclusive sum of the flags: the kept points before it) + the new points of lower
// cells + the new points of its own cell that precede it in the spliced sequence: those with c < ncum[nr - 1].  `order` ascends
// inside a run of equal new keys (the sort is stable), so that count is one more bounded search; without new points (a removal)
// nothing is searched and the move is the stable compaction.  16-byte load and store, the key (recomputed with the build's
// floorf(p * inv)) for the cell boundaries, the original index renumbered to the one it has in the spliced sequence.  Per resident
// point 4 B (flag) + 4 B (scan) + 4 B (sidx) read, per kept point 16 B read and 16 + 8 + 4 B written.
__global__ __launch_bounds__(256) void ibl_mg_replace_old_kernel(const float4* __restrict__ src, const int* __restrict__ sidx_src, int64_t n,
                                                                 float inv, const int* __restrict__ rbeg, const int* __restrict__ rend,
                                                                 const int* __restrict__ rcum, const int* __restrict__ ncum, int R,
                                                                 const int* __restrict__ keep, const int* __restrict__ keep_scan,
                                                                 const unsigned long long* __restrict__ nkeys, const int* __restrict__ order,
                                                                 int n_new, int64_t n_out, float4* __restrict__ dst,
                                                                 int* __restrict__ sidx_dst, unsigned long long* __restrict__ mkeys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    int nr;
    const int idx = sidx_src[i];
    mg_kept(rbeg, rend, R, idx, &nr);
    const int c_before = nr ? ncum[nr - 1] : 0;
    const float4 p = src[i];
    const unsigned long long k = mg_key((int)floorf(p.x * inv), (int)floorf(p.y * inv), (int)floorf(p.z * inv));
    int64_t d = keep_scan[i];
    if (n_new > 0) {
        const int lo = mg_bound(nkeys, n_new, k, 0);
        d += (lo < n_new && nkeys[lo] == k) ? mg_bound_int(order, lo, mg_bound(nkeys, n_new, k, 1), c_before) : lo;
    }
    if (d < 0 || d >= n_out) return;                // (cannot happen: the host counted n_out from the same ranges)
    dst[d] = p;
    mkeys[d] = k;
    sidx_dst[d] = idx - (nr ? rcum[nr - 1] : 0) + c_before;
}

// New side: sorted new point j of range r moves up by the kept old points before it: those of lower cells and, inside its own cell
// [s, e) of the old grid, those below rbeg[r] -- sidx ascends inside a cell, one bounded search; a cell the old grid does not have
// begins where the next higher one does.  keep_scan has n + 1 entries (a position behind the last slot counts every kept point).
__global__ __launch_bounds__(256) void ibl_mg_replace_new_kernel(const float4* __restrict__ pts, const int* __restrict__ order,
                                                                 const unsigned long long* __restrict__ nkeys, int n_new,
                                                                 const unsigned long long* __restrict__ ukeys, const int* __restrict__ ustart,
                                                                 int n_cells, const int* __restrict__ sidx_src,
                                                                 const int* __restrict__ keep_scan, const int* __restrict__ rbeg,
                                                                 const int* __restrict__ rcum, const int* __restrict__ ncum, int R,
                                                                 int64_t n_out, float4* __restrict__ dst, int* __restrict__ sidx_dst,
                                                                 unsigned long long* __restrict__ mkeys) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_new) return;
    const unsigned long long k = nkeys[j];
    const int c = order[j];
    const int r = min(mg_bound_int(ncum, 0, R, c + 1), R - 1);      // the first range with ncum[r] > c (ranges without new points pass)
    const int cell = mg_bound(ukeys, n_cells, k, 0);
    int pos = ustart[cell];
    if (cell < n_cells && ukeys[cell] == k) pos = mg_bound_int(sidx_src, pos, ustart[cell + 1], rbeg[r]);
    const int64_t d = (int64_t)j + keep_scan[pos];
    if (d < 0 || d >= n_out) return;                // (cannot happen, as above)
    dst[d] = pts[c];
    mkeys[d] = k;
    sidx_dst[d] = rbeg[r] - (r ? rcum[r - 1] : 0) + c;
}

__global__ __launch_bounds__(256) void ibl_mg_merged_cells_kernel(const unsigned long long* __restrict__ mkeys, const int* __restrict__ head,
                                                                  const int* __restrict__ head_scan, int64_t n,
                                                                  unsigned long long* __restrict__ ukeys, int* __restrict__ ustart) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (head[i]) { const int c = head_scan[i]; ukeys[c] = mkeys[i]; ustart[c] = (int)i; }
}

// linear probing, the walk bounded by the table: a key that found no slot (cannot happen at <= 1 / 3 load) is reported, never waited for
__global__ __launch_bounds__(256) void ibl_mg_insert_bounded_kernel(const unsigned long long* __restrict__ ukeys, int n_cells,
                                                                    unsigned long long hmask, unsigned long long* __restrict__ tkeys,
                                                                    int* __restrict__ tvals, int* __restrict__ failed) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const unsigned long long k = ukeys[c];
    unsigned long long h = mg_hash(k) & hmask;
    for (unsigned long long probe = 0; probe <= hmask; ++probe) {
        const unsigned long long prev = atomicCAS(&tkeys[h], MG_EMPTY, k);
        if (prev == MG_EMPTY) { tvals[h] = c; return; }
        h = (h + 1) & hmask;
    }
    atomicExch(failed, 1);
}

// Frees the half of the ping-pong pair that is not current and allocates it again for `cap` points (a live grid's original indices
// with it).  The current half, and with it the grid, is untouched whatever happens.
static int mg_alloc_other(ibl_memgrid* g, int64_t cap, hipStream_t s, const char* who) {
    const int o = 1 - g->cur;
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    (void)hipFree(g->buf[o]); (void)hipFree(g->sidx[o]);
    g->buf[o] = nullptr; g->sidx[o] = nullptr; g->buf_cap[o] = 0;
    hipError_t e = hipMalloc(&g->buf[o], sizeof(float4) * (size_t)cap);
    if (e == hipSuccess && !g->fixed) e = hipMalloc(&g->sidx[o], sizeof(int) * (size_t)cap);
    if (e != hipSuccess) {
        (void)hipFree(g->buf[o]);
        g->buf[o] = nullptr;
        return ibl_set_error(IBL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    g->buf_cap[o] = cap;
    return IBL_OK;
}

// The tail of a merge and of a splice: buf[1 - cur] holds the n points of the new state in cell order and mkeys their keys.  Reads
// the cells off the keys (head flags, scan), dimensions and allocates what no longer fits, makes the other buffer the current one
// and refills the table.  head / hscan: n + 1 ints each, tmp: tmp_bytes of scan scratch, failed: 1 int -- the caller's arena scratch.
// Synchronises `s` after the cells are counted and before it returns.
static int mg_cells_table(ibl_memgrid* g, int64_t n, const unsigned long long* mkeys, int* head, int* hscan, int* failed,
                          unsigned char* tmp, size_t tmp_bytes, int64_t reserve_points, hipStream_t s, const char* who) {
    const int o = 1 - g->cur;
    float4* dst = g->buf[o];
    const unsigned nb = (unsigned)((n + 255) / 256);
    size_t t2 = tmp_bytes;
    // cells of the new order, counted
    hipLaunchKernelGGL(ibl_mg_heads_kernel, dim3(nb), dim3(256), 0, s, mkeys, n, head);
    IBL_LAUNCH_CHECK();
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, t2, head, hscan, (int)n, s));
    int last_scan = 0, last_head = 0;
    IBL_HIP_CHECK(hipMemcpyAsync(&last_scan, hscan + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipMemcpyAsync(&last_head, head + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));         // (the merge has read the old cell arrays: they may be replaced now)
    const int n_cells = last_scan + last_head;
    // The table is dimensioned from the OCCUPIED CELLS (round 4): it used to hold 2 n slots -- 128 M slots = 1.5 GB for a 10 000-instance
    // memory whose 50 M surface points occupy a few million 4 cm cells -- so that every probe of the evaluation was a first touch of HBM
    // (1.9 GB moved per launch for 158 MB of points).  At <= 1 / 3 load the table of the same memory is ~100 MB: it stays in the
    // Infinity Cache, and a miss walks 1.5 slots on average.
    unsigned long long H = 1024;
    while (H < (unsigned long long)n_cells * 3) H <<= 1;
    // every allocation the new state needs before any of the old state is overwritten: a failure here leaves the grid as it was
    unsigned long long* ukeys = g->v.ukeys; int* ustart = g->v.ustart; int64_t cell_cap = g->cell_cap;
    unsigned long long* tkeys = g->v.tkeys; int* tvals = g->v.tvals;
    if (n_cells > cell_cap) {
        cell_cap = std::max<int64_t>(n_cells + std::min<int64_t>(reserve_points, n_cells / 2), cell_cap + cell_cap / 2);
        ukeys = nullptr; ustart = nullptr;
        hipError_t e = hipMalloc(&ukeys, sizeof(unsigned long long) * (size_t)cell_cap);
        if (e == hipSuccess) e = hipMalloc(&ustart, sizeof(int) * (size_t)(cell_cap + 1));
        if (e != hipSuccess) { (void)hipFree(ukeys); return ibl_set_error(IBL_ERR_HIP, "%s: %s", who, hipGetErrorString(e)); }
    }
    if (H > g->tab_cap) {
        tkeys = nullptr; tvals = nullptr;
        hipError_t e = hipMalloc(&tkeys, sizeof(unsigned long long) * H);
        if (e == hipSuccess) e = hipMalloc(&tvals, sizeof(int) * H);
        if (e != hipSuccess) {
            (void)hipFree(tkeys);
            if (ukeys != g->v.ukeys) { (void)hipFree(ukeys); (void)hipFree(ustart); }
            return ibl_set_error(IBL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        }
    }
    if (ukeys != g->v.ukeys) { (void)hipFree(g->v.ukeys); (void)hipFree(g->v.ustart); g->v.ukeys = ukeys; g->v.ustart = ustart; g->cell_cap = cell_cap; }
    if (tkeys != g->v.tkeys) { (void)hipFree(g->v.tkeys); (void)hipFree(g->v.tvals); g->v.tkeys = tkeys; g->v.tvals = tvals; g->tab_cap = H; }
    g->v.sorted = dst; g->cur = o; g->v.n = n; g->v.n_cells = n_cells; g->v.hmask = H - 1;
    hipLaunchKernelGGL(ibl_mg_merged_cells_kernel, dim3(nb), dim3(256), 0, s, mkeys, head, hscan, n, g->v.ukeys, g->v.ustart);
    IBL_LAUNCH_CHECK();
    const int nn = (int)n;
    IBL_HIP_CHECK(hipMemcpyAsync(g->v.ustart + n_cells, &nn, sizeof(int), hipMemcpyHostToDevice, s));
    // the table (smallest power of two >= 3 n_cells, >= 1024), refilled: the cell indices have shifted
    IBL_HIP_CHECK(hipMemsetAsync(g->v.tkeys, 0xFF, sizeof(unsigned long long) * H, s));
    IBL_HIP_CHECK(hipMemsetAsync(failed, 0, sizeof(int), s));
    hipLaunchKernelGGL(ibl_mg_insert_bounded_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, s, g->v.ukeys, n_cells, g->v.hmask, g->v.tkeys,
                       g->v.tvals, failed);
    IBL_LAUNCH_CHECK();
    int h_failed = 0;
    IBL_HIP_CHECK(hipMemcpyAsync(&h_failed, failed, sizeof(int), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    if (h_failed) return ibl_set_error(IBL_ERR_OVERFLOW, "%s: the cell table is full", who);
    return IBL_OK;
}

// Merges n_new (> 0) further points into the grid -- all of them into an empty grid: that is the build.  The new points are keyed and
// sorted (stable: equal keys keep their index order), both sides are merged into the other point buffer, the cells are read off the
// merged keys and the table is refilled.  reserve_points: room for further cells when the cell arrays are (re)allocated.
// The arena is scratch only.  Synchronises `s` after the cells are counted and before it returns.
static int mg_merge(ibl_reg_ctx* ctx, ibl_memgrid* g, const float4* P, int64_t n_new, int64_t reserve_points, hipStream_t s, const char* who) {
    const int64_t n_old = g->v.n, n = n_old + n_new;
    ArenaMark scratch(ctx);
    unsigned long long *keys, *nkeys, *mkeys; int *vals, *order, *head, *hscan, *failed; unsigned char* tmp;
    IBL_ARENA(keys, unsigned long long, n_new);
    IBL_ARENA(nkeys, unsigned long long, n_new);
    IBL_ARENA(vals, int, n_new);
    IBL_ARENA(order, int, n_new);
    IBL_ARENA(mkeys, unsigned long long, n);
    IBL_ARENA(head, int, n + 1);
    IBL_ARENA(hscan, int, n + 1);
    IBL_ARENA(failed, int, 1);
    size_t t1 = 0, t2 = 0;
    IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, head, hscan, (int)n, s));
    IBL_ARENA(tmp, unsigned char, (int64_t)std::max(t1, t2) + 256);
    // the other half of the ping-pong pair: grown by 1.5 when the merged points no longer fit
    const int o = 1 - g->cur;
    if (g->buf_cap[o] < n) {
        const int st = mg_alloc_other(g, std::min<int64_t>(0x7FFFFFF0ll, std::max<int64_t>(n, g->buf_cap[g->cur] + g->buf_cap[g->cur] / 2)), s, who);
        if (st != IBL_OK) return st;
    }
    float4* dst = g->buf[o];
    const unsigned nb_new = (unsigned)((n_new + 255) / 256), nb_old = (unsigned)((n_old + 255) / 256);
    hipLaunchKernelGGL(ibl_mg_key_kernel, dim3(nb_new), dim3(256), 0, s, P, n_new, g->v.inv, keys, vals);
    IBL_LAUNCH_CHECK();
    IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, t1, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
    if (n_old > 0) {
        hipLaunchKernelGGL(ibl_mg_merge_old_kernel, dim3(nb_old), dim3(256), 0, s, g->v.sorted, g->sidx[g->cur], n_old, g->v.inv, nkeys,
                           (int)n_new, dst, g->sidx[o], mkeys);
        IBL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ibl_mg_merge_new_kernel, dim3(nb_new), dim3(256), 0, s, P, order, nkeys, (int)n_new, g->v.ukeys, g->v.ustart,
                       g->v.n_cells, (int)n_old, dst, g->sidx[o], mkeys);
    IBL_LAUNCH_CHECK();
    return mg_cells_table(g, n, mkeys, head, hscan, failed, tmp, t2, reserve_points, s, who);
}

// The one edit of the middle of a live grid, for ibl_memgrid_remove and ibl_memgrid_replace: `h` = rbeg | rend | rcum | ncum of R
// validated ranges (above), P the n_new = ncum[R - 1] >= 0 new points.  The grid afterwards is the build of the spliced sequence.
// No sort of resident points: the resident slots are flagged and scanned, the new points (if any) are keyed and sorted as an
// append's are, and both sides scatter into the other point buffer to positions found by bounded binary searches
// (ibl_mg_replace_old_kernel / _new_kernel); cells and table then follow as after a merge.  A removal (n_new = 0) takes no sort
// scratch, launches no sort and no new side: it is one stable compaction, and dropping points from the resident (cell, original
// index) order and renumbering them monotonely leaves the order the build gives the kept points alone.
// Traffic per resident point: 36 B for points and indices (16 + 4 read, 16 + 4 written when kept) and ~40 B for flags, keys, head
// flags and their scans, + 8 B of the new keys' searches (cached) when there are new points; per new point 16 + 8 + 4 B read and
// 16 + 8 + 4 B written.  Scratch (arena, released on return): 8 B per resident point, 16 B per point of the result, 24 B per new
// point + the sort's and scans'.  Nothing is launched before every arena and buffer allocation has succeeded.
// ibl_memgrid_append and the build do NOT come through here, although an append is the splice of one empty range at n: here it would
// flag and scan every resident point (~12 B per resident point) that the merge kernels never touch, and an append is the edit a
// growing memory makes most.  mg_merge stays.
static int mg_splice(ibl_reg_ctx* ctx, ibl_memgrid* g, const std::vector<int>& h, int R, const float4* P, hipStream_t s, const char* who) {
    const int64_t n = g->v.n, n_keep = n - h[3 * (size_t)R - 1], n_new = h[4 * (size_t)R - 1], n_out = n_keep + n_new;
    const int n_scan = (int)(n_new > 0 ? n + 1 : n);        // (the new side reads the scan one behind the last slot)
    ArenaMark scratch(ctx);
    int *ranges, *keep, *kscan, *vals = nullptr, *order = nullptr, *head, *hscan, *failed;
    unsigned long long *keys = nullptr, *nkeys = nullptr, *mkeys; unsigned char* tmp;
    IBL_ARENA(ranges, int, 4 * (int64_t)R);
    IBL_ARENA(keep, int, n + 1);
    IBL_ARENA(kscan, int, n + 1);
    size_t t0 = 0, t1 = 0, t2 = 0;
    if (n_new > 0) {
        IBL_ARENA(keys, unsigned long long, n_new);
        IBL_ARENA(nkeys, unsigned long long, n_new);
        IBL_ARENA(vals, int, n_new);
        IBL_ARENA(order, int, n_new);
        IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t0, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
    }
    IBL_ARENA(mkeys, unsigned long long, n_out);
    IBL_ARENA(head, int, n_out + 1);
    IBL_ARENA(hscan, int, n_out + 1);
    IBL_ARENA(failed, int, 1);
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, keep, kscan, n_scan, s));
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, head, hscan, (int)n_out, s));
    IBL_ARENA(tmp, unsigned char, (int64_t)std::max(t0, std::max(t1, t2)) + 256);
    // The other half of the ping-pong pair becomes the current one.  It is brought to the current half's capacity first (there is none
    // before the first append, and it lags one growth behind after an append that grew), so that the capacity the grid reports never
    // shrinks and what a removal freed is headroom; a result that no longer fits grows it by 1.5 as in a merge.
    const int o = 1 - g->cur;
    const int64_t cap_cur = g->buf_cap[g->cur];
    const int64_t cap = n_out <= cap_cur ? cap_cur : std::min<int64_t>(0x7FFFFFF0ll, std::max<int64_t>(n_out, cap_cur + cap_cur / 2));
    if (g->buf_cap[o] < cap) {
        const int st = mg_alloc_other(g, cap, s, who);
        if (st != IBL_OK) return st;
    }
    const int *rbeg = ranges, *rend = ranges + R, *rcum = ranges + 2 * (size_t)R, *ncum = ranges + 3 * (size_t)R;
    const unsigned nb = (unsigned)((n + 255) / 256), nb_new = (unsigned)((n_new + 255) / 256);
    auto scatter = [&]() -> int {
        int st = ibl_stage_upload(ctx, ranges, h.data(), (int64_t)(sizeof(int) * h.size()), s);
        if (st != IBL_OK) return st;
        if (n_new > 0) {
            hipLaunchKernelGGL(ibl_mg_key_kernel, dim3(nb_new), dim3(256), 0, s, P, n_new, g->v.inv, keys, vals);
            IBL_LAUNCH_CHECK();
            IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, t0, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
            IBL_HIP_CHECK(hipMemsetAsync(keep + n, 0, sizeof(int), s));
        }
        hipLaunchKernelGGL(ibl_mg_remove_flag_kernel, dim3(nb), dim3(256), 0, s, g->sidx[g->cur], n, rbeg, rend, R, keep);
        IBL_LAUNCH_CHECK();
        IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, t1, keep, kscan, n_scan, s));
        hipLaunchKernelGGL(ibl_mg_replace_old_kernel, dim3(nb), dim3(256), 0, s, g->v.sorted, g->sidx[g->cur], n, g->v.inv, rbeg, rend, rcum, ncum,
                           R, keep, kscan, nkeys, order, (int)n_new, n_out, g->buf[o], g->sidx[o], mkeys);
        IBL_LAUNCH_CHECK();
        if (n_new > 0) {
            hipLaunchKernelGGL(ibl_mg_replace_new_kernel, dim3(nb_new), dim3(256), 0, s, P, order, nkeys, (int)n_new, g->v.ukeys, g->v.ustart,
                               g->v.n_cells, g->sidx[g->cur], kscan, rbeg, rcum, ncum, R, n_out, g->buf[o], g->sidx[o], mkeys);
            IBL_LAUNCH_CHECK();
        }
        return mg_cells_table(g, n_out, mkeys, head, hscan, failed, tmp, t2, 0, s, who);
    };
    const int st = scatter();
    if (st != IBL_OK) (void)hipStreamSynchronize(s);        // (mg_cells_table has synchronised when it succeeds)
    ibl_stage_reset(ctx);                                   // the pinned staging of the ranges is recycled by the next call
    return st;
}

extern "C" int ibl_memgrid_destroy(ibl_memgrid* g) {
    if (!g) return IBL_OK;
    (void)hipFree(g->buf[0]); (void)hipFree(g->buf[1]); (void)hipFree(g->sidx[0]); (void)hipFree(g->sidx[1]); (void)hipFree(g->v.ukeys); (void)hipFree(g->v.ustart);
    (void)hipFree(g->v.tkeys); (void)hipFree(g->v.tvals);
    delete g;
    return IBL_OK;
}

// a build is the merge of all points into an empty grid (n = 0, no cells, ustart[0] = 0) whose point buffer holds n + reserve_points
static int mg_build(ibl_reg_ctx* ctx, const float* mem_pts4, int64_t n, double cell, int64_t reserve_points, int fixed, ibl_memgrid** out,
                    hipStream_t s, const char* who) {
    std::unique_ptr<ibl_memgrid, int (*)(ibl_memgrid*)> g(new ibl_memgrid(), ibl_memgrid_destroy);      // freed on every error return below
    g->v.cell = (float)cell; g->v.inv = 1.0f / (float)cell;
    g->fixed = fixed;
    g->cur = 1;                                                                                          // the merge writes buf[0]
    IBL_HIP_CHECK(hipMalloc(&g->buf[0], sizeof(float4) * (size_t)(n + reserve_points)));
    g->buf_cap[0] = n + reserve_points;
    if (!fixed) IBL_HIP_CHECK(hipMalloc(&g->sidx[0], sizeof(int) * (size_t)(n + reserve_points)));
    IBL_HIP_CHECK(hipMalloc(&g->v.ustart, sizeof(int)));
    IBL_HIP_CHECK(hipMemsetAsync(g->v.ustart, 0, sizeof(int), s));
    const int st = mg_merge(ctx, g.get(), reinterpret_cast<const float4*>(mem_pts4), n, reserve_points, s, who);
    if (st != IBL_OK) return st;
    *out = g.release();
    return IBL_OK;
}

extern "C" int ibl_memgrid_build(ibl_reg_ctx* ctx, const float* mem_pts4, int64_t n, double cell, int live, int64_t reserve_points,
                                 ibl_memgrid** out, void* stream) {
    if (!ctx || !mem_pts4 || !out || n <= 0 || n > 0x7FFFFFF0ll || cell <= 0 || reserve_points < 0 || reserve_points > 0x7FFFFFF0ll - n)
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_build: bad argument");
    if (!live && reserve_points != 0) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_build: reserve_points needs a live grid");
    return mg_build(ctx, mem_pts4, n, cell, reserve_points, live ? 0 : 1, out, (hipStream_t)stream, "ibl_memgrid_build");
}

extern "C" int ibl_memgrid_append(ibl_reg_ctx* ctx, ibl_memgrid* g, const float* new_pts4, int64_t n_new, void* stream) {
    if (!ctx || !g || n_new < 0 || (n_new > 0 && !new_pts4)) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_append: bad argument");
    if (g->fixed) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_append: a grid built with live = 0 is immutable (build it with live = 1)");
    if (n_new == 0) return IBL_OK;
    if (g->v.n + n_new > 0x7FFFFFF0ll) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_append: more than 0x7FFFFFF0 points");
    return mg_merge(ctx, g, reinterpret_cast<const float4*>(new_pts4), n_new, 0, (hipStream_t)stream, "ibl_memgrid_append");
}

// Removes the points whose ORIGINAL indices lie in the given ranges: the splice that puts nothing in their place.  Everything is
// checked on the host before the first launch.
extern "C" int ibl_memgrid_remove(ibl_reg_ctx* ctx, ibl_memgrid* g, const int64_t* range_begin, const int64_t* range_end, int n_ranges,
                                  void* stream) {
    if (!ctx || !g || n_ranges < 0 || (n_ranges > 0 && (!range_begin || !range_end)))
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: bad argument");
    if (g->fixed) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: a grid built with live = 0 is immutable (build it with live = 1)");
    if (n_ranges == 0) return IBL_OK;
    const int64_t n = g->v.n;
    const int R = n_ranges;
    std::vector<int> h(4 * (size_t)R, 0);           // rbeg | rend | rcum | ncum (no new points)
    int64_t removed = 0, prev_end = 0;
    for (int r = 0; r < R; ++r) {
        if (range_begin[r] < prev_end || range_end[r] <= range_begin[r] || range_end[r] > n)
            return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: range %d [%lld, %lld) is empty, out of order, overlaps the one before or "
                                 "passes the grid's %lld points", r, (long long)range_begin[r], (long long)range_end[r], (long long)n);
        prev_end = range_end[r];
        removed += range_end[r] - range_begin[r];
        h[r] = (int)range_begin[r]; h[R + r] = (int)range_end[r]; h[2 * (size_t)R + r] = (int)removed;
    }
    if (removed >= n) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: the ranges cover every point (a grid is never empty)");
    return mg_splice(ctx, g, h, R, nullptr, (hipStream_t)stream, "ibl_memgrid_remove");
}

// Replaces the points whose ORIGINAL indices lie in range r by the next new_count[r] rows of new_pts4: the new points take the place
// of the range in the index space, everything else keeps its relative order, and the grid afterwards is the build of the spliced
// sequence.  Everything is checked on the host before the first launch.
extern "C" int ibl_memgrid_replace(ibl_reg_ctx* ctx, ibl_memgrid* g, const int64_t* range_begin, const int64_t* range_end,
                                   const int64_t* new_count, const float* new_pts4, int n_ranges, void* stream) {
    if (!ctx || !g || n_ranges < 0 || (n_ranges > 0 && (!range_begin || !range_end || !new_count)))
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: bad argument");
    if (g->fixed) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: a grid built with live = 0 is immutable (build it with live = 1)");
    if (n_ranges == 0) return IBL_OK;
    const int64_t n = g->v.n;
    const int R = n_ranges;
    std::vector<int> h(4 * (size_t)R);              // rbeg | rend | rcum | ncum
    int64_t removed = 0, added = 0, prev_end = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t b = range_begin[r], e = range_end[r], c = new_count[r];
        if (b < prev_end || e < b || e > n || (r > 0 && b == range_begin[r - 1]))
            return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: range %d [%lld, %lld) is reversed, out of order, overlaps the one before, "
                                 "begins where it begins or passes the grid's %lld points", r, (long long)b, (long long)e, (long long)n);
        if (c < 0 || (c == 0 && e == b) || c > 0x7FFFFFF0ll)
            return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: range %d [%lld, %lld) gets %lld new points (an empty range needs some)", r,
                                 (long long)b, (long long)e, (long long)c);
        prev_end = e;
        removed += e - b;
        added += c;
        if (added > 0x7FFFFFF0ll) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: more than 0x7FFFFFF0 points");
        h[r] = (int)b; h[R + r] = (int)e; h[2 * (size_t)R + r] = (int)removed; h[3 * (size_t)R + r] = (int)added;
    }
    const int64_t n_out = n - removed + added;
    if (added > 0 && !new_pts4) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: new_pts4 is null");
    if (n_out <= 0) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: nothing would remain (a grid is never empty)");
    if (n_out > 0x7FFFFFF0ll) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: more than 0x7FFFFFF0 points");
    return mg_splice(ctx, g, h, R, reinterpret_cast<const float4*>(new_pts4), (hipStream_t)stream, "ibl_memgrid_replace");
}

extern "C" int ibl_memgrid_export(const ibl_memgrid* g, float* sorted_out, uint64_t* ukeys_out, int32_t* ustart_out, void* stream) {
    if (!g) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_export: grid is null");
    hipStream_t s = (hipStream_t)stream;
    if (sorted_out) IBL_HIP_CHECK(hipMemcpyAsync(sorted_out, g->v.sorted, sizeof(float4) * (size_t)g->v.n, hipMemcpyDeviceToDevice, s));
    if (ukeys_out)
        IBL_HIP_CHECK(hipMemcpyAsync(ukeys_out, g->v.ukeys, sizeof(unsigned long long) * (size_t)g->v.n_cells, hipMemcpyDeviceToDevice, s));
    if (ustart_out) IBL_HIP_CHECK(hipMemcpyAsync(ustart_out, g->v.ustart, sizeof(int) * ((size_t)g->v.n_cells + 1), hipMemcpyDeviceToDevice, s));
    return IBL_OK;
}

extern "C" int ibl_memgrid_info(const ibl_memgrid* g, int64_t* n, int32_t* n_cells, int64_t* table_slots, int64_t* point_capacity,
                                int32_t* ustart_end, void* stream) {
    if (!g) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_info: grid is null");
    if (n) *n = g->v.n;
    if (n_cells) *n_cells = g->v.n_cells;
    if (table_slots) *table_slots = (int64_t)(g->v.hmask + 1);
    if (point_capacity) *point_capacity = g->buf_cap[g->cur];
    if (ustart_end) {
        IBL_HIP_CHECK(hipMemcpyAsync(ustart_end, g->v.ustart + g->v.n_cells, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
        IBL_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    }
    return IBL_OK;
}
