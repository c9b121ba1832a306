// reg_eval.hip -- scoring of registration results against the whole memory: a hash grid over the concatenation of all memory
// clouds (ibl_memgrid) and the fitness / rmse of every job's transformed detected points against it.
//
// Replaces, for a whole batch of (frame, assignment) jobs at once,
//   utils/fpfh_register.py:145-150            evaluate_transform against the concatenation of all memory clouds
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <memory>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ibloc.h"
#include "reg_common.h"
#include "reg_stages.h"

// ------------------------------------------------------------------------------------------------
// whole-memory hash grid + evaluate_registration
// ------------------------------------------------------------------------------------------------
// what the evaluation kernel takes by value
struct MemGridView {
    float cell, inv;
    int64_t n;
    int n_cells;
    unsigned long long hmask;
    float4* sorted;                 // points in cell order
    unsigned long long* ukeys;      // unique cell keys
    int* ustart;                    // [n_cells + 1]
    unsigned long long* tkeys;      // hash table keys (EMPTY = ~0)
    int* tvals;                     // cell index
};

// The grid owns its device arrays (hipMalloc; freed by ibl_memgrid_destroy): a ping-pong pair for the points (a merge writes buf[cur]
// and the new points into buf[1 - cur], which the first append that needs it allocates), cell arrays and a table with their own
// capacities.  v.sorted is buf[cur].  A live grid also remembers, per sorted slot, the original index of the point that sits there
// (sidx, 4 bytes per point, allocated, ping-ponged and grown with the point buffers): ibl_memgrid_remove finds a removed instance's
// slots by it, ibl_memgrid_replace also the place of the new points inside a cell, ibl_memgrid_overlap the instance a resident point belongs
// to.  Nothing on the query path reads it; an immutable grid has none.
struct ibl_memgrid {
    MemGridView v = {};
    int fixed = 0;                      // 1: made by ibl_memgrid_build with live = 0 -- immutable, ibl_memgrid_append / _remove / _replace refuse it
    float4* buf[2] = {nullptr, nullptr};
    int* sidx[2] = {nullptr, nullptr};  // original index of the point in slot i of buf[.] (live grids only)
    int64_t buf_cap[2] = {0, 0};        // points
    int cur = 0;
    int64_t cell_cap = 0;               // ukeys holds cell_cap, ustart cell_cap + 1 entries
    unsigned long long tab_cap = 0;     // slots of tkeys / tvals
};

#define MG_EMPTY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ unsigned long long mg_key(int ix, int iy, int iz) {
    return ((unsigned long long)(unsigned)(ix + (1 << 20)) << 42) | ((unsigned long long)(unsigned)(iy + (1 << 20)) << 21) |
           (unsigned long long)(unsigned)(iz + (1 << 20));
}
__device__ __forceinline__ unsigned long long mg_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; k ^= k >> 33;
    return k;
}

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

// first index of the sorted keys[0, n) whose key is not below k (strict = 0) / is above k (strict = 1)
__device__ __forceinline__ int mg_bound(const unsigned long long* __restrict__ keys, int n, unsigned long long k, int strict) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const unsigned long long v = keys[mid];
        if (strict ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
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

// ---- removal: a stable compaction of the cell-ordered points (ibl_memgrid_remove) ------------------------------------------------
// The removed points are given as R ascending, disjoint ranges of original indices: rbeg / rend, and rcum[r] = the points in the
// ranges 0 .. r (a replacement's ranges may be empty; a removal's are not).  For original index `idx`: is it kept, and *nr = the
// number of ranges that begin at or below it -- rcum[*nr - 1] removed points lie below a kept point.  One binary search, bounded by
// R (a few thousand entries at most: they stay in cache).
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

// Kept slot i moves to keep_scan[i] (the exclusive sum of the flags) of the other point buffer: 16-byte load and store, its key
// (recomputed with the build's floorf(p * inv)) for the cell boundaries, its original index renumbered to the index it has among
// the kept points.  Per resident point 4 B (flag) + 4 B (scan) + 4 B (sidx) read, per kept point 16 B read and 16 + 8 + 4 B written.
__global__ __launch_bounds__(256) void ibl_mg_remove_scatter_kernel(const float4* __restrict__ src, const int* __restrict__ sidx_src, int64_t n,
                                                                    float inv, const int* __restrict__ rbeg, const int* __restrict__ rend,
                                                                    const int* __restrict__ rcum, int R, const int* __restrict__ keep,
                                                                    const int* __restrict__ keep_scan, int64_t n_keep, float4* __restrict__ dst,
                                                                    int* __restrict__ sidx_dst, unsigned long long* __restrict__ mkeys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int64_t d = keep_scan[i];
    if (d < 0 || d >= n_keep) return;               // (cannot happen: the host counted n_keep from the same ranges)
    int nr;
    const int idx = sidx_src[i];
    mg_kept(rbeg, rend, R, idx, &nr);
    const float4 p = src[i];
    dst[d] = p;
    mkeys[d] = mg_key((int)floorf(p.x * inv), (int)floorf(p.y * inv), (int)floorf(p.z * inv));
    sidx_dst[d] = idx - (nr ? rcum[nr - 1] : 0);
}

// ---- replacement: points spliced into the middle of the index space (ibl_memgrid_replace) -------------------------------------------
// The ranges of a replacement are those of a removal (rbeg / rend / rcum; empty ones allowed) with ncum[r] = the new points of the
// ranges 0 .. r: the new points, in the order they are given, carry the concatenation indices c = 0 .. n_new - 1, those of range r
// are ncum[r - 1] <= c < ncum[r].  In the spliced sequence an old point with original index idx stands behind the new points of
// every range that begins at or below idx, a new point of range r behind the old points below rbeg[r] -- and that order, within
// a cell, is the build's.

// first index of the ascending vals[lo, hi) that is not below v
__device__ __forceinline__ int mg_bound_int(const int* __restrict__ vals, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (vals[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Old side: kept slot i moves to keep_scan[i] (the kept points before it) + the new points of lower cells + the new points of its
// own cell that precede it in the spliced sequence: those with c < ncum[nr - 1].  `order` ascends inside a run of equal new keys
// (the sort is stable), so that count is one more bounded search.  16-byte load and store, the key for the cell boundaries.
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

// The tail of a merge and of a removal: buf[1 - cur] holds the n points of the new state in cell order and mkeys their keys.  Reads
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

// The compaction of a removal: flags the n resident slots whose original index lies outside the R uploaded ranges (`ranges` = rbeg |
// rend | rcum), scans the flags and moves the n_keep kept points, their renumbered indices and their keys into the other buffer.
static int mg_remove_compact(ibl_memgrid* g, int64_t n, int64_t n_keep, const int* ranges, int R, int* keep, int* kscan,
                             unsigned long long* mkeys, unsigned char* tmp, size_t tmp_bytes, hipStream_t s) {
    const int o = 1 - g->cur;
    const int *rbeg = ranges, *rend = ranges + R, *rcum = ranges + 2 * (size_t)R;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(ibl_mg_remove_flag_kernel, dim3(nb), dim3(256), 0, s, g->sidx[g->cur], n, rbeg, rend, R, keep);
    IBL_LAUNCH_CHECK();
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, keep, kscan, (int)n, s));
    hipLaunchKernelGGL(ibl_mg_remove_scatter_kernel, dim3(nb), dim3(256), 0, s, g->v.sorted, g->sidx[g->cur], n, g->v.inv, rbeg, rend, rcum, R,
                       keep, kscan, n_keep, g->buf[o], g->sidx[o], mkeys);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
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

// Removes the points whose ORIGINAL indices lie in the given ranges: one stable compaction of the cell-ordered points into the other
// point buffer -- no sort.  The resident order is (cell, original index); dropping points from it leaves the kept points in (cell,
// index) order, and renumbering them by the count of removed points below is monotone, so the result is the order the build gives the
// kept points alone.  Cells and table then follow as after a merge.  Traffic per resident point: 36 B for points and indices (16 + 4
// read, 16 + 4 written when kept) and ~40 B for flags, keys, head flags and their scans.  Scratch (arena, released on return): 8 B per
// resident point + 16 B per kept point + the scan's.  Everything is checked on the host before the first launch.
extern "C" int ibl_memgrid_remove(ibl_reg_ctx* ctx, ibl_memgrid* g, const int64_t* range_begin, const int64_t* range_end, int n_ranges,
                                  void* stream) {
    if (!ctx || !g || n_ranges < 0 || (n_ranges > 0 && (!range_begin || !range_end)))
        return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: bad argument");
    if (g->fixed) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_remove: a grid built with live = 0 is immutable (build it with live = 1)");
    if (n_ranges == 0) return IBL_OK;
    const int64_t n = g->v.n;
    const int R = n_ranges;
    std::vector<int> h(3 * (size_t)R);              // rbeg | rend | rcum
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
    const int64_t n_keep = n - removed;
    hipStream_t s = (hipStream_t)stream;
    ArenaMark scratch(ctx);
    int *ranges, *keep, *kscan, *head, *hscan, *failed; unsigned long long* mkeys; unsigned char* tmp;
    IBL_ARENA(ranges, int, 3 * (int64_t)R);
    IBL_ARENA(keep, int, n + 1);
    IBL_ARENA(kscan, int, n + 1);
    IBL_ARENA(mkeys, unsigned long long, n_keep);
    IBL_ARENA(head, int, n_keep + 1);
    IBL_ARENA(hscan, int, n_keep + 1);
    IBL_ARENA(failed, int, 1);
    size_t t1 = 0, t2 = 0;
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, keep, kscan, (int)n, s));
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, head, hscan, (int)n_keep, s));
    IBL_ARENA(tmp, unsigned char, (int64_t)std::max(t1, t2) + 256);
    // The other half of the ping-pong pair becomes the current one: it is brought to the current half's capacity first (there is none
    // before the first append, and it lags one growth behind after an append that grew), so that the capacity the grid reports never
    // shrinks and what was freed is headroom.
    const int o = 1 - g->cur;
    if (g->buf_cap[o] < g->buf_cap[g->cur]) {
        const int st = mg_alloc_other(g, g->buf_cap[g->cur], s, "ibl_memgrid_remove");
        if (st != IBL_OK) return st;
    }
    int st = ibl_stage_upload(ctx, ranges, h.data(), (int64_t)(sizeof(int) * h.size()), s);
    if (st == IBL_OK) st = mg_remove_compact(g, n, n_keep, ranges, R, keep, kscan, mkeys, tmp, t1, s);
    if (st == IBL_OK) st = mg_cells_table(g, n_keep, mkeys, head, hscan, failed, tmp, t2, 0, s, "ibl_memgrid_remove");
    if (st != IBL_OK) (void)hipStreamSynchronize(s);        // (mg_cells_table has synchronised when it succeeds)
    ibl_stage_reset(ctx);                                   // the pinned staging of the ranges is recycled by the next call
    return st;
}

// Replaces the points whose ORIGINAL indices lie in range r by the next new_count[r] rows of new_pts4: the new points take the place
// of the range in the index space, everything else keeps its relative order, and the grid afterwards is the build of the spliced
// sequence.  No sort of resident points: the new points are keyed and sorted as an append's are, the resident slots are flagged and
// scanned as a removal's are, and both sides scatter into the other point buffer to positions found by bounded binary searches
// (ibl_mg_replace_old_kernel / _new_kernel).  Traffic per resident point: as a removal, + 8 B of the new keys' searches (cached);
// per new point 16 + 8 + 4 B read and 16 + 8 + 4 B written.  Scratch (arena, released on return): 8 B per resident point, 16 B per
// point of the result, 24 B per new point + the sort's and scans'.  Everything is checked on the host before the first launch.
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
    const int64_t n_keep = n - removed, n_new = added, n_out = n_keep + n_new;
    if (n_new > 0 && !new_pts4) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: new_pts4 is null");
    if (n_out <= 0) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: nothing would remain (a grid is never empty)");
    if (n_out > 0x7FFFFFF0ll) return ibl_set_error(IBL_ERR_ARG, "ibl_memgrid_replace: more than 0x7FFFFFF0 points");
    hipStream_t s = (hipStream_t)stream;
    ArenaMark scratch(ctx);
    int *ranges, *keep, *kscan, *vals, *order, *head, *hscan, *failed; unsigned long long *keys, *nkeys, *mkeys; unsigned char* tmp;
    IBL_ARENA(ranges, int, 4 * (int64_t)R);
    IBL_ARENA(keep, int, n + 1);
    IBL_ARENA(kscan, int, n + 1);
    IBL_ARENA(keys, unsigned long long, n_new);
    IBL_ARENA(nkeys, unsigned long long, n_new);
    IBL_ARENA(vals, int, n_new);
    IBL_ARENA(order, int, n_new);
    IBL_ARENA(mkeys, unsigned long long, n_out);
    IBL_ARENA(head, int, n_out + 1);
    IBL_ARENA(hscan, int, n_out + 1);
    IBL_ARENA(failed, int, 1);
    size_t t0 = 0, t1 = 0, t2 = 0;
    if (n_new > 0) IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, t0, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t1, keep, kscan, (int)(n + 1), s));
    IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, t2, head, hscan, (int)n_out, s));
    IBL_ARENA(tmp, unsigned char, (int64_t)std::max(t0, std::max(t1, t2)) + 256);
    // the other half of the ping-pong pair: brought to the current half's capacity as in a removal, grown by 1.5 as in a merge when
    // the result no longer fits -- the capacity the grid reports never shrinks
    const int o = 1 - g->cur;
    const int64_t cap_cur = g->buf_cap[g->cur];
    const int64_t cap = n_out <= cap_cur ? cap_cur : std::min<int64_t>(0x7FFFFFF0ll, std::max<int64_t>(n_out, cap_cur + cap_cur / 2));
    if (g->buf_cap[o] < cap) {
        const int st = mg_alloc_other(g, cap, s, "ibl_memgrid_replace");
        if (st != IBL_OK) return st;
    }
    const int *rbeg = ranges, *rend = ranges + R, *rcum = ranges + 2 * (size_t)R, *ncum = ranges + 3 * (size_t)R;
    const float4* P = reinterpret_cast<const float4*>(new_pts4);
    const unsigned nb = (unsigned)((n + 255) / 256), nb_new = (unsigned)((n_new + 255) / 256);
    auto scatter = [&]() -> int {
        int st = ibl_stage_upload(ctx, ranges, h.data(), (int64_t)(sizeof(int) * h.size()), s);
        if (st != IBL_OK) return st;
        if (n_new > 0) {
            hipLaunchKernelGGL(ibl_mg_key_kernel, dim3(nb_new), dim3(256), 0, s, P, n_new, g->v.inv, keys, vals);
            IBL_LAUNCH_CHECK();
            IBL_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, t0, keys, nkeys, vals, order, (int)n_new, 0, 63, s));
        }
        hipLaunchKernelGGL(ibl_mg_remove_flag_kernel, dim3(nb), dim3(256), 0, s, g->sidx[g->cur], n, rbeg, rend, R, keep);
        IBL_LAUNCH_CHECK();
        IBL_HIP_CHECK(hipMemsetAsync(keep + n, 0, sizeof(int), s));
        IBL_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, t1, keep, kscan, (int)(n + 1), s));
        hipLaunchKernelGGL(ibl_mg_replace_old_kernel, dim3(nb), dim3(256), 0, s, g->v.sorted, g->sidx[g->cur], n, g->v.inv, rbeg, rend, rcum, ncum,
                           R, keep, kscan, nkeys, order, (int)n_new, n_out, g->buf[o], g->sidx[o], mkeys);
        IBL_LAUNCH_CHECK();
        if (n_new > 0) {
            hipLaunchKernelGGL(ibl_mg_replace_new_kernel, dim3(nb_new), dim3(256), 0, s, P, order, nkeys, (int)n_new, g->v.ukeys, g->v.ustart,
                               g->v.n_cells, g->sidx[g->cur], kscan, rbeg, rcum, ncum, R, n_out, g->buf[o], g->sidx[o], mkeys);
            IBL_LAUNCH_CHECK();
        }
        return IBL_OK;
    };
    int st = scatter();
    if (st == IBL_OK) st = mg_cells_table(g, n_out, mkeys, head, hscan, failed, tmp, t2, 0, s, "ibl_memgrid_replace");
    if (st != IBL_OK) (void)hipStreamSynchronize(s);        // (mg_cells_table has synchronised when it succeeds)
    ibl_stage_reset(ctx);                                   // the pinned staging of the ranges is recycled by the next call
    return st;
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

struct EvalJob {
    double T[12];
    int begin, end;      // detected point range (all cleaned detected clouds of the job's frame)
    long long out;       // offset of this job's per-point distances (d2_out of ibl_evaluate_batch)
};

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
        // The box is padded as the overlap kernel's is: a hit has |q - m| < thr (1 + 3 * 2^-24) per axis (the roundings of thr2, of the
        // difference and of its square), not |q - m| < (float)thr.  For a threshold whose float, squared in fp32, lies below thr2 (0.021,
        // 0.036: not 0.02) a difference of exactly (float)thr is a hit, and q - thr = 0 put a point 1e-10 below 0 one cell outside.
        const float px = thr * 1.000001f + 2.4e-7f * fabsf(qx), py = thr * 1.000001f + 2.4e-7f * fabsf(qy), pz = thr * 1.000001f + 2.4e-7f * fabsf(qz);
        const int x0 = (int)floorf((qx - px) * g.inv), x1 = (int)floorf((qx + px) * g.inv);
        const int y0 = (int)floorf((qy - py) * g.inv), y1 = (int)floorf((qy + py) * g.inv);
        const int z0 = (int)floorf((qz - pz) * g.inv), z1 = (int)floorf((qz + pz) * g.inv);
        // The query's own cell first, then the (up to seven) others of its +-thr box only while they can still hold a closer point:
        // a neighbouring cell lies behind the face it shares with the own cell, so the distance to that face (per axis that differs) bounds
        // every point of it from below.  Round 4: an inlier's nearest point is millimetres away and the faces are centimetres away, so ~1.5
        // instead of 8 cells are looked up and read (1.6 of the 1.9 GB a launch moved were the points of those cells).  The bound is
        // conservative -- the slack covers the rounding of floorf(x * inv) against the geometric face, which grows with the coordinate -- and
        // a cell is skipped only when its bound already reaches the best: the minimum is that of the full scan.
        const int hx = (int)floorf(qx * g.inv), hy = (int)floorf(qy * g.inv), hz = (int)floorf(qz * g.inv);
        auto scan_cell = [&](int ix, int iy, int iz) {
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
        auto face_gap = [&](int i, int hcell, float q) {   // distance from q to the face between its own cell and cell i on this axis (0: same cell)
            if (i == hcell) return 0.0f;
            const float face = (float)(i < hcell ? hcell : hcell + 1) * g.cell;
            return fmaxf(fabsf(q - face) - (1e-3f * g.cell + 5e-7f * fabsf(face)), 0.0f);
        };
        scan_cell(hx, hy, hz);
        for (int ix = x0; ix <= x1; ++ix) {
            const float gx = face_gap(ix, hx, qx);
            for (int iy = y0; iy <= y1; ++iy) {
                const float gy = face_gap(iy, hy, qy);
                for (int iz = z0; iz <= z1; ++iz) {
                    if (ix == hx && iy == hy && iz == hz) continue;
                    const float gz = face_gap(iz, hz, qz);
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
    std::vector<EvalJob> jobs(J);
    for (int j = 0; j < J; ++j) {
        for (int t = 0; t < 12; ++t) jobs[j].T[t] = T_global[16 * j + t];
        jobs[j].begin = job_begin[j]; jobs[j].end = job_end[j];
        if (job_end[j] < job_begin[j]) return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_batch: bad point range");
        jobs[j].out = j == 0 ? 0 : jobs[j - 1].out + (jobs[j - 1].end - jobs[j - 1].begin);
    }
    EvalJob* d_jobs; double* partial;
    IBL_ARENA(d_jobs, EvalJob, J);
    IBL_ARENA(partial, double, (int64_t)J * ICP_BPJ * 2);
    IBL_HIP_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(EvalJob) * J, hipMemcpyHostToDevice, s));
    const int prune = !ctx->diag.eval_fullscan;          // diagnostics: full scan = every cell of the query's box (the tests compare both)
    void* tok;
    ibl_prof_begin(IBL_PROF_ST_EVAL, 24.0 * (double)(jobs[J - 1].out + (jobs[J - 1].end - jobs[J - 1].begin)), s, &tok);
    // gridDim.y holds at most 65 535 rows: more jobs go in several launches.  A launch numbers its jobs from 0, so it is given its part
    // of the jobs and of the partials; job.out stays an offset into the whole of d2_out.
    const int max_rows = 65535;
    for (int j0 = 0; j0 < J; j0 += max_rows)
        hipLaunchKernelGGL(ibl_evaluate_kernel, dim3(ICP_BPJ, std::min(J - j0, max_rows)), dim3(256), 0, s, grid->v,
                           reinterpret_cast<const float4*>(det_pts4), d_jobs + j0, (float)threshold, (float)(threshold * threshold),
                           partial + (int64_t)j0 * ICP_BPJ * 2, d2_out, prune);
    ibl_prof_end(tok, s);
    IBL_LAUNCH_CHECK();
    std::vector<double> h((size_t)J * ICP_BPJ * 2);
    IBL_HIP_CHECK(hipMemcpyAsync(h.data(), partial, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    IBL_HIP_CHECK(hipStreamSynchronize(s));
    for (int j = 0; j < J; ++j) {
        double cnt = 0, err2 = 0;
        for (int b = 0; b < ICP_BPJ; ++b) { cnt += h[((size_t)j * ICP_BPJ + b) * 2]; err2 += h[((size_t)j * ICP_BPJ + b) * 2 + 1]; }
        const int ns = job_end[j] - job_begin[j];
        fitness_out[j] = ns > 0 ? cnt / (double)ns : 0.0;
        rmse_out[j] = cnt > 0 ? std::sqrt(err2 / cnt) : 0.0;
    }
    return IBL_OK;
}

// ------------------------------------------------------------------------------------------------
// association: which resident instances does a detection cloud overlap (ibl_memgrid_overlap)
// ------------------------------------------------------------------------------------------------
// hits(D, m) = #{ p in D : some point q of instance m has dist2f(p, q) < r2 }.  "Some point within r", not "the owner of the
// nearest point": a point that is near several instances counts for each of them, so no tie between instances decides a count.
#define AS_SEEN 8          // distinct instances a thread remembers in registers; further ones are deduplicated by a re-scan (exact)

// the cell index of key k, or -1: linear probing bounded by the table (an absent key ends at an empty slot; a full table cannot spin)
__device__ __forceinline__ int mg_find_cell(const MemGridView& g, unsigned long long k) {
    unsigned long long h = mg_hash(k) & g.hmask;
    for (unsigned long long probe = 0; probe <= g.hmask; ++probe) {
        const unsigned long long tk = g.tkeys[h];
        if (tk == k) return g.tvals[h];
        if (tk == MG_EMPTY) return -1;
        h = (h + 1) & g.hmask;
    }
    return -1;
}

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
        // The box: a hit has |q - m| < r (1 + 3 * 2^-24) per axis (the roundings of r2, of the difference and of its square), and
        // floorf(x * inv) is monotone in x, so the cells of q -+ pad bound the cell of every hit when pad exceeds that by more than
        // the rounding of the subtraction (half an ulp of q).
        const float px = thr * 1.000001f + 2.4e-7f * fabsf(qx), py = thr * 1.000001f + 2.4e-7f * fabsf(qy), pz = thr * 1.000001f + 2.4e-7f * fabsf(qz);
        const int x0 = (int)floorf((qx - px) * g.inv), x1 = (int)floorf((qx + px) * g.inv);
        const int y0 = (int)floorf((qy - py) * g.inv), y1 = (int)floorf((qy + py) * g.inv);
        const int z0 = (int)floorf((qz - pz) * g.inv), z1 = (int)floorf((qz + pz) * g.inv);
        int seen[AS_SEEN];
        int n_seen = 0;
        int* row = counts + (int64_t)d * n_inst;
        for (int ix = x0; ix <= x1; ++ix)
            for (int iy = y0; iy <= y1; ++iy)
                for (int iz = z0; iz <= z1; ++iz) {
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
                            for (int jx = x0; jx <= ix && !dup; ++jx)
                                for (int jy = y0; jy <= (jx < ix ? y1 : iy) && !dup; ++jy)
                                    for (int jz = z0; jz <= ((jx < ix || jy < iy) ? z1 : iz - 1) && !dup; ++jz) {
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
// the table probe is bounded (mg_find_cell).  The ten sums are reduced in the evaluation kernel's fixed order: no atomics.
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
        // the padded box of ibl_evaluate_kernel (see there)
        const float px = thr * 1.000001f + 2.4e-7f * fabsf(qx), py = thr * 1.000001f + 2.4e-7f * fabsf(qy), pz = thr * 1.000001f + 2.4e-7f * fabsf(qz);
        const int x0 = (int)floorf((qx - px) * g.inv), x1 = (int)floorf((qx + px) * g.inv);
        const int y0 = (int)floorf((qy - py) * g.inv), y1 = (int)floorf((qy + py) * g.inv);
        const int z0 = (int)floorf((qz - pz) * g.inv), z1 = (int)floorf((qz + pz) * g.inv);
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
        auto face_gap = [&](int i, int hcell, float q) {   // as in ibl_evaluate_kernel: a lower bound of the distance to cell i on this axis
            if (i == hcell) return 0.0f;
            const float face = (float)(i < hcell ? hcell : hcell + 1) * g.cell;
            return fmaxf(fabsf(q - face) - (1e-3f * g.cell + 5e-7f * fabsf(face)), 0.0f);
        };
        scan_cell(hx, hy, hz);
        for (int ix = x0; ix <= x1; ++ix) {
            const float gx = face_gap(ix, hx, qx);
            for (int iy = y0; iy <= y1; ++iy) {
                const float gy = face_gap(iy, hy, qy);
                for (int iz = z0; iz <= z1; ++iz) {
                    if (ix == hx && iy == hy && iz == hz) continue;
                    const float gz = face_gap(iz, hz, qz);
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
    std::vector<EvalJob> jobs(J);
    for (int j = 0; j < J; ++j) {
        for (int t = 0; t < 12; ++t) jobs[j].T[t] = T_global[16 * j + t];
        jobs[j].begin = job_begin[j]; jobs[j].end = job_end[j];
        if (job_begin[j] < 0 || job_end[j] < job_begin[j]) return ibl_set_error(IBL_ERR_ARG, "ibl_evaluate_information: bad point range");
        jobs[j].out = j == 0 ? 0 : jobs[j - 1].out + (jobs[j - 1].end - jobs[j - 1].begin);
    }
    const double ox = about ? about[0] : 0.0, oy = about ? about[1] : 0.0, oz = about ? about[2] : 0.0;
    EvalJob* d_jobs; double* partial;
    IBL_ARENA(d_jobs, EvalJob, J);
    IBL_ARENA(partial, double, (int64_t)J * ICP_BPJ * INFO_SUMS);
    IBL_HIP_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(EvalJob) * J, hipMemcpyHostToDevice, s));
    const int prune = !ctx->diag.eval_fullscan;
    std::vector<double> h((size_t)J * ICP_BPJ * INFO_SUMS);
    auto run = [&]() -> int {
        // at most 65 535 jobs per launch, as ibl_evaluate_batch: a launch gets its part of the jobs and of the partials
        const int max_rows = 65535;
        for (int j0 = 0; j0 < J; j0 += max_rows)
            hipLaunchKernelGGL(ibl_information_kernel, dim3(ICP_BPJ, std::min(J - j0, max_rows)), dim3(256), 0, s, grid->v,
                               reinterpret_cast<const float4*>(det_pts4), d_jobs + j0, (float)threshold, (float)(threshold * threshold), ox, oy, oz,
                               partial + (int64_t)j0 * ICP_BPJ * INFO_SUMS, reinterpret_cast<float4*>(nn_out), prune);
        IBL_LAUNCH_CHECK();
        IBL_HIP_CHECK(hipMemcpyAsync(h.data(), partial, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipStreamSynchronize(s));
        return IBL_OK;
    };
    const int st = run();
    if (st != IBL_OK) { (void)hipStreamSynchronize(s); return st; }      // (nothing queued may outlive the scratch or `jobs`)
    for (int j = 0; j < J; ++j) {
        double S[INFO_SUMS];
        for (int t = 0; t < INFO_SUMS; ++t) {
            S[t] = 0.0;
            for (int b = 0; b < ICP_BPJ; ++b) S[t] += h[((size_t)j * ICP_BPJ + b) * INFO_SUMS + t];
        }
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
