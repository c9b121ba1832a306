// reg_memgrid.h -- the whole-memory hash grid (ibl_memgrid) as its users see it: the view a kernel takes by value, the cell keys and
// the table probe, the padded box of a query and the face bound of a neighbouring cell.  reg_memgrid.hip builds and edits the grid,
// reg_eval.hip (evaluation, information matrix) and reg_assoc.hip (association) read it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "reg_common.h"

// what a kernel that reads the grid takes by value
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

// first index of the ascending vals[lo, hi) that is not below v
__device__ __forceinline__ int mg_bound_int(const int* __restrict__ vals, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (vals[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

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

// The cells [x0, x1] x [y0, y1] x [z0, z1] that can hold a point m with dist2f(q, m) < (float)(thr * thr).  Such a hit has
// |q - m| < thr (1 + 3 * 2^-24) per axis (the roundings of thr2, of the difference and of its square), not |q - m| < (float)thr: for
// a threshold whose float, squared in fp32, lies below thr2 (0.021, 0.036: not 0.02) a difference of exactly (float)thr is a hit,
// and q - thr = 0 put a point 1e-10 below 0 one cell outside.  floorf(x * inv) is monotone in x, so the cells of q -+ pad bound the
// cell of every hit when pad exceeds that by more than the rounding of the subtraction (half an ulp of q).
struct MgBox { int x0, x1, y0, y1, z0, z1; };
__device__ __forceinline__ MgBox mg_query_box(float inv, float qx, float qy, float qz, float thr) {
    const float px = thr * 1.000001f + 2.4e-7f * fabsf(qx), py = thr * 1.000001f + 2.4e-7f * fabsf(qy), pz = thr * 1.000001f + 2.4e-7f * fabsf(qz);
    return {(int)floorf((qx - px) * inv), (int)floorf((qx + px) * inv), (int)floorf((qy - py) * inv), (int)floorf((qy + py) * inv),
            (int)floorf((qz - pz) * inv), (int)floorf((qz + pz) * inv)};
}

// distance from q to the face between its own cell `hcell` and cell i on one axis (0: same cell), less a slack that covers the
// rounding of floorf(x * inv) against the geometric face, which grows with the coordinate: a lower bound for every point of cell i
__device__ __forceinline__ float mg_face_gap(int i, int hcell, float q, float cell) {
    if (i == hcell) return 0.0f;
    const float face = (float)(i < hcell ? hcell : hcell + 1) * cell;
    return fmaxf(fabsf(q - face) - (1e-3f * cell + 5e-7f * fabsf(face)), 0.0f);
}
