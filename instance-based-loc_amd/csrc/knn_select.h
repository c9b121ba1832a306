// knn_select.h -- the hybrid (radius + k-nearest) neighbour selection on the batch grids: everything a search needs and nothing a
// consumer owns.  Included by one .hip per consumer (reg_normals.hip, reg_fpfh.hip, reg_colorgrad.hip), each of which states its
// consumer, its factory and its launcher and so instantiates the tile and list kernels for exactly the factories it holds.
//
// Replaces Open3D's KDTreeSearchParamHybrid searches inside
//   estimate_normals / compute_fpfh_feature          (utils/fpfh_register.py:90-97)
//   InitializePointCloudForColoredICP                (registration_colored_icp, :132-135)
//
// One wavefront per query point.  The <= max_nn nearest candidates with d2 < r2 are selected without
// sorting and without storing the candidate list: pass 1 histograms the in-radius candidates over 256
// linear d2 bins (LDS, per wave), the bin holding the k-th neighbour is located with a wave scan,
// pass 2 hands every candidate of a lower bin straight to the consumer and parks only the boundary
// bin (<= 256 entries) in LDS, where the exact (d2, index) order decides the rest.  Candidate rows are
// contiguous runs of the cell-sorted point array, read as coalesced float4.  Memory-bound HIP: no
// MFMA here (normals+FPFH row, HBM roofline).
//
// The including .hip opens with `#pragma clang fp contract(off)` AHEAD of its includes: the library is compiled with -ffp-contract=on,
// and the fp64 sums of the consumers must not fuse (normals and histograms equal the oracle's bit for bit).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "reg_common.h"

#define KNN_BINS 256
#ifndef KNN_ROWS
#define KNN_ROWS 8        // candidate rows whose first 64 points are in flight together
#endif
#define KNN_CAPB 256
#ifndef KNN_TILE_CAP3
#define KNN_TILE_CAP3 1600     // candidates of a packed tile: 3 x (1 600 x 16 B + tables + 4 x 6.5 KB of wave scratch) fit a CU's 160 KB
#endif
#ifndef KNN_GUESS_SHIFT
#define KNN_GUESS_SHIFT 2      // margin of the threshold-bin guess: + 1 / 4 (12.5 % and 50 % measured 1 % slower)
#endif

// inclusive prefix sum over the 64 lanes on the DPP network (row_shr 1 / 2 / 4 / 8 inside the rows of 16, then row_bcast 15 and 31):
// six VALU instructions, no LDS -- the ds_bpermute form (__shfl_up) cost six LDS round trips, and a query runs three or four scans
__device__ __forceinline__ int wave_incl_scan_i(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct WaveLds {
    int hist[KNN_BINS];
    unsigned b_bits[KNN_CAPB];
    int b_idx[KNN_CAPB];
    int b_j[KNN_CAPB];
    int scratch[64];         // [0, 33) SPFH histogram, [62, 64) key range of the index sort
    int rank_pre[64];        // index sort: packed per-word bitmap prefixes
    int sel_j[256];          // consumers that do heavy per-neighbour work first compact the selected set here
    float sel_d2[256];
};

#ifdef KNN_LAB_CLK           // lab builds only: clocks of the phases of a tile's workgroup (thread 0), summed over the tiles.  Internal
                             // linkage: every object that includes this header carries its own counters, read by its own launch_knn
static __device__ unsigned long long knn_lab_clk[16];
#define KNN_CLK(k)                                                                            \
    do {                                                                                      \
        if (threadIdx.x == 0) {                                                               \
            const long long _t = (long long)__builtin_amdgcn_s_memtime();                     \
            atomicAdd(&knn_lab_clk[k], (unsigned long long)(_t - _clk_prev));                 \
            _clk_prev = _t;                                                                   \
        }                                                                                     \
    } while (0)
#else
#define KNN_CLK(k)
#endif

// A selected candidate is handed to the consumers as a HANDLE; the accessor turns it into the point and its original index.
//   GlobalAcc: handle = position in the cell-sorted point array (the per-query walk over the grid, hybrid_select)
//   TileAcc:   handle = slot of the workgroup's LDS-staged neighbourhood (tile_select)
struct GlobalAcc {
    const float4* sorted;
    const int* order;
    __device__ __forceinline__ float4 pt(int h) const { return sorted[h]; }
    __device__ __forceinline__ int ord(int h) const { return order[h]; }
};
struct TileAcc {
    const float4* pts;       // LDS
    const int* ordl;         // LDS, or null: the original index rides in the w component of the staged point (packed tiles)
    int key_base, key_span;  // the original indices of the tile's segment lie in [key_base, key_base + key_span)
    __device__ __forceinline__ float4 pt(int h) const { return pts[h]; }
    __device__ __forceinline__ int ord(int h) const { return ordl ? ordl[h] : __float_as_int(pts[h].w); }
};
// key range of the handles a consumer sorts by original index: known up front for a tile (its segment), found by a reduction otherwise
__device__ __forceinline__ bool key_range_hint(const GlobalAcc&, int*, unsigned*) { return false; }
__device__ __forceinline__ bool key_range_hint(const TileAcc& a, int* kmin, unsigned* span) { *kmin = a.key_base; *span = (unsigned)a.key_span; return true; }

// LDS-staged neighbourhood of one tile (a cube of ts^3 cells): every point of the cube of `rho` cells around the tile, copied once
// per workgroup and searched by all the tile's queries
#define KT_ROWS 144          // candidate rows (z, y) of the staging cube: (ts + 2 rho)^2 <= 144
// PACK: the consumer never reads a staged point's intensity (normals, SPFH: geometry only), so the point's original index is staged in
// its w component and the separate index array (4 B per candidate: 10 KB of the tile) goes -- with it and six waves per workgroup the
// 100-neighbour search keeps three waves per SIMD resident instead of two.
template <int KT_CAP, bool PACK = false>        // staged candidates
struct TileLds {
    static constexpr int CAP = KT_CAP;
    static constexpr bool PACKED = PACK;
    float4 pts[KT_CAP];
    int ord[PACK ? 1 : KT_CAP];
    int row_b[KT_ROWS];
    int row_off[KT_ROWS + 1];
    int q_b[16];
    int q_off[17];
    int next_q;              // the next query of the tile nobody has taken yet (tile_knn_block: waves take queries as they finish)
    __device__ __forceinline__ int ord_of(int t) const { return PACK ? __float_as_int(pts[t].w) : ord[t]; }
};

// ------------------------------------------------------------------------------------------------
// the per-query walk over the grid
// ------------------------------------------------------------------------------------------------
template <class Consumer>
__device__ void hybrid_select(const BatchGrid& g, const SegGrid sg, const float4 q, int qi, float radius, float r2, int max_nn,
                              WaveLds* L, Consumer& cons, int* status) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int reach_max = (int)ceilf(radius * sg.inv);
    if (reach_max < 1) reach_max = 1;
    const int cx = cell_clamp(q.x, sg.minx, sg.inv, sg.nx), cy = cell_clamp(q.y, sg.miny, sg.inv, sg.ny),
              cz = cell_clamp(q.z, sg.minz, sg.inv, sg.nz);
    const float bscale = (float)KNN_BINS / r2;

    // The grids are finer than the search radius (cell = radius / 3 .. radius / 5, reg_api.hip): with max_nn = 100 neighbours inside
    // r = 0.25 m a dense cloud (5 000 points on a 0.5 m object) has ALL its points in radius, and scanning them twice per query
    // was 90 % of the feature time.  The max_nn nearest are searched in the cube of `reach` cells around the query's cell first:
    // that cube holds every point closer than reach * cell, so once max_nn candidates lie inside that ball the cube's k nearest
    // are the cloud's k nearest (anything outside the cube is farther than all of them), and the result is the one of the full
    // radius, bit for bit.  reach starts at the first cube whose population (read from the cell table, no distances) promises
    // enough candidates and doubles when the ball count falls short.
    int reach = reach_max;
    for (int rho = 1; rho < reach_max; ++rho) {
        const int xa = max(cx - rho, 0), xb = min(cx + rho, sg.nx - 1);
        const int ya = max(cy - rho, 0), yb = min(cy + rho, sg.ny - 1);
        const int za = max(cz - rho, 0), zb = min(cz + rho, sg.nz - 1);
        const int nyr = yb - ya + 1, nr = nyr * (zb - za + 1);
        int pop = 0;
        for (int r = lane; r < nr; r += 64) {
            const int row = sg.cell_base + ((za + r / nyr) * sg.ny + ya + r % nyr) * sg.nx;
            pop += g.cell_start[row + xb + 1] - g.cell_start[row + xa];
        }
        pop = wave_sum_i(pop);
        // a ball of radius rho * cell covers ~1/3 (rho = 1) .. ~1/2 of the surface patch its cube cuts out
        if (pop >= (rho == 1 ? 3 : 2) * max_nn + 8) { reach = rho; break; }
    }
    int x0, x1, y0, y1, z0, z1, ny, nrows, my_b, my_e;
    auto set_reach = [&](int rho) {
        x0 = max(cx - rho, 0); x1 = min(cx + rho, sg.nx - 1);
        y0 = max(cy - rho, 0); y1 = min(cy + rho, sg.ny - 1);
        z0 = max(cz - rho, 0); z1 = min(cz + rho, sg.nz - 1);
        ny = y1 - y0 + 1; nrows = ny * (z1 - z0 + 1);
        my_b = my_e = 0;
        if (lane < nrows) {             // bounds of the first 64 candidate rows (runs of the cell-sorted point array, one per (z, y))
            const int row = sg.cell_base + ((z0 + lane / ny) * sg.ny + y0 + lane % ny) * sg.nx;
            my_b = g.cell_start[row + x0];
            my_e = g.cell_start[row + x1 + 1];
        }
    };
    // A wave's walk is a chain of dependent latencies (row bounds -> points -> next row), and these kernels are bound by it, so the
    // bounds of 64 rows are fetched in one step (lane r holds row r), empty rows are dropped by ballot, and the first 64 points of
    // KNN_ROWS rows at a time are in flight together.
    auto scan = [&](auto&& f) {
        for (int rc = 0; rc < nrows; rc += 64) {
            int cb = my_b, ce = my_e;
            if (rc > 0) {
                cb = ce = 0;
                const int r = rc + lane;
                if (r < nrows) {
                    const int row = sg.cell_base + ((z0 + r / ny) * sg.ny + y0 + r % ny) * sg.nx;
                    cb = g.cell_start[row + x0];
                    ce = g.cell_start[row + x1 + 1];
                }
            }
            unsigned long long live = __ballot(ce > cb);
            while (live) {
                int b[KNN_ROWS], e[KNN_ROWS];
                float4 p[KNN_ROWS];
#pragma unroll
                for (int u = 0; u < KNN_ROWS; ++u) {
                    const bool have = live != 0ull;
                    const int r = have ? __ffsll((long long)live) - 1 : 0;
                    if (have) live &= live - 1ull;
                    b[u] = __shfl(cb, r, 64);
                    e[u] = have ? __shfl(ce, r, 64) : b[u];
                    p[u] = b[u] + lane < e[u] ? g.sorted_pts[b[u] + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < KNN_ROWS; ++u) {
                    for (int jb = b[u]; jb < e[u]; jb += 64) {
                        const int j = jb + lane;
                        float4 q4 = p[u];
                        if (jb != b[u]) q4 = j < e[u] ? g.sorted_pts[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float d2 = j < e[u] ? dist2f(q.x, q.y, q.z, q4.x, q4.y, q4.z) : INFINITY;
                        f(d2 < r2, j, q4, d2);
                    }
                }
            }
        }
    };
    auto bin_of = [&](float d2) { int b = (int)(d2 * bscale); return b > KNN_BINS - 1 ? KNN_BINS - 1 : b; };

    // ---- pass 1: histogram (repeated on a larger cube while the ball inside the cube holds fewer than max_nn candidates) ------
    for (;;) {
        set_reach(reach);
#pragma unroll
        for (int t = 0; t < KNN_BINS / 64; ++t) L->hist[lane * (KNN_BINS / 64) + t] = 0;
        wave_lds_sync();
        // every point closer than (reach - 0.001) cells is inside the cube (the margin covers the rounding of the cell index)
        const float ball = ((float)reach - 1e-3f) / sg.inv;
        const float ball2 = reach < reach_max ? ball * ball : INFINITY;
        int in_ball = 0;
        scan([&](bool in, int, const float4&, float d2) {
            if (in) atomicAdd(&L->hist[bin_of(d2)], 1);
            in_ball += (in && d2 < ball2) ? 1 : 0;
        });
        wave_lds_sync();
        if (reach >= reach_max) break;
        if (wave_sum_i(in_ball) >= max_nn) break;
        reach = min(reach_max, 2 * reach);
        wave_lds_sync();
    }
    int hb[KNN_BINS / 64];
    int s = 0;
#pragma unroll
    for (int t = 0; t < KNN_BINS / 64; ++t) { hb[t] = L->hist[lane * (KNN_BINS / 64) + t]; s += hb[t]; }
    int incl = wave_incl_scan_i(s);
    const int cnt = __shfl(incl, 63, 64);
    const int excl = incl - s;
    const int k = cnt < max_nn ? cnt : max_nn;
    bool select_all = cnt <= max_nn;
    int bstar = KNN_BINS, n_below = 0, pop = 0;
    if (!select_all) {
        const unsigned long long m = __ballot(incl >= max_nn);
        const int Lc = __ffsll((long long)m) - 1;
        int bin_here = 0, my_below = 0, my_pop = 0;
        {
            int run = excl;
#pragma unroll
            for (int t = 0; t < KNN_BINS / 64; ++t) {
                if (my_pop == 0 && run + hb[t] >= max_nn) { bin_here = lane * (KNN_BINS / 64) + t; my_below = run; my_pop = hb[t]; }
                run += hb[t];
            }
        }
        bstar = __shfl(bin_here, Lc, 64);
        n_below = __shfl(my_below, Lc, 64);
        pop = __shfl(my_pop, Lc, 64);
    }
    cons.begin(k);

    // ---- pass 2: emit lower bins, park the boundary bin ---------------------------------------
    const bool fast = pop <= KNN_CAPB;
    int bcount = 0;
    scan([&](bool in, int j, const float4& p, float d2) {
        const int b = in ? bin_of(d2) : KNN_BINS;
        cons.accept(in && (select_all || b < bstar), j, p, d2);
        if (!select_all && fast) {
            const bool park = in && b == bstar;
            const unsigned long long m = __ballot(park);
            if (park) {
                const int pos = bcount + __popcll(m & lt_mask);
                L->b_bits[pos] = __float_as_uint(d2);
                L->b_idx[pos] = g.order[j];
                L->b_j[pos] = j;
            }
            bcount += __popcll(m);
        }
    });
    if (!select_all) {
        const int need = max_nn - n_below;
        if (fast) {
            wave_lds_sync();
            unsigned eb[KNN_CAPB / 64];
            int ei[KNN_CAPB / 64];
            bool ev[KNN_CAPB / 64];
#pragma unroll
            for (int t = 0; t < KNN_CAPB / 64; ++t) {
                const int e = lane + 64 * t;
                ev[t] = e < pop;
                eb[t] = ev[t] ? L->b_bits[e] : 0xFFFFFFFFu;
                ei[t] = ev[t] ? L->b_idx[e] : 0x7FFFFFFF;
            }
            unsigned lo = 0, hi = 0x7F800000u;
            while (lo < hi) {
                const unsigned mid = lo + ((hi - lo) >> 1);
                int c = 0;
#pragma unroll
                for (int t = 0; t < KNN_CAPB / 64; ++t) c += __popcll(__ballot(ev[t] && eb[t] <= mid));
                if (c >= need) hi = mid; else lo = mid + 1;
            }
            const unsigned T = lo;
            int cl = 0, ct = 0;
#pragma unroll
            for (int t = 0; t < KNN_CAPB / 64; ++t) { cl += __popcll(__ballot(ev[t] && eb[t] < T)); ct += __popcll(__ballot(ev[t] && eb[t] == T)); }
            const int need2 = need - cl;
            int I = 0x7FFFFFFF;
            if (ct > need2) {
                int ilo = 0, ihi = 0x7FFFFFFF;
                while (ilo < ihi) {
                    const int mid = ilo + ((ihi - ilo) >> 1);
                    int c = 0;
#pragma unroll
                    for (int t = 0; t < KNN_CAPB / 64; ++t) c += __popcll(__ballot(ev[t] && eb[t] == T && ei[t] <= mid));
                    if (c >= need2) ihi = mid; else ilo = mid + 1;
                }
                I = ilo;
            }
#pragma unroll
            for (int t = 0; t < KNN_CAPB / 64; ++t) {
                const bool sel = ev[t] && (eb[t] < T || (eb[t] == T && ei[t] <= I));
                int j = 0;
                float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
                if (sel) { j = L->b_j[lane + 64 * t]; p = g.sorted_pts[j]; }
                cons.accept(sel, j, p, __uint_as_float(eb[t]));
            }
        } else {
            // boundary bin larger than the LDS list (many near-equidistant candidates): exact thresholds by
            // re-scanning the candidates -- slow, correct, flagged in the status word
            if (lane == 0) atomicOr(status, IBL_ST_KNN_SLOWPATH);
            unsigned lo = 0, hi = 0x7F800000u;
            while (lo < hi) {
                const unsigned mid = lo + ((hi - lo) >> 1);
                int c = 0;
                scan([&](bool in, int, const float4&, float d2) {
                    c += (in && bin_of(d2) == bstar && __float_as_uint(d2) <= mid) ? 1 : 0;
                });
                c = wave_sum_i(c);
                if (c >= need) hi = mid; else lo = mid + 1;
            }
            const unsigned T = lo;
            int cl = 0, ct = 0;
            scan([&](bool in, int, const float4&, float d2) {
                const bool bb = in && bin_of(d2) == bstar;
                cl += (bb && __float_as_uint(d2) < T) ? 1 : 0;
                ct += (bb && __float_as_uint(d2) == T) ? 1 : 0;
            });
            cl = wave_sum_i(cl); ct = wave_sum_i(ct);
            const int need2 = need - cl;
            int I = 0x7FFFFFFF;
            if (ct > need2) {
                int ilo = 0, ihi = 0x7FFFFFFF;
                while (ilo < ihi) {
                    const int mid = ilo + ((ihi - ilo) >> 1);
                    int c = 0;
                    scan([&](bool in, int j, const float4&, float d2) {
                        if (in && bin_of(d2) == bstar && __float_as_uint(d2) == T) c += (g.order[j] <= mid) ? 1 : 0;
                    });
                    c = wave_sum_i(c);
                    if (c >= need2) ihi = mid; else ilo = mid + 1;
                }
                I = ilo;
            }
            scan([&](bool in, int j, const float4& p, float d2) {
                bool sel = false;
                if (in && bin_of(d2) == bstar) {
                    const unsigned bits = __float_as_uint(d2);
                    sel = bits < T || (bits == T && g.order[j] <= I);
                }
                cons.accept(sel, j, p, d2);
            });
        }
    }
    cons.finish(k);
}

// ------------------------------------------------------------------------------------------------
// what every consumer does first: its selected neighbours in ascending original index
// ------------------------------------------------------------------------------------------------
// The selected neighbours arrive in the enumeration order of the grid.  Consumers reduce them in ascending ORIGINAL
// point index instead (rank sort of the <= 256 list entries in LDS), so that every floating-point sum is independent
// of the grid a cloud was enumerated from: features of an instance computed on its own (ibl_instance_features_batch)
// are bit-identical to those computed inside a concatenation whose other instances are out of reach.
// in: L->sel_j[0..k) (+ sel_d2); out: L->b_j[0..k) (+ b_bits = d2 bits) in ascending order[j].
template <bool WITH_D2, class Acc>
__device__ __forceinline__ void sort_selected_by_index(WaveLds* L, const Acc& acc, int k) {
    const int lane = threadIdx.x & 63;
    int kmin;
    unsigned span;
    if (key_range_hint(acc, &kmin, &span) && span <= 32u * KNN_BINS) {
        // a tile: every key lies in its segment's index range -- no reduction (64 lanes' atomicMin / atomicMax on one LDS word serialised)
        for (int t = lane; t < k; t += 64) L->b_idx[t] = acc.ord(L->sel_j[t]);
        if (span > 0) --span;
        wave_lds_sync();
    } else {
        int mn = 0x7FFFFFFF, mx = -1;
        for (int t = lane; t < k; t += 64) {
            const int key = acc.ord(L->sel_j[t]);
            L->b_idx[t] = key;
            mn = min(mn, key);
            mx = max(mx, key);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { mn = min(mn, __shfl_xor(mn, off, 64)); mx = max(mx, __shfl_xor(mx, off, 64)); }
        kmin = mn;
        span = (unsigned)(mx - mn);
        wave_lds_sync();
    }
    if (span < 32u * KNN_BINS) {
        // the keys are distinct original indices: rank = number of set bits below the key's bit in a bitmap of the span
        // (L->hist is free once the selection is over); per-word exclusive prefixes fit a byte (rank < k <= 256)
        unsigned* bits = reinterpret_cast<unsigned*>(L->hist);
        *reinterpret_cast<uint4*>(&bits[4 * lane]) = make_uint4(0u, 0u, 0u, 0u);
        wave_lds_sync();
        for (int t = lane; t < k; t += 64) {
            const unsigned o = (unsigned)(L->b_idx[t] - kmin);
            atomicOr(&bits[o >> 5], 1u << (o & 31u));
        }
        wave_lds_sync();
        const uint4 w = *reinterpret_cast<const uint4*>(&bits[4 * lane]);
        const int c0 = __popc(w.x), c1 = __popc(w.y), c2 = __popc(w.z), c3 = __popc(w.w);
        const int s = c0 + c1 + c2 + c3;
        int incl = wave_incl_scan_i(s);
        const unsigned e0 = (unsigned)(incl - s), e1 = e0 + c0, e2 = e1 + c1, e3 = e2 + c2;
        reinterpret_cast<unsigned*>(L->rank_pre)[lane] = (e0 & 255u) | ((e1 & 255u) << 8) | ((e2 & 255u) << 16) | ((e3 & 255u) << 24);
        wave_lds_sync();
        const unsigned char* pre = reinterpret_cast<const unsigned char*>(L->rank_pre);
        for (int t = lane; t < k; t += 64) {
            const unsigned o = (unsigned)(L->b_idx[t] - kmin);
            const int r = (int)pre[o >> 5] + __popc(bits[o >> 5] & ((1u << (o & 31u)) - 1u));
            L->b_j[r] = L->sel_j[t];
            if (WITH_D2) L->b_bits[r] = __float_as_uint(L->sel_d2[t]);
        }
    } else {
        for (int t = lane; t < k; t += 64) {
            const int key = L->b_idx[t];
            int r = 0;
            for (int u = 0; u < k; ++u) r += L->b_idx[u] < key ? 1 : 0;
            L->b_j[r] = L->sel_j[t];
            if (WITH_D2) L->b_bits[r] = __float_as_uint(L->sel_d2[t]);
        }
    }
    wave_lds_sync();
}

// ------------------------------------------------------------------------------------------------
// the search on an LDS-staged neighbourhood
// ------------------------------------------------------------------------------------------------
// One wavefront, one query, `total` candidates in T (every point of the staging cube).  cover2 = squared distance from the query to
// the nearest face of the staging cube (INFINITY when the cube reaches past the search radius or the cloud's bounds on every side):
// all points closer than that are staged, so once max_nn of them are, the staged k nearest are the cloud's k nearest.  Returns
// false -- before any consumer call -- when that cannot be shown or the boundary bin overflows its list; the caller then runs
// hybrid_select for the query.  Selection rule and tie order (d2 bits, then original index) are those of hybrid_select.
#ifdef KNN_LAB_STATS
static __device__ int knn_lab_stats[8];      // (internal linkage: see knn_lab_clk)
#endif

// Round 3 fast path of tile_select: with a GUESS of the squared distance of the query's max_nn-th neighbour (the previous query of this
// wave -- a neighbour in the same tile -- plus a margin) ONE pass over the staged candidates collects those closer than the guess (two
// ballots and two LDS stores per 64 candidates: no histogram, no bins, no atomics in the pass that touches every candidate; it was 8 200
// of a query's 24 000 clocks).  The list then holds every staged candidate with d2 < guess; when it has at least max_nn entries (and at
// most the 256 the list holds) the max_nn nearest are among them -- anything outside is strictly farther -- and are selected from the
// list alone through a 256-bin histogram of the LIST over [0, guess): the same candidates, the same (d2 bits, original index) order as
// the two-pass selection below.  Returns 1 = done, 0 = not provable from the staged cube (the query joins the grid walk), -1 = the
// guess was too small or too large (the caller runs the two-pass selection, which also renews the guess).
template <class TL, class Consumer>
__device__ int tile_select_guess(const TL& T, int total, const float4 q, float cover2, float r2, int max_nn, WaveLds* L, Consumer& cons, float& gthr) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const float thr = fminf(gthr, r2);
#ifdef KNN_LAB_CLK
    long long _clk_prev = (long long)__builtin_amdgcn_s_memtime();
#endif
    int ccount = 0, in_ball = 0;
    // 128 candidates per step, both LDS reads of the NEXT step in flight while this one is evaluated (the pass is a chain of LDS round
    // trips otherwise: two waves per SIMD do not hide them)
    const int last = total - 1;
    float4 pa = T.pts[min(lane, last)], pb = T.pts[min(lane + 64, last)];
#pragma unroll 1
    for (int t0 = 0; t0 < total; t0 += 128) {
        const float4 p0 = pa, p1 = pb;
        pa = T.pts[min(t0 + 128 + lane, last)];
        pb = T.pts[min(t0 + 192 + lane, last)];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = t0 + 64 * h + lane;
            const float4 p = h ? p1 : p0;
            const float d2 = dist2f(q.x, q.y, q.z, p.x, p.y, p.z);
            const bool valid = t < total;
            in_ball += __popcll(__ballot(valid && d2 < cover2));
            const bool col = valid && d2 < thr;
            const unsigned long long mc = __ballot(col);
            if (col) {
                const int pos = ccount + __popcll(mc & lt_mask);
                if (pos < KNN_CAPB) { L->b_j[pos] = t; L->b_bits[pos] = __float_as_uint(d2); }
            }
            ccount += __popcll(mc);
        }
    }
    KNN_CLK(8);
    if (cover2 != INFINITY && in_ball < max_nn) return 0;
    if (ccount > KNN_CAPB || (ccount < max_nn && thr < r2)) return -1;
    wave_lds_sync();
    const int k = ccount < max_nn ? ccount : max_nn;
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    // the list, four entries per lane
    unsigned eb[KNN_CAPB / 64];
    int et[KNN_CAPB / 64];
#pragma unroll
    for (int u = 0; u < KNN_CAPB / 64; ++u) {
        const int e = lane + 64 * u;
        eb[u] = e < ccount ? L->b_bits[e] : 0xFFFFFFFFu;
        et[u] = e < ccount ? L->b_j[e] : 0;
    }
    if (ccount <= max_nn) {                         // (thr == r2 here: the list is every staged candidate in radius)
        cons.begin(k);                              // (a consumer with an inner set finds it itself on this rare path)
#pragma unroll
        for (int u = 0; u < KNN_CAPB / 64; ++u) cons.accept(lane + 64 * u < ccount, et[u], none, __uint_as_float(eb[u]));
        cons.finish(k);
        return 1;
    }
    const float lscale = (float)KNN_BINS / thr;
    int ebin[KNN_CAPB / 64];
#pragma unroll
    for (int t = 0; t < KNN_BINS / 64; ++t) L->hist[lane * (KNN_BINS / 64) + t] = 0;
    wave_lds_sync();
#pragma unroll
    for (int u = 0; u < KNN_CAPB / 64; ++u) {
        const bool v = lane + 64 * u < ccount;
        ebin[u] = v ? (int)fminf(__uint_as_float(eb[u]) * lscale, (float)(KNN_BINS - 1)) : KNN_BINS;
        if (v) atomicAdd(&L->hist[ebin[u]], 1);
    }
    wave_lds_sync();
    int hb[KNN_BINS / 64];
    int s = 0;
#pragma unroll
    for (int t = 0; t < KNN_BINS / 64; ++t) { hb[t] = L->hist[lane * (KNN_BINS / 64) + t]; s += hb[t]; }
    int incl = wave_incl_scan_i(s);
    int bstar, n_below, pop;
    {
        const unsigned long long m = __ballot(incl >= max_nn);
        const int Lc = __ffsll((long long)m) - 1;
        int bin_here = 0, my_below = 0, my_pop = 0;
        int run = incl - s;
#pragma unroll
        for (int t = 0; t < KNN_BINS / 64; ++t) {
            if (my_pop == 0 && run + hb[t] >= max_nn) { bin_here = lane * (KNN_BINS / 64) + t; my_below = run; my_pop = hb[t]; }
            run += hb[t];
        }
        bstar = __shfl(bin_here, Lc, 64);
        n_below = __shfl(my_below, Lc, 64);
        pop = __shfl(my_pop, Lc, 64);
    }
    // The inner set of a consumer that wants one (the normal's <= kn nearest inside rn2): {d2 < rn2} is a prefix of the (d2, index) order
    // and so is the selection, hence n_in = min(k, list entries inside rn2); when n_in <= kn every selected entry inside rn2 belongs to
    // it, otherwise the kn first of the order do: the bins below the one that holds the kn-th entry + that bin's entries by rank.
    bool inner[KNN_CAPB / 64];
    bool use_flags = false;
    if constexpr (Consumer::WANTS_INNER) {
        const float rn2 = cons.rn2;
        const int kn = cons.kn;
        int n_in_list = 0;
#pragma unroll
        for (int u = 0; u < KNN_CAPB / 64; ++u) {
            inner[u] = lane + 64 * u < ccount && __uint_as_float(eb[u]) < rn2;
            n_in_list += __popcll(__ballot(inner[u]));
        }
        use_flags = true;
        if ((n_in_list < k ? n_in_list : k) > kn) {
            const unsigned long long m = __ballot(incl >= kn);
            const int Lc = __ffsll((long long)m) - 1;
            int bin_here = 0, my_below = 0, my_pop = 0;
            int run = incl - s;
#pragma unroll
            for (int t = 0; t < KNN_BINS / 64; ++t) {
                if (my_pop == 0 && run + hb[t] >= kn) { bin_here = lane * (KNN_BINS / 64) + t; my_below = run; my_pop = hb[t]; }
                run += hb[t];
            }
            const int b30 = __shfl(bin_here, Lc, 64);
            const int need30 = kn - __shfl(my_below, Lc, 64);
            const int pop30 = __shfl(my_pop, Lc, 64);
            if (pop30 > 64) use_flags = false;          // (the consumer finds its inner set itself)
            else {
                // the kn-th entry's bin: its entries by (d2 bits, original index), parked in the idle sort scratch
                int c30 = 0;
#pragma unroll
                for (int u = 0; u < KNN_CAPB / 64; ++u) {
                    const bool pk = ebin[u] == b30;
                    const unsigned long long mp = __ballot(pk);
                    if (pk) {
                        const int pos = c30 + __popcll(mp & lt_mask);
                        L->rank_pre[pos] = (int)eb[u];
                        L->scratch[pos] = T.ord_of(et[u]);
                    }
                    c30 += __popcll(mp);
                }
                wave_lds_sync();
#pragma unroll
                for (int u = 0; u < KNN_CAPB / 64; ++u) {
                    if (ebin[u] < b30) inner[u] = true;
                    else if (ebin[u] > b30) inner[u] = false;
                    else {
                        const int mi = T.ord_of(et[u]);
                        int rank = 0;
                        for (int w = 0; w < pop30; ++w) {
                            const unsigned ub = (unsigned)L->rank_pre[w];
                            rank += (ub < eb[u] || (ub == eb[u] && L->scratch[w] < mi)) ? 1 : 0;
                        }
                        inner[u] = rank < need30;
                    }
                }
                wave_lds_sync();
            }
        }
    }
    KNN_CLK(9);
    cons.begin(k);
    // entries below the threshold bin go to the consumer; the threshold bin's entries are parked at the head of the list arrays (every
    // lane holds its entries in registers by now)
    int bcount = 0;
#pragma unroll
    for (int u = 0; u < KNN_CAPB / 64; ++u) {
        if constexpr (Consumer::WANTS_INNER) {
            if (use_flags) cons.accept_in(ebin[u] < bstar, et[u], __uint_as_float(eb[u]), inner[u]);
            else cons.accept(ebin[u] < bstar, et[u], none, __uint_as_float(eb[u]));
        } else
        cons.accept(ebin[u] < bstar, et[u], none, __uint_as_float(eb[u]));
        const bool park = ebin[u] == bstar;
        const unsigned long long m = __ballot(park);
        if (park) {
            const int pos = bcount + __popcll(m & lt_mask);
            L->b_bits[pos] = eb[u];
            L->b_idx[pos] = T.ord_of(et[u]);
            bool fl = false;
            if constexpr (Consumer::WANTS_INNER) fl = use_flags && inner[u];
            L->b_j[pos] = et[u] | (fl ? 0x40000000 : 0);        // (bit 30: inner flag of a parked entry)
        }
        bcount += __popcll(m);
    }
    KNN_CLK(10);
    const int need = max_nn - n_below;
    wave_lds_sync();
    for (int e0 = 0; e0 < pop; e0 += 64) {
        const int e = e0 + lane;
        const bool v = e < pop;
        const unsigned mb = v ? L->b_bits[e] : 0xFFFFFFFFu;
        const int mi = v ? L->b_idx[e] : 0x7FFFFFFF;
        int rank = 0;
        for (int u = 0; u < pop; ++u) {
            const unsigned ub = L->b_bits[u];
            const int ui = L->b_idx[u];
            rank += (ub < mb || (ub == mb && ui < mi)) ? 1 : 0;
        }
        const int hj = v ? L->b_j[e] : 0;
        if constexpr (Consumer::WANTS_INNER) {
            if (use_flags) cons.accept_in(v && rank < need, hj & 0x3FFFFFFF, __uint_as_float(mb), (hj & 0x40000000) != 0);
            else cons.accept(v && rank < need, hj & 0x3FFFFFFF, none, __uint_as_float(mb));
        } else
        cons.accept(v && rank < need, hj & 0x3FFFFFFF, none, __uint_as_float(mb));
    }
    KNN_CLK(11);
    // next guess: the upper edge of the threshold bin + a margin (a 30-neighbour search has 8x head-room in the 256-entry list)
    gthr = fminf(r2, (float)(bstar + 1) / lscale * (max_nn * 4 <= KNN_CAPB ? 2.0f : 1.3f));
    cons.finish(k);
    KNN_CLK(12);
    return 1;
}

template <class TL, class Consumer>
__device__ bool tile_select(const TL& T, int total, const float4 q, float cover2, float r2, int max_nn, WaveLds* L, Consumer& cons, int& gbin) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const float bscale = (float)KNN_BINS / r2;
    auto bin_of = [&](float d2) { int b = (int)(d2 * bscale); return b > KNN_BINS - 1 ? KNN_BINS - 1 : b; };
#ifdef KNN_LAB_CLK
    long long _clk_prev = (long long)__builtin_amdgcn_s_memtime();
#endif
#pragma unroll
    for (int t = 0; t < KNN_BINS / 64; ++t) L->hist[lane * (KNN_BINS / 64) + t] = 0;
    wave_lds_sync();
    int in_ball = 0;
    // While the histogram is built, the candidates up to a GUESS of the threshold bin (the previous query of this wave, a neighbour in
    // the same tile, + 25 %) are parked in the boundary arrays, which are idle until the second pass.  When the guess covers the true
    // threshold bin and the list did not overflow, the selection below runs over that list (<= 256 entries) instead of all the staged
    // candidates a second time (~1 200): the same candidates in the same (d2 bits, index) order either way.
    const int guess = gbin;
    int ccount = 0;
    float4 pnext = T.pts[lane < total ? lane : 0];        // one step ahead: two waves per SIMD do not hide the LDS round trip
#pragma unroll 1
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        const float4 p = pnext;
        if (t0 + 64 < total) pnext = T.pts[t + 64 < total ? t + 64 : 0];
        const float d2 = dist2f(q.x, q.y, q.z, p.x, p.y, p.z);
        const bool in = t < total && d2 < r2;
        const int b = in ? bin_of(d2) : KNN_BINS;
        if (in) atomicAdd(&L->hist[b], 1);
        in_ball += __popcll(__ballot(in && d2 < cover2));
        const bool col = b <= guess;
        const unsigned long long mc = __ballot(col);
        if (col) {
            const int pos = ccount + __popcll(mc & lt_mask);
            if (pos < KNN_CAPB) { L->b_j[pos] = t; L->b_bits[pos] = __float_as_uint(d2); }
        }
        ccount += __popcll(mc);
    }
    wave_lds_sync();
    KNN_CLK(8);
    int hb[KNN_BINS / 64];
    int s = 0;
#pragma unroll
    for (int t = 0; t < KNN_BINS / 64; ++t) { hb[t] = L->hist[lane * (KNN_BINS / 64) + t]; s += hb[t]; }
    int incl = wave_incl_scan_i(s);
    const int cnt = __shfl(incl, 63, 64);
    if (cover2 != INFINITY && in_ball < max_nn) return false;
    const int excl = incl - s;
    const int k = cnt < max_nn ? cnt : max_nn;
    const bool select_all = cnt <= max_nn;
    int bstar = KNN_BINS, n_below = 0, pop = 0;
    if (!select_all) {
        const unsigned long long m = __ballot(incl >= max_nn);
        const int Lc = __ffsll((long long)m) - 1;
        int bin_here = 0, my_below = 0, my_pop = 0;
        int run = excl;
#pragma unroll
        for (int t = 0; t < KNN_BINS / 64; ++t) {
            if (my_pop == 0 && run + hb[t] >= max_nn) { bin_here = lane * (KNN_BINS / 64) + t; my_below = run; my_pop = hb[t]; }
            run += hb[t];
        }
        bstar = __shfl(bin_here, Lc, 64);
        n_below = __shfl(my_below, Lc, 64);
        pop = __shfl(my_pop, Lc, 64);
        if (pop > KNN_CAPB) return false;
        // (a 30-neighbour search has 8x head-room in the 256-entry list: its guess doubles the bin instead of adding a quarter)
        gbin = min(KNN_BINS - 1, bstar + (max_nn * 4 <= KNN_CAPB ? bstar : (bstar >> KNN_GUESS_SHIFT)) + 2);
    }
    cons.begin(k);
    KNN_CLK(9);
    int bcount = 0;
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool from_list = !select_all && bstar <= guess && ccount <= KNN_CAPB;
#ifdef KNN_LAB_STATS
    if (lane == 0) { atomicAdd(&knn_lab_stats[0], 1); if (from_list) atomicAdd(&knn_lab_stats[1], 1); if (select_all) atomicAdd(&knn_lab_stats[2], 1); if (!select_all && bstar > guess) atomicAdd(&knn_lab_stats[3], 1); if (ccount > KNN_CAPB) atomicAdd(&knn_lab_stats[4], 1); }
#endif
    if (from_list) {
#pragma unroll 1
        for (int e0 = 0; e0 < ccount; e0 += 64) {
            const int e = e0 + lane;
            const bool v = e < ccount;
            const int t = v ? L->b_j[e] : 0;
            const unsigned bits = v ? L->b_bits[e] : 0u;
            const float d2 = __uint_as_float(bits);
            const int b = v ? bin_of(d2) : KNN_BINS;
            cons.accept(b < bstar, t, none, d2);
            // the boundary bin is compacted in place: a parked entry lands at or before the slot it was read from, and every lane of
            // this step has read its slot before the first store is issued
            const bool park = b == bstar;
            const unsigned long long m = __ballot(park);
            if (park) {
                const int pos = bcount + __popcll(m & lt_mask);
                L->b_bits[pos] = bits;
                L->b_idx[pos] = T.ord_of(t);
                L->b_j[pos] = t;
            }
            bcount += __popcll(m);
        }
    } else
#pragma unroll 1
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        const float4 p = T.pts[t < total ? t : 0];
        const float d2 = dist2f(q.x, q.y, q.z, p.x, p.y, p.z);        // the same bits as in pass 1
        const bool in = t < total && d2 < r2;
        const int b = in ? bin_of(d2) : KNN_BINS;
        cons.accept(in && (select_all || b < bstar), t, none, d2);
        if (!select_all) {
            const bool park = in && b == bstar;
            const unsigned long long m = __ballot(park);
            if (park) {
                const int pos = bcount + __popcll(m & lt_mask);
                L->b_bits[pos] = __float_as_uint(d2);
                L->b_idx[pos] = T.ord_of(t);
                L->b_j[pos] = t;
            }
            bcount += __popcll(m);
        }
    }
    KNN_CLK(10);
    if (!select_all) {
        // the boundary bin: an entry is selected when fewer than `need` entries precede it in (d2 bits, original index) order
        const int need = max_nn - n_below;
        wave_lds_sync();
        for (int e0 = 0; e0 < pop; e0 += 64) {
            const int e = e0 + lane;
            const bool v = e < pop;
            const unsigned mb = v ? L->b_bits[e] : 0xFFFFFFFFu;
            const int mi = v ? L->b_idx[e] : 0x7FFFFFFF;
            int rank = 0;
            for (int u = 0; u < pop; ++u) {
                const unsigned ub = L->b_bits[u];
                const int ui = L->b_idx[u];
                rank += (ub < mb || (ub == mb && ui < mi)) ? 1 : 0;
            }
            const bool sel = v && rank < need;
            cons.accept(sel, v ? L->b_j[e] : 0, none, __uint_as_float(mb));
        }
    }
    KNN_CLK(11);
    cons.finish(k);
    KNN_CLK(12);
    return true;
}

// Workgroup per tile: stage the neighbourhood, then every wavefront takes queries of the tile in turn.  need_pop[rho] = candidates
// the staging cube of reach rho should hold for the ball inside it to contain max_nn of them (host: 1.15 max_nn (ts + 2 rho)^2 /
// (pi rho^2)); the reach grows from 2 until it does, the cube fills the LDS budget or covers the whole radius.
struct NeedPop { float v[8]; int rho_start; int guess; };       // guess: tile_select_guess on (0: IBL_KNN_NOGUESS=1, the two-pass selection only)
// Factory::Pending of a consumer that parks nothing between queries (the tile's per-wave slot keeps only its counter)
struct NoPending { int n; };

template <int TS, int NW, class TL, class Factory>
__device__ void tile_knn_block(const BatchGrid& g, float radius, float r2, int max_nn, const NeedPop& need_pop, int* __restrict__ fb_list,
                               int* __restrict__ fb_count, const Factory& fac, int q_lo, int q_hi, TL& T, WaveLds* wl,
                               typename Factory::Pending* pend) {
    constexpr int KT_CAP = TL::CAP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    if (tile >= g.n_tiles) return;
#ifdef KNN_LAB_CLK
    long long _clk_prev = (long long)__builtin_amdgcn_s_memtime();
#endif
    int lo = 0, hi = g.n_seg;                      // the segment whose tile range holds `tile`
    if (g.tile_seg) lo = g.tile_seg[tile];
    else
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (g.tile_base[mid] <= tile) lo = mid; else hi = mid;
        }
    const SegGrid sg = g.seg[lo];
    const int ntx = (sg.nx + TS - 1) / TS, nty = (sg.ny + TS - 1) / TS;
    int tt = tile - g.tile_base[lo];
    const int tx = tt % ntx; tt /= ntx;
    const int ty = tt % nty, tz = tt / nty;
    const int cx0 = tx * TS, cx1 = min(cx0 + TS, sg.nx) - 1;
    const int cy0 = ty * TS, cy1 = min(cy0 + TS, sg.ny) - 1;
    const int cz0 = tz * TS, cz1 = min(cz0 + TS, sg.nz) - 1;
    // the tile's queries: runs of the cell-sorted array, one per (z, y) row of the tile
    const int qny = cy1 - cy0 + 1, qrows = qny * (cz1 - cz0 + 1);
    if (tid < qrows) {
        const int row = sg.cell_base + ((cz0 + tid / qny) * sg.ny + cy0 + tid % qny) * sg.nx;
        const int b = g.cell_start[row + cx0];
        T.q_b[tid] = b;
        T.q_off[tid + 1] = g.cell_start[row + cx1 + 1] - b;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        T.q_off[0] = 0;
        for (int r = 0; r < qrows; ++r) { acc += T.q_off[r + 1]; T.q_off[r + 1] = acc; }
        T.next_q = NW;
    }
    __syncthreads();
    const int nq = T.q_off[qrows];
    KNN_CLK(0);
    if (nq == 0) return;

    int reach_max = (int)ceilf(radius * sg.inv);
    if (reach_max < 1) reach_max = 1;
    const int rho_cap = min(reach_max, TS <= 2 ? 5 : 4);            // (TS + 2 rho)^2 <= KT_ROWS
    int rho = min(need_pop.rho_start, rho_cap);
    int x0, x1, y0, y1, z0, z1, total = 0;
    bool staged = false, final_try = false;
    for (int it = 0; it < 8; ++it) {
        x0 = max(cx0 - rho, 0); x1 = min(cx1 + rho, sg.nx - 1);
        y0 = max(cy0 - rho, 0); y1 = min(cy1 + rho, sg.ny - 1);
        z0 = max(cz0 - rho, 0); z1 = min(cz1 + rho, sg.nz - 1);
        const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
        __syncthreads();                              // row tables of the previous attempt are no longer read
        if (tid < nrows) {
            const int row = sg.cell_base + ((z0 + tid / ny) * sg.ny + y0 + tid % ny) * sg.nx;
            const int b = g.cell_start[row + x0];
            T.row_b[tid] = b;
            T.row_off[tid + 1] = g.cell_start[row + x1 + 1] - b;
        }
        __syncthreads();
        if (wave == 0) {                              // exclusive prefix of <= 144 row lengths: three per lane + a wave scan
            int v[3], sum = 0;
#pragma unroll
            for (int u = 0; u < 3; ++u) { const int r = 3 * lane + u; v[u] = r < nrows ? T.row_off[r + 1] : 0; sum += v[u]; }
            int incl = wave_incl_scan_i(sum);
            int run = incl - sum;
            if (lane == 0) T.row_off[0] = 0;
#pragma unroll
            for (int u = 0; u < 3; ++u) { const int r = 3 * lane + u; run += v[u]; if (r < nrows) T.row_off[r + 1] = run; }
        }
        __syncthreads();
        total = T.row_off[nrows];
        if (total > KT_CAP) {
            if (rho > 1 && !final_try) { --rho; final_try = true; continue; }
            break;                                     // does not fit at any reach: every query takes the global walk
        }
        if (final_try || rho >= rho_cap || (float)total >= need_pop.v[rho]) { staged = true; break; }
        ++rho;
    }
    const float cellw = 1.0f / sg.inv;
    KNN_CLK(1);
    if (staged) {
        const int ny = y1 - y0 + 1, nrows = ny * (z1 - z0 + 1);
        for (int t = tid; t < total; t += NW * 64) {
            int a = 0, b = nrows;                      // the row r with row_off[r] <= t < row_off[r + 1]
            while (b - a > 1) {
                const int mid = (a + b) >> 1;
                if (T.row_off[mid] <= t) a = mid; else b = mid;
            }
            const int j = T.row_b[a] + (t - T.row_off[a]);
            float4 sp = g.sorted_pts[j];
            if (TL::PACKED) sp.w = __int_as_float(g.order[j]);
            else T.ord[t] = g.order[j];
            T.pts[t] = sp;
        }
    }
    __syncthreads();
    KNN_CLK(2);
    // faces of the staging cube (none where it reaches the cloud's bounds: nothing lies beyond), pulled in by the rounding margin of
    // the cell index
    const float mgn = 1e-3f * cellw;
    const float fx0 = x0 > 0 ? sg.minx + (float)x0 * cellw + mgn : -INFINITY, fx1 = x1 < sg.nx - 1 ? sg.minx + (float)(x1 + 1) * cellw - mgn : INFINITY;
    const float fy0 = y0 > 0 ? sg.miny + (float)y0 * cellw + mgn : -INFINITY, fy1 = y1 < sg.ny - 1 ? sg.miny + (float)(y1 + 1) * cellw - mgn : INFINITY;
    const float fz0 = z0 > 0 ? sg.minz + (float)z0 * cellw + mgn : -INFINITY, fz1 = z1 < sg.nz - 1 ? sg.minz + (float)(z1 + 1) * cellw - mgn : INFINITY;
    WaveLds* L = &wl[wave];
    typename Factory::Pending* P = &pend[wave];
    if (lane == 0) P->n = 0;
    wave_lds_sync();
    // original-index range of the tile's segment (points are sorted by (segment, cell): a segment's sorted positions are its indices)
    const int key_base = g.cell_start[sg.cell_base];
    const TileAcc tacc{T.pts, TL::PACKED ? nullptr : T.ord, key_base, g.cell_start[sg.cell_base + sg.nx * sg.ny * sg.nz] - key_base};
    // threshold-bin guess carried from query to query of this wave.  To start (a tile holds ~9 queries, so the four waves' first
    // queries are 4 of 9): a pilot -- the whole workgroup histograms the staged candidates around the tile's middle query (five steps
    // of 256 threads) and the bin that holds its max_nn-th neighbour, + the margin, seeds every wave.  A guess that is too small or
    // too large only costs that query the full second pass.
    int gbin = -1;
    float gthr = -1.0f;                            // round 3: the guess as a squared distance (tile_select_guess)
    if (staged && nq > 4) {
        int* ph = wl[0].hist;                          // idle until the first query
        __shared__ int pilot_bin;
        for (int t = tid; t < KNN_BINS; t += NW * 64) ph[t] = 0;
        __syncthreads();
        int pr = 0;
        const int pk = nq >> 1;
        while (pk >= T.q_off[pr + 1]) ++pr;
        const float4 pq = g.sorted_pts[T.q_b[pr] + (pk - T.q_off[pr])];
        const float bscale = (float)KNN_BINS / r2;
        for (int t = tid; t < total; t += NW * 64) {
            const float4 p = T.pts[t];
            const float d2 = dist2f(pq.x, pq.y, pq.z, p.x, p.y, p.z);
            if (d2 < r2) atomicAdd(&ph[min((int)(d2 * bscale), KNN_BINS - 1)], 1);
        }
        __syncthreads();
        if (wave == 0) {
            int hb4[KNN_BINS / 64], sum = 0;
#pragma unroll
            for (int u = 0; u < KNN_BINS / 64; ++u) { hb4[u] = ph[lane * (KNN_BINS / 64) + u]; sum += hb4[u]; }
            int incl = wave_incl_scan_i(sum);
            const unsigned long long m = __ballot(incl >= max_nn);
            if (lane == 0) pilot_bin = -1;
            if (m != 0ull && lane == __ffsll((long long)m) - 1) {
                int run = incl - sum, bb = lane * (KNN_BINS / 64);
#pragma unroll
                for (int u = 0; u < KNN_BINS / 64; ++u) {
                    if (run + hb4[u] >= max_nn) { bb = lane * (KNN_BINS / 64) + u; break; }
                    run += hb4[u];
                }
                pilot_bin = bb;
            }
        }
        __syncthreads();
        const int pb = pilot_bin;
        if (pb >= 0) {
            gbin = min(KNN_BINS - 1, pb + (max_nn * 4 <= KNN_CAPB ? pb : (pb >> KNN_GUESS_SHIFT)) + 2);
            gthr = fminf(r2, (float)(gbin + 1) / bscale);
        }
        __syncthreads();                               // wl[0].hist is wave 0's again
    }
    const bool use_guess = need_pop.guess != 0;
    KNN_CLK(3);
#ifdef KNN_LAB_CLK
    if (tid == 0) { atomicAdd(&knn_lab_clk[6], 1ull); atomicAdd(&knn_lab_clk[7], (unsigned long long)nq); }
#endif
    int run_r = 0;
    const int sny = y1 - y0 + 1;
    // A wave's first query is its own number; after that it takes the next one nobody has taken (queries differ in cost -- list or
    // two-pass selection, candidates in reach -- and a tile ends with its slowest wave: taking them in turn left the others idle)
    auto next_query = [&]() {
        int v = 0;
        if (lane == 0) v = atomicAdd(&T.next_q, 1);
        return __builtin_amdgcn_readfirstlane(v);
    };
    for (int qk = wave; qk < nq; qk = next_query()) {
        while (qk >= T.q_off[run_r + 1]) ++run_r;
        const int jq = T.q_b[run_r] + (qk - T.q_off[run_r]);
        // a query is a point of the tile, and the tile lies inside its staged cube: the point and its original index come from LDS (the two
        // dependent global loads per query were ~15 % of a tile's time with two waves per SIMD to hide them)
        int qi;
        float4 q;
        if (staged) {
            const int sr = (cz0 + run_r / qny - z0) * sny + (cy0 + run_r % qny - y0);
            const int ts_ = T.row_off[sr] + (jq - T.row_b[sr]);
            qi = T.ord_of(ts_);
            q = T.pts[ts_];
        } else {
            qi = g.order[jq];
            q = g.sorted_pts[jq];
        }
        if (qi < q_lo || qi >= q_hi) continue;
        bool done = false;
        if (staged) {
            float cover = fminf(fminf(q.x - fx0, fx1 - q.x), fminf(fminf(q.y - fy0, fy1 - q.y), fminf(q.z - fz0, fz1 - q.z)));
            if (cover < 0.f) cover = 0.f;
            const float cover2 = cover >= radius ? INFINITY : cover * cover;
            auto cons = fac.template make<TileAcc>(qi, q, L, tacc, P);
            int fast = -1;
            if (use_guess && gthr > 0.0f) fast = tile_select_guess(T, total, q, cover2, r2, max_nn, L, cons, gthr);
            if (fast < 0) {
                done = tile_select(T, total, q, cover2, r2, max_nn, L, cons, gbin);
                if (done && gbin >= 0) gthr = fminf(r2, (float)(gbin + 1) * r2 / (float)KNN_BINS);
            } else done = fast == 1;
        }
        // not provable from the staged cube (sparse spot, LDS budget, boundary-bin overflow): the query joins the list of the
        // per-query grid walk that runs after this kernel (ibl_knn_list_kernel)
        if (!done && lane == 0) fb_list[atomicAdd(fb_count, 1)] = jq;
    }
    KNN_CLK(4);
    fac.flush_block(pend, tacc);            // the queries still parked (normals)
    KNN_CLK(5);
}

// tiles: one workgroup each.  NW waves per workgroup; PACK: original indices in the staged points' w (see TileLds).  A factory states
// the one tile its consumer is searched on as TILE_TS (edge in cells), TILE_CAP (staged candidates), TILE_PACK and TILE_OCC (workgroups
// per CU of the launch bound); launch_knn instantiates that kernel and no other.
template <int TS, int CAP, class Factory, int NW = 4, bool PACK = false, int OCC = 1>
__global__ __launch_bounds__(NW * 64, OCC) void ibl_knn_tile_kernel(BatchGrid g, float radius, float r2, int max_nn, NeedPop need_pop, Factory fac,
                                                              int q_lo, int q_hi, int* __restrict__ fb_list, int* __restrict__ fb_count) {
    __shared__ TileLds<CAP, PACK> T;
    __shared__ WaveLds wl[NW];
    __shared__ typename Factory::Pending pend[NW];
    tile_knn_block<TS, NW>(g, radius, r2, max_nn, need_pop, fb_list, fb_count, fac, q_lo, q_hi, T, wl, pend);
}

// the queries the tile kernel could not answer from its staged cubes: one wavefront each, walking the grid (sorted positions in list)
template <class Factory>
__global__ __launch_bounds__(256) void ibl_knn_list_kernel(BatchGrid g, const int* __restrict__ seg_off, float radius, float r2, int max_nn,
                                                           Factory fac, const int* __restrict__ list, const int* __restrict__ count, int* status) {
    __shared__ WaveLds lds[4];
    const int n = *count;
    for (int e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        const int jq = list[e];
        const int qi = g.order[jq];
        const float4 q = g.sorted_pts[jq];
        const int s = seg_of(seg_off, g.n_seg, qi);
        auto cons = fac.template make<GlobalAcc>(qi, q, &lds[threadIdx.x >> 6], GlobalAcc{g.sorted_pts, g.order});
        hybrid_select(g, g.seg[s], q, qi, radius, r2, max_nn, &lds[threadIdx.x >> 6], cons, status);
    }
}

// ------------------------------------------------------------------------------------------------
// host: one search = the tile kernel + the grid walk of the queries it could not answer (used by the launchers of the including .hip)
// ------------------------------------------------------------------------------------------------
static NeedPop need_pop_table(const RegDiag& diag, int max_nn, int ts) {
    NeedPop np;
    np.v[0] = 0.f;
    for (int rho = 1; rho < 8; ++rho)
        np.v[rho] = (float)(diag.knn_safety * max_nn * (ts + 2.0 * rho) * (ts + 2.0 * rho) / (3.14159265358979 * rho * rho));
    np.rho_start = diag.knn_rho;
    np.guess = diag.knn_noguess ? 0 : 1;          // diagnostics: the tests compare both selections bit for bit
    return np;
}

template <class Factory>
static int launch_knn(ibl_reg_ctx* ctx, const BatchGrid& g, const int* seg_off, int n, int q0, int q1, double radius, int max_nn, const Factory& fac,
                      int* status, hipStream_t s) {
    if (q1 <= q0) return IBL_OK;
    const float r = (float)radius, r2 = (float)(radius * radius);
    // No kernel walks a grid without tiles (the per-query kernel that stood here could not be launched): every caller builds its grid with
    // ibl_build_tile_grid, which gives each segment, empty ones included, at least one tile (nx, ny, nz >= 1), and q1 > q0 means the
    // batch has a point, hence a segment, hence n_tiles >= 1.  The edge is the factory's at every call site (KNN_TILE_*, reg_common.h).
    if (!g.tile_base || g.n_tiles <= 0) return ibl_set_error(IBL_ERR_INTERNAL, "k-NN search needs a tile grid (ibl_build_tile_grid): this grid has no tiles");
    if (g.ts != Factory::TILE_TS) return ibl_set_error(IBL_ERR_INTERNAL, "k-NN tiles of %d^3 cells are not built", g.ts);
    ArenaMark m(ctx);                    // (released on return: later allocations are used by later kernels of the same stream)
    int *fb_list, *fb_count;
    IBL_ARENA(fb_list, int, (int64_t)n + 64);
    IBL_ARENA(fb_count, int, 64);
    IBL_HIP_CHECK(hipMemsetAsync(fb_count, 0, sizeof(int), s));
    const NeedPop np = need_pop_table(ctx->diag, max_nn, g.ts);
    // LDS budget of the staged cube.  The kernel is bound by its resident workgroups: with its LDS padded so that only ONE workgroup fits a
    // CU it ran the 100-neighbour search in 10.6 ms against 5.4 ms with two.  Round 3, final form for the consumers that read geometry only
    // (TILE_PACK): a PACKED tile (the original index rides in the staged point's w: 16 instead of 20 B per candidate) of 1 600 candidates +
    // the four waves' scratch = 53.5 KB and a 168-register launch bound -> THREE four-wave workgroups per CU: feature call 8.49 -> 7.0 ms
    // although 0.4 % (not 0.1 %) of the queries now overflow a cube and join the grid walk.  (Six waves per workgroup on a 2 528-candidate
    // packed tile -- also twelve waves per CU -- was slower, 7.13 vs 5.27 ms for the search: the per-tile set-up and barriers are then
    // shared by fewer queries per wave; two eight-wave workgroups per CU, sixteen waves, brought nothing: 6.39 against 6.41 ms,
    // DESIGN.md.)  The colour-gradient search reads the staged intensity and keeps the 20-byte tile (1 024 candidates, three workgroups
    // per CU as well).
    hipLaunchKernelGGL((ibl_knn_tile_kernel<Factory::TILE_TS, Factory::TILE_CAP, Factory, 4, Factory::TILE_PACK, Factory::TILE_OCC>), dim3(g.n_tiles), dim3(256), 0,
                       s, g, r, r2, max_nn, np, fac, q0, q1, fb_list, fb_count);
    IBL_LAUNCH_CHECK();
#ifdef KNN_LAB_CLK
    { unsigned long long h[16]; (void)hipStreamSynchronize(s); (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(knn_lab_clk), sizeof(h));
      const double nt = (double)std::max<unsigned long long>(h[6], 1);
      fprintf(stderr, "[knn-clk] k=%d ts=%d tiles with queries %llu (%.1f queries each): clocks (100 MHz ticks) per tile: query rows %.0f, rho loop %.0f, staging %.0f, "
              "pilot %.0f, queries(wave 0) %.0f, flush %.0f\n", max_nn, g.ts, h[6], (double)h[7] / nt, h[0] / nt, h[1] / nt, h[2] / nt, h[3] / nt, h[4] / nt, h[5] / nt);
      const double nq0 = (double)h[7] / 4.0;         // queries of wave 0
      fprintf(stderr, "[knn-clk]   per query of wave 0: pass 1 %.0f, threshold %.0f, pass 2 %.0f, boundary rank %.0f, consumer finish %.0f\n", h[8] / nq0, h[9] / nq0,
              h[10] / nq0, h[11] / nq0, h[12] / nq0);
      fprintf(stderr, "[knn-clk]   consumer finish: index sort %.0f, list write %.0f, inner selection %.0f\n", h[13] / nq0, h[14] / nq0, h[15] / nq0);
      unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(knn_lab_clk), z, sizeof(z)); }
#endif
#ifdef KNN_LAB_STATS
    { int h[8]; (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(knn_lab_stats), sizeof(h)); fprintf(stderr, "[knn-lab] k=%d queries %d from_list %d select_all %d guess_low %d overflow %d\n", max_nn, h[0], h[1], h[2], h[3], h[4]); int z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(knn_lab_stats), z, sizeof(z)); }
#endif
    const int blocks = std::max(1, std::min(2048, (q1 - q0 + 3) / 4));
    hipLaunchKernelGGL((ibl_knn_list_kernel<Factory>), dim3(blocks), dim3(256), 0, s, g, seg_off, r, r2, max_nn, fac, fb_list, fb_count, status);
    if (ctx->diag.knn_debug) {                      // diagnostics: how many queries the staged cubes could not answer
        int h = 0;
        (void)hipMemcpyAsync(&h, fb_count, sizeof(int), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        fprintf(stderr, "[knn] r=%.3f k=%d ts=%d tiles=%d queries=%d fallback=%d (%.1f %%)\n", radius, max_nn, g.ts, g.n_tiles, q1 - q0, h, 100.0 * h / (q1 - q0));
    }
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}
