// reg_normals.hip -- normals of every point of a batch from its <= max_nn nearest neighbours within a radius (Open3D estimate_normals with
// KDTreeSearchParamHybrid, utils/fpfh_register.py:90-97): the consumer of the neighbour selection (knn_select.h) that parks each query's
// sorted neighbour list and solves the normals in batches (knn_normal.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "reg_common.h"
#include "knn_select.h"
#include "knn_normal.h"

template <class Acc>
struct NormalConsumer {
    static constexpr bool WANTS_INNER = false;
    float4* normals;
    Acc acc;
    WaveLds* L;
    NormalPending* P;        // null: solve at once (the list kernel, whose handles are 32-bit)
    int qi;
    int ncount;
    __device__ void begin(int) { ncount = 0; }
    __device__ void accept(bool sel, int j, const float4&, float) {
        const int lane = threadIdx.x & 63;
        const unsigned long long m = __ballot(sel);
        if (sel) L->sel_j[ncount + __popcll(m & ((1ull << lane) - 1ull))] = j;
        ncount += __popcll(m);
    }
    __device__ void finish(int k) {
        const int lane = threadIdx.x & 63;
        sort_selected_by_index<false>(L, acc, k);
        if (P != nullptr && k <= NP_MAXK) {
            const int slot = P->n;
            if (lane < k) P->h[slot][lane] = (unsigned short)L->b_j[lane];
            if (lane == 0) { P->qi[slot] = qi; P->k[slot] = k; P->n = slot + 1; }
            if (slot + 1 == NP_SLOTS) normal_flush(P, acc, normals);
            else wave_lds_sync();
        } else if (lane == 0) {
            normal_solve(acc, L->b_j, k, qi, normals);
        }
    }
};

struct NormalFactory {
    // its tile: 4^3 cells, 1 024 candidates with their index array (its pending normals are solved by a 4-wave block flush)
    static constexpr int TILE_TS = KNN_TILE_NORMAL, TILE_CAP = 1024, TILE_OCC = 1;
    static constexpr bool TILE_PACK = false;
    typedef NormalPending Pending;
    float4* normals;
    template <class Acc> __device__ NormalConsumer<Acc> make(int qi, const float4&, WaveLds* L, const Acc& acc, Pending* P = nullptr) const {
        NormalConsumer<Acc> c;
        c.normals = normals; c.acc = acc; c.L = L; c.P = P; c.qi = qi; c.ncount = 0;
        return c;
    }
    template <class Acc> __device__ void flush(Pending* P, const Acc& acc) const { normal_flush(P, acc, normals); }
    template <class Acc> __device__ void flush_block(Pending* pend, const Acc& acc) const { normal_flush_block(pend, acc, normals); }
};

int ibl_launch_normals(ibl_reg_ctx* ctx, const BatchGrid& g, const float4* pts, const int* seg_off, int n, double radius, int max_nn, float4* normals,
                       int* status, hipStream_t s) {
    if (n <= 0) return IBL_OK;
    if (max_nn > 256) return ibl_set_error(IBL_ERR_UNSUPPORTED, "normals: max_nn %d > 256", max_nn);
    void* tok;
    ibl_prof_begin(IBL_PROF_NORMALS, 24.0 * (double)n, s, &tok);
    const int st = launch_knn(ctx, g, seg_off, n, 0, n, radius, max_nn, NormalFactory{normals}, status, s);
    ibl_prof_end(tok, s);
    return st;
}
