// reg_colorgrad.hip -- colour (intensity) gradient of every point in its tangent plane from its <= max_nn nearest neighbours within a
// radius (Open3D InitializePointCloudForColoredICP, registration_colored_icp :132-135): a consumer of the neighbour selection
// (knn_select.h) that reads the staged intensity, so its tiles are not packed.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "reg_common.h"
#include "knn_select.h"

// Symmetric 3x3 solve, LDL^T with diagonal pivoting (Open3D solves the gradient system with Eigen's ldlt()): at each step the largest
// remaining diagonal entry is moved to the front by a symmetric exchange, then eliminated.  x stays zero when a pivot is zero or not
// finite (a singular system: coincident or collinear neighbours).  Cramer's rule, which stood here, lost up to 7e-4 of max|g| to
// cancelling cofactors on dense, small neighbourhoods.  Scalars only (no indexed arrays: nothing goes to scratch); the same statements
// as solve3_sym of oracle/oracle_reg.c.
__device__ __forceinline__ void swap_d(double& u, double& v) { const double t = u; u = v; v = t; }
__device__ inline bool solve3_sym(const double M[3][3], const double B[3], double x[3]) {
    double a00 = M[0][0], a01 = M[0][1], a02 = M[0][2], a11 = M[1][1], a12 = M[1][2], a22 = M[2][2];
    double b0 = B[0], b1 = B[1], b2 = B[2];
    x[0] = x[1] = x[2] = 0.0;
    int first = 0;                                   // the index exchanged with 0
    if (fabs(a11) > fabs(a00) && fabs(a11) >= fabs(a22)) first = 1;
    else if (fabs(a22) > fabs(a00)) first = 2;
    if (first == 1) { swap_d(a00, a11); swap_d(a02, a12); swap_d(b0, b1); }
    if (first == 2) { swap_d(a00, a22); swap_d(a01, a12); swap_d(b0, b2); }
    if (a00 == 0.0 || !isfinite(a00)) return false;
    const double l1 = a01 / a00, l2 = a02 / a00;
    a11 -= l1 * a01; a12 -= l1 * a02; a22 -= l2 * a02;
    b1 -= l1 * b0; b2 -= l2 * b0;
    const bool second = fabs(a22) > fabs(a11);      // 1 and 2 exchanged
    if (second) { swap_d(a11, a22); swap_d(a01, a02); swap_d(b1, b2); }
    if (a11 == 0.0 || !isfinite(a11)) return false;
    const double l = a12 / a11;
    a22 -= l * a12;
    b2 -= l * b1;
    if (a22 == 0.0 || !isfinite(a22)) return false;
    double x2 = b2 / a22;
    double x1 = (b1 - a12 * x2) / a11;
    double x0 = (b0 - a01 * x1 - a02 * x2) / a00;
    if (second) swap_d(x1, x2);
    if (first == 1) swap_d(x0, x1);
    if (first == 2) swap_d(x0, x2);
    x[0] = x0; x[1] = x1; x[2] = x2;
    return true;
}

template <class Acc>
struct GradConsumer {
    static constexpr bool WANTS_INNER = false;
    const float4* normals;
    Acc acc;
    float4* grad;
    int qi;
    float4 q, qn;
    WaveLds* L;
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
        double a[9];             // AtA (6 unique: 00 01 02 11 12 22) + Atb (3)
        for (int t = 0; t < 9; ++t) a[t] = 0.0;
        for (int t = lane; t < k; t += 64) {
            const int j = L->b_j[t];
            if (acc.ord(j) == qi) continue;
            const float4 p = acc.pt(j);
            const double vt[3] = {q.x, q.y, q.z}, nt[3] = {qn.x, qn.y, qn.z};
            const double dd[3] = {(double)p.x - vt[0], (double)p.y - vt[1], (double)p.z - vt[2]};
            const double pr = dot3d(dd, nt);
            const double r[3] = {(double)p.x - pr * nt[0] - vt[0], (double)p.y - pr * nt[1] - vt[1], (double)p.z - pr * nt[2] - vt[2]};
            const double b = (double)p.w - (double)q.w;
            a[0] += r[0] * r[0]; a[1] += r[0] * r[1]; a[2] += r[0] * r[2]; a[3] += r[1] * r[1]; a[4] += r[1] * r[2]; a[5] += r[2] * r[2];
            a[6] += r[0] * b; a[7] += r[1] * b; a[8] += r[2] * b;
        }
        for (int t = 0; t < 9; ++t) a[t] = wave_sum_d(a[t]);
        if (lane == 0) {
            double gx[3] = {0, 0, 0};
            if (k >= 4) {
                const double nt[3] = {qn.x, qn.y, qn.z};
                const double wgt = (double)(k - 1);
                double M[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] += wgt * nt[r] * wgt * nt[c];
                const double B[3] = {a[6], a[7], a[8]};
                solve3_sym(M, B, gx);
            }
            grad[qi] = make_float4((float)gx[0], (float)gx[1], (float)gx[2], 0.0f);
        }
    }
};

struct GradFactory {
    // its tile: 4^3 cells, 1 024 candidates with their index array (reads the staged intensity: no room for the index in w)
    static constexpr int TILE_TS = KNN_TILE_NORMAL, TILE_CAP = 1024, TILE_OCC = 1;
    static constexpr bool TILE_PACK = false;
    typedef NoPending Pending;
    const float4* normals; float4* grad;
    template <class Acc> __device__ void flush(Pending*, const Acc&) const {}
    template <class Acc> __device__ void flush_block(Pending*, const Acc&) const {}
    template <class Acc> __device__ GradConsumer<Acc> make(int qi, const float4& q, WaveLds* L, const Acc& acc, Pending* = nullptr) const {
        GradConsumer<Acc> c;
        c.normals = normals; c.acc = acc; c.grad = grad; c.qi = qi; c.q = q; c.qn = normals[qi]; c.L = L; c.ncount = 0;
        return c;
    }
};

int ibl_launch_color_grad(ibl_reg_ctx* ctx, const BatchGrid& g, const float4* pts, const float4* normals, const int* seg_off, int q0, int q1, double radius,
                          int max_nn, float4* grad, int* status, hipStream_t s) {
    if (q1 <= q0) return IBL_OK;
    if (max_nn > 256) return ibl_set_error(IBL_ERR_UNSUPPORTED, "colour gradient: max_nn %d > 256", max_nn);
    return launch_knn(ctx, g, seg_off, q1, q0, q1, radius, max_nn, GradFactory{normals, grad}, status, s);
}
