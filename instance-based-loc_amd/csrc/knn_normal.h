// knn_normal.h -- a normal from its neighbours: the nine moment sums in ascending original index, the covariance, and the eigenvector of
// its smallest eigenvalue; the parked ("pending") neighbour lists that let a wave solve one normal per lane.  Shared by the stand-alone
// normals search (reg_normals.hip) and by ibl_normals_from_mask_kernel of the fused normals + FPFH path (reg_fpfh.hip): the same
// arithmetic in the same order, so a point's normal does not depend on which kernel found its neighbours.
#pragma once
#include "knn_select.h"

// ------------------------------------------------------------------------------------------------
// robust symmetric 3x3 eigen solver (Open3D FastEigen3x3 / Eberly): smallest-eigenvalue eigenvector
// ------------------------------------------------------------------------------------------------
__device__ inline void eigenvector0_d(const double* A, double ev, double* out) {
    double r0[3] = {A[0] - ev, A[1], A[2]}, r1[3] = {A[1], A[3] - ev, A[4]}, r2[3] = {A[2], A[4], A[5] - ev};
    double c01[3], c02[3], c12[3];
    cross3d(r0, r1, c01); cross3d(r0, r2, c02); cross3d(r1, r2, c12);
    const double d0 = dot3d(c01, c01), d1 = dot3d(c02, c02), d2 = dot3d(c12, c12);
    double dmax = d0; int imax = 0;
    if (d1 > dmax) { dmax = d1; imax = 1; }
    if (d2 > dmax) { imax = 2; }
    const double* c = imax == 0 ? c01 : (imax == 1 ? c02 : c12);
    const double d = imax == 0 ? d0 : (imax == 1 ? d1 : d2);
    const double s = sqrt(d);
    out[0] = c[0] / s; out[1] = c[1] / s; out[2] = c[2] / s;
}

__device__ inline void eigenvector1_d(const double* A, const double* e0, double ev1, double* out) {
    double U[3], V[3];
    if (fabs(e0[0]) > fabs(e0[1])) {
        const double inv = 1.0 / sqrt(e0[0] * e0[0] + e0[2] * e0[2]);
        U[0] = -e0[2] * inv; U[1] = 0; U[2] = e0[0] * inv;
    } else {
        const double inv = 1.0 / sqrt(e0[1] * e0[1] + e0[2] * e0[2]);
        U[0] = 0; U[1] = e0[2] * inv; U[2] = -e0[1] * inv;
    }
    cross3d(e0, U, V);
    double AU[3] = {A[0] * U[0] + A[1] * U[1] + A[2] * U[2], A[1] * U[0] + A[3] * U[1] + A[4] * U[2],
                    A[2] * U[0] + A[4] * U[1] + A[5] * U[2]};
    double AV[3] = {A[0] * V[0] + A[1] * V[1] + A[2] * V[2], A[1] * V[0] + A[3] * V[1] + A[4] * V[2],
                    A[2] * V[0] + A[4] * V[1] + A[5] * V[2]};
    double m00 = dot3d(U, AU) - ev1, m01 = dot3d(U, AV), m11 = dot3d(V, AV) - ev1;
    const double a00 = fabs(m00), a01 = fabs(m01), a11 = fabs(m11);
    if (a00 >= a11) {
        const double mx = a00 > a01 ? a00 : a01;
        if (mx > 0) {
            if (a00 >= a01) { m01 /= m00; m00 = 1 / sqrt(1 + m01 * m01); m01 *= m00; }
            else { m00 /= m01; m01 = 1 / sqrt(1 + m00 * m00); m00 *= m01; }
            for (int i = 0; i < 3; ++i) out[i] = m01 * U[i] - m00 * V[i];
        } else { out[0] = U[0]; out[1] = U[1]; out[2] = U[2]; }
    } else {
        const double mx = a11 > a01 ? a11 : a01;
        if (mx > 0) {
            if (a11 >= a01) { m01 /= m11; m11 = 1 / sqrt(1 + m01 * m01); m01 *= m11; }
            else { m11 /= m01; m01 = 1 / sqrt(1 + m11 * m11); m11 *= m01; }
            for (int i = 0; i < 3; ++i) out[i] = m11 * U[i] - m01 * V[i];
        } else { out[0] = U[0]; out[1] = U[1]; out[2] = U[2]; }
    }
}

__device__ inline void fast_eigen_normal_d(const double* cov, double* n) {
    double mc = cov[0];
    for (int i = 1; i < 6; ++i) if (cov[i] > mc) mc = cov[i];
    if (mc == 0) { n[0] = n[1] = n[2] = 0; return; }
    double A[6];
    for (int i = 0; i < 6; ++i) A[i] = cov[i] / mc;
    const double norm = A[1] * A[1] + A[2] * A[2] + A[4] * A[4];
    if (norm > 0) {
        const double q = (A[0] + A[3] + A[5]) / 3;
        const double b00 = A[0] - q, b11 = A[3] - q, b22 = A[5] - q;
        const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * 2) / 6);
        const double c00 = b11 * b22 - A[4] * A[4];
        const double c01 = A[1] * b22 - A[4] * A[2];
        const double c02 = A[1] * A[4] - b11 * A[2];
        const double det = (b00 * c00 - A[1] * c01 + A[2] * c02) / (p * p * p);
        double half_det = det * 0.5;
        if (half_det < -1.0) half_det = -1.0;
        if (half_det > 1.0) half_det = 1.0;
        const double angle = acos(half_det) / 3.0;
        const double two_thirds_pi = 2.09439510239319549;
        const double beta2 = cos(angle) * 2;
        const double beta0 = cos(angle + two_thirds_pi) * 2;
        const double beta1 = -(beta0 + beta2);
        const double e0 = q + p * beta0, e1 = q + p * beta1, e2 = q + p * beta2;
        double v0[3], v1[3], v2[3];
        if (half_det >= 0) {
            eigenvector0_d(A, e2, v2);
            if (e2 < e0 && e2 < e1) { n[0] = v2[0]; n[1] = v2[1]; n[2] = v2[2]; return; }
            eigenvector1_d(A, v2, e1, v1);
            if (e1 < e0 && e1 < e2) { n[0] = v1[0]; n[1] = v1[1]; n[2] = v1[2]; return; }
            cross3d(v1, v2, v0);
            n[0] = v0[0]; n[1] = v0[1]; n[2] = v0[2];
        } else {
            eigenvector0_d(A, e0, v0);
            if (e0 < e1 && e0 < e2) { n[0] = v0[0]; n[1] = v0[1]; n[2] = v0[2]; return; }
            eigenvector1_d(A, v0, e1, v1);
            if (e1 < e0 && e1 < e2) { n[0] = v1[0]; n[1] = v1[1]; n[2] = v1[2]; return; }
            cross3d(v0, v1, v2);
            n[0] = v2[0]; n[1] = v2[1]; n[2] = v2[2];
        }
    } else {
        if (cov[0] < cov[3] && cov[0] < cov[5]) { n[0] = 1; n[1] = 0; n[2] = 0; }
        else if (cov[3] < cov[0] && cov[3] < cov[5]) { n[0] = 0; n[1] = 1; n[2] = 0; }
        else { n[0] = 0; n[1] = 0; n[2] = 1; }
    }
}

// Normals are solved in batches: a wave parks the sorted neighbour list of each query (<= NP_MAXK handles) in NormalPending and, once
// NP_SLOTS queries are parked (or its tile is finished), every lane takes one query: covariance sums in ascending original index, then
// the 3x3 eigen solve (~500 fp64 instructions that used to run on lane 0 alone, once per query, plus nine 64-lane fp64 reductions).
// The sums run in the same order on every path (tile kernel, list kernel, ibl_normals_from_mask_kernel), so a point's normal does not
// depend on which one served it.
#define NP_SLOTS 16
#define NP_MAXK 32
template <int SLOTS_>
struct NormalPendingT {
    static constexpr int SLOTS = SLOTS_;
    unsigned short h[SLOTS_][NP_MAXK];
    int qi[SLOTS_];
    int k[SLOTS_];
    int n;
};
typedef NormalPendingT<NP_SLOTS> NormalPending;

// the nine moment sums of a normal's neighbours (ascending original index) -> covariance -> smallest eigenvector
__device__ __forceinline__ void normal_from_moments(double* c, int k, int qi, float4* __restrict__ normals);

template <class Acc, class H>
__device__ __forceinline__ void normal_solve(const Acc& acc, const H* __restrict__ hnd, int k, int qi, float4* __restrict__ normals) {
    double c[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) c[t] = 0.0;
    for (int t = 0; t < k; ++t) {
        const float4 p = acc.pt((int)hnd[t]);
        const double x = p.x, y = p.y, z = p.z;
        c[0] += x; c[1] += y; c[2] += z;
        c[3] += x * x; c[4] += x * y; c[5] += x * z; c[6] += y * y; c[7] += y * z; c[8] += z * z;
    }
    normal_from_moments(c, k, qi, normals);
}

__device__ __forceinline__ void normal_from_moments(double* c, int k, int qi, float4* __restrict__ normals) {
    double n[3];
    if (k >= 3) {
#pragma unroll
        for (int t = 0; t < 9; ++t) c[t] /= (double)k;
        double cov[6] = {c[3] - c[0] * c[0], c[4] - c[0] * c[1], c[5] - c[0] * c[2],
                         c[6] - c[1] * c[1], c[7] - c[1] * c[2], c[8] - c[2] * c[2]};
        fast_eigen_normal_d(cov, n);
    } else {
        double cov[6] = {1, 0, 0, 1, 0, 1};
        fast_eigen_normal_d(cov, n);
    }
    if (sqrt(dot3d(n, n)) == 0.0) { n[0] = 0; n[1] = 0; n[2] = 1; }
    normals[qi] = make_float4((float)n[0], (float)n[1], (float)n[2], 0.0f);
}

template <class Acc, class PT>
__device__ __forceinline__ void normal_flush(PT* P, const Acc& acc, float4* __restrict__ normals) {
    const int lane = threadIdx.x & 63;
    wave_lds_sync();
    const int n = P->n;
    if (lane < n) normal_solve(acc, P->h[lane], P->k[lane], P->qi[lane], normals);
    wave_lds_sync();
    if (lane == 0) P->n = 0;
    wave_lds_sync();
}

// End of a tile: the queries still parked by the four waves (two or three each -- a tile holds ~10 queries) are solved together by
// wave 0, one per lane, instead of once per wave with two or three lanes active.
template <class Acc, class PT>
__device__ __forceinline__ void normal_flush_block(PT* pend, const Acc& acc, float4* __restrict__ normals) {
    __syncthreads();
    if ((threadIdx.x >> 6) == 0) {
        const int lane = threadIdx.x & 63;
        const int n0 = pend[0].n, n1 = pend[1].n, n2 = pend[2].n, n3 = pend[3].n;
        if (lane < n0 + n1 + n2 + n3) {
            const int w = lane < n0 ? 0 : (lane < n0 + n1 ? 1 : (lane < n0 + n1 + n2 ? 2 : 3));
            const int sl = lane - (w > 0 ? n0 : 0) - (w > 1 ? n1 : 0) - (w > 2 ? n2 : 0);
            normal_solve(acc, pend[w].h[sl], pend[w].k[sl], pend[w].qi[sl], normals);
        }
    }
}
