// obb_iou.hip -- the distance matrix of ObjectMemory._recluster_IoU (object_memory.py:710-747) on the device: D[i][j] = 1 - IoU of
// the oriented boxes of objects i and j, the matrix the host loop builds pair by pair with calculate_obj_aligned_3d_IoU
// (utils/IoU_ops.py) and hands to scikit-learn.  The boxes (Qhull hull + PCA frame) are computed on the host, one per object; this
// file does the N^2 / 2 box-box intersections.
//
// One workgroup per 64 x 64 tile of the upper triangle, its two sets of boxes staged in LDS:
//   phase 1  one thread per pair: separating-axis test on the 15 axes (3 + 3 face normals, 9 edge cross products), fp64.  A separated
//            or merely touching pair has IoU exactly 0 (distance exactly 1.0, the value the host produces); most pairs end here
//   phase 2  the survivors, listed in LDS, get their exact intersection volume: V = 1/3 sum_k h_k area_k over the 12 face planes,
//            face k of one box clipped by the other box's 6 planes (Sutherland-Hodgman in the face's 2-D coordinates), h_k the signed
//            distance of plane k from the centre of box A.  A plane of B that coincides with a plane of A with the same outward normal
//            is counted once, as A's face
//   out      the tile goes to D row by row and, off the diagonal, transposed, both through LDS so that every store is coalesced.
// Every element is written by exactly one thread and nothing is accumulated in floating point across threads: the output is
// deterministic.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ibloc.h"
#include "reg_common.h"

namespace {

constexpr int TILE = 64;
constexpr int THREADS = 256;
constexpr int BOX = 15;              // centre (3), R row-major (9, columns = box axes), half extents (3)
constexpr int MAXV = 12;             // a rectangle clipped by 6 half-planes has at most 10 vertices; 2 slots of headroom for rounding
constexpr double TOUCH_REL = 1e-12;  // an overlap no deeper than this fraction of the projected sizes ...
constexpr double TOUCH_ABS = 2e-12;  // ... or than this (the host calls an intersection empty when its inscribed ball has r <= 1e-12)
constexpr double CROSS_MIN2 = 1e-6;  // squared length below which an edge cross product is too ill-conditioned to test (phase 2 decides)
constexpr double COPLANAR = 1e-12;   // normals within this (per component), offsets within this relative to the box sizes

struct Box {
    double c[3], R[3][3], h[3];
};

__device__ __forceinline__ void load_box(const double (*s)[TILE], int k, Box& b) {
    for (int a = 0; a < 3; ++a) b.c[a] = s[a][k];
    for (int r = 0; r < 3; ++r)
        for (int a = 0; a < 3; ++a) b.R[r][a] = s[3 + 3 * r + a][k];
    for (int a = 0; a < 3; ++a) b.h[a] = s[12 + a][k];
}

// relative frame of a pair: C[i][j] = a_i . b_j, T = cB - cA, TA = R_A^T T, TB = R_B^T T
struct Frame {
    double C[3][3], TA[3], TB[3];
};

__host__ __device__ __forceinline__ void make_frame(const Box& A, const Box& B, Frame& f) {
    const double T[3] = {B.c[0] - A.c[0], B.c[1] - A.c[1], B.c[2] - A.c[2]};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) f.C[i][j] = A.R[0][i] * B.R[0][j] + A.R[1][i] * B.R[1][j] + A.R[2][i] * B.R[2][j];
        f.TA[i] = A.R[0][i] * T[0] + A.R[1][i] * T[1] + A.R[2][i] * T[2];
        f.TB[i] = B.R[0][i] * T[0] + B.R[1][i] * T[1] + B.R[2][i] * T[2];
    }
}

// projections of the two boxes on axis L are disjoint, or overlap by no more than the touching tolerance (|L| = len)
__host__ __device__ __forceinline__ bool apart(double d, double rA, double rB, double len) {
    const double r = rA + rB;
    return d - r >= -fmax(TOUCH_REL * r, TOUCH_ABS * len);
}

// separating-axis test: true when the boxes are disjoint or only touch (IoU exactly 0)
__host__ __device__ bool separated(const Box& A, const Box& B, const Frame& f) {
    double aC[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) aC[i][j] = fabs(f.C[i][j]);
    for (int i = 0; i < 3; ++i)
        if (apart(fabs(f.TA[i]), A.h[i], B.h[0] * aC[i][0] + B.h[1] * aC[i][1] + B.h[2] * aC[i][2], 1.0)) return true;
    for (int j = 0; j < 3; ++j)
        if (apart(fabs(f.TB[j]), A.h[0] * aC[0][j] + A.h[1] * aC[1][j] + A.h[2] * aC[2][j], B.h[j], 1.0)) return true;
    // L = a_i x b_j; in A's frame L = e_i x C[:, j], so a_i1 . L = -C[i2][j], a_i2 . L = C[i1][j], and b_j1 . L = +-C[i][j2] (B right-handed)
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            const double len2 = f.C[i1][j] * f.C[i1][j] + f.C[i2][j] * f.C[i2][j];
            if (len2 < CROSS_MIN2) continue;
            const double rA = A.h[i1] * aC[i2][j] + A.h[i2] * aC[i1][j];
            const double rB = B.h[j1] * aC[i][j2] + B.h[j2] * aC[i][j1];
            const double d = fabs(f.TA[i2] * f.C[i1][j] - f.TA[i1] * f.C[i2][j]);
            if (apart(d, rA, rB, sqrt(len2))) return true;
        }
    }
    return false;
}

// area of the rectangle [-hu, hu] x [-hv, hv] clipped by the half-planes la[m] s + lb[m] t + lc[m] <= 0 not flagged in `skip`
// (Sutherland-Hodgman; the polygon lives in private memory, indexed at run time)
__host__ __device__ double clipped_area(double hu, double hv, const double* la, const double* lb, const double* lc, unsigned skip) {
    double ps[2][MAXV], pt[2][MAXV];
    ps[0][0] = -hu; pt[0][0] = -hv;
    ps[0][1] = hu;  pt[0][1] = -hv;
    ps[0][2] = hu;  pt[0][2] = hv;
    ps[0][3] = -hu; pt[0][3] = hv;
    int n = 4, cur = 0;
    for (int m = 0; m < 6; ++m) {
        if ((skip >> m) & 1u) continue;
        const int nx = cur ^ 1;
        int k = 0;
        double sp = ps[cur][n - 1], tp = pt[cur][n - 1];
        double dp = la[m] * sp + lb[m] * tp + lc[m];
        for (int v = 0; v < n; ++v) {
            const double sq = ps[cur][v], tq = pt[cur][v];
            const double dq = la[m] * sq + lb[m] * tq + lc[m];
            if (((dp < 0.0 && dq > 0.0) || (dp > 0.0 && dq < 0.0)) && k < MAXV) {
                const double u = dp / (dp - dq);
                ps[nx][k] = sp + u * (sq - sp);
                pt[nx][k] = tp + u * (tq - tp);
                ++k;
            }
            if (dq <= 0.0 && k < MAXV) {
                ps[nx][k] = sq;
                pt[nx][k] = tq;
                ++k;
            }
            sp = sq; tp = tq; dp = dq;
        }
        n = k;
        cur = nx;
        if (n < 3) return 0.0;
    }
    double a = 0.0;
    for (int v = 0; v < n; ++v) {
        const int w = v + 1 == n ? 0 : v + 1;
        a += ps[cur][v] * pt[cur][w] - ps[cur][w] * pt[cur][v];
    }
    return 0.5 * a;
}

__host__ __device__ __forceinline__ bool same_plane(const Box& A, int a, double s, const Box& B, int j, double sg, double oA, double oB) {
    for (int r = 0; r < 3; ++r)
        if (fabs(s * A.R[r][a] - sg * B.R[r][j]) > COPLANAR) return false;
    return fabs(oA - oB) <= COPLANAR * (A.h[0] + A.h[1] + A.h[2] + B.h[0] + B.h[1] + B.h[2] + fabs(oA) + fabs(oB));
}

// exact volume of A n B (both boxes valid, the pair survived the separating-axis test)
__host__ __device__ double intersection_volume(const Box& A, const Box& B, const Frame& f) {
    // planes relative to A's centre: A (a, s): n = s a_a, offset hA_a; B (j, sg): n = sg b_j, offset sg TB_j + hB_j
    unsigned same[6] = {0, 0, 0, 0, 0, 0};      // same[A face] bit (B plane): coinciding planes with the same outward normal
    unsigned b_dup = 0;                          // B faces counted as A's
    for (int a = 0; a < 3; ++a)
        for (int sa = 0; sa < 2; ++sa)
            for (int j = 0; j < 3; ++j)
                for (int sb = 0; sb < 2; ++sb) {
                    const double s = sa ? -1.0 : 1.0, sg = sb ? -1.0 : 1.0;
                    if (same_plane(A, a, s, B, j, sg, A.h[a], sg * f.TB[j] + B.h[j])) {
                        same[2 * a + sa] |= 1u << (2 * j + sb);
                        b_dup |= 1u << (2 * j + sb);
                    }
                }
    double la[6], lb[6], lc[6];
    double vol = 0.0;
    // faces of A clipped by B's planes
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        for (int sa = 0; sa < 2; ++sa) {
            const double s = sa ? -1.0 : 1.0;
            for (int j = 0; j < 3; ++j)
                for (int sb = 0; sb < 2; ++sb) {
                    const double sg = sb ? -1.0 : 1.0;
                    la[2 * j + sb] = sg * f.C[b][j];
                    lb[2 * j + sb] = sg * f.C[c][j];
                    lc[2 * j + sb] = sg * (s * A.h[a] * f.C[a][j] - f.TB[j]) - B.h[j];
                }
            vol += A.h[a] * clipped_area(A.h[b], A.h[c], la, lb, lc, same[2 * a + sa]);
        }
    }
    // faces of B clipped by A's planes
    for (int j = 0; j < 3; ++j) {
        const int k = (j + 1) % 3, l = (j + 2) % 3;
        for (int sb = 0; sb < 2; ++sb) {
            if ((b_dup >> (2 * j + sb)) & 1u) continue;
            const double sg = sb ? -1.0 : 1.0;
            for (int i = 0; i < 3; ++i)
                for (int sa = 0; sa < 2; ++sa) {
                    const double s = sa ? -1.0 : 1.0;
                    la[2 * i + sa] = s * f.C[i][k];
                    lb[2 * i + sa] = s * f.C[i][l];
                    lc[2 * i + sa] = s * (f.TA[i] + sg * B.h[j] * f.C[i][j]) - A.h[i];
                }
            vol += (sg * f.TB[j] + B.h[j]) * clipped_area(B.h[k], B.h[l], la, lb, lc, 0u);
        }
    }
    return vol / 3.0;
}

__host__ __device__ double iou_distance(const Box& A, const Box& B, const Frame& f) {
    const double inter = fmax(intersection_volume(A, B, f), 0.0);
    const double v1 = 8.0 * (A.h[0] * A.h[1] * A.h[2]), v2 = 8.0 * (B.h[0] * B.h[1] * B.h[2]);
    const double uni = v1 + v2 - inter;
    return 1.0 - (uni > 0.0 ? inter / uni : 0.0);
}

// grid (tiles, tiles): block (x = column tile, y = row tile); the blocks below the diagonal exit at once
__global__ __launch_bounds__(THREADS) void ibl_obb_iou_tile_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ valid, int64_t n,
                                                                   double* __restrict__ dist, unsigned long long* __restrict__ n_overlap) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ double sA[BOX][TILE], sB[BOX][TILE];
    __shared__ int vA[TILE], vB[TILE];
    __shared__ double tile[TILE][TILE + 1];
    __shared__ unsigned short list[TILE * TILE];
    __shared__ int n_list;
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)bi * TILE, j0 = (int64_t)bj * TILE;
    const bool diag = bi == bj;
    if (tid == 0) n_list = 0;
    for (int e = tid; e < BOX * TILE; e += THREADS) {
        const int k = e / BOX, q = e - k * BOX;        // consecutive threads read consecutive doubles of the box rows
        sA[q][k] = i0 + k < n ? boxes[(i0 + k) * BOX + q] : 0.0;
        sB[q][k] = j0 + k < n ? boxes[(j0 + k) * BOX + q] : 0.0;
    }
    if (tid < TILE) {
        vA[tid] = i0 + tid < n ? valid[i0 + tid] : 0;
        vB[tid] = j0 + tid < n ? valid[j0 + tid] : 0;
    }
    __syncthreads();

    // phase 1: column c per thread (its box B in registers), rows r = tid / 64 + 4 t
    const int c = tid & (TILE - 1);
    Box B;
    load_box(sB, c, B);
    for (int r = tid >> 6; r < TILE; r += THREADS / TILE) {
        if (diag && r >= c) {
            if (r == c) tile[r][c] = 1.0;
            continue;
        }
        if (i0 + r >= n || j0 + c >= n) continue;
        if (vA[r] && vB[c]) {
            Box A;
            load_box(sA, r, A);
            Frame f;
            make_frame(A, B, f);
            if (!separated(A, B, f)) {
                const int slot = atomicAdd(&n_list, 1);
                list[slot] = (unsigned short)((r << 8) | c);
                continue;
            }
        }
        tile[r][c] = 1.0;      // an invalid box, or separated / touching boxes: IoU exactly 0
    }
    __syncthreads();

    // phase 2: exact volumes of the survivors
    const int cnt = n_list;
    for (int k = tid; k < cnt; k += THREADS) {
        const int r = list[k] >> 8, cc = list[k] & 0xff;
        Box A, Bx;
        load_box(sA, r, A);
        load_box(sB, cc, Bx);
        Frame f;
        make_frame(A, Bx, f);
        tile[r][cc] = iou_distance(A, Bx, f);
    }
    if (tid == 0 && cnt > 0) atomicAdd(n_overlap, (unsigned long long)cnt);      // integer count: order-independent
    __syncthreads();

    // out: rows of the tile (and, on the diagonal, their mirror), then the transposed tile
    for (int e = tid; e < TILE * TILE; e += THREADS) {
        const int r = e >> 6, cc = e & (TILE - 1);
        if (i0 + r >= n || j0 + cc >= n) continue;
        const double v = !diag || r <= cc ? tile[r][cc] : tile[cc][r];
        dist[(i0 + r) * n + j0 + cc] = v;
    }
    if (!diag)
        for (int e = tid; e < TILE * TILE; e += THREADS) {
            const int cc = e >> 6, r = e & (TILE - 1);
            if (i0 + r >= n || j0 + cc >= n) continue;
            dist[(j0 + cc) * n + i0 + r] = tile[r][cc];
        }
}

}  // namespace

extern "C" int ibl_obb_iou_matrix(ibl_reg_ctx* ctx, const double* boxes, const int32_t* valid, int64_t n, double* dist, int64_t* n_overlapping,
                                  void* stream) {
    if (!ctx || n < 0) return ibl_set_error(IBL_ERR_ARG, "ibl_obb_iou_matrix: bad argument");
    if (n_overlapping) *n_overlapping = 0;
    if (n == 0) return IBL_OK;
    if (!boxes || !valid || !dist) return ibl_set_error(IBL_ERR_ARG, "ibl_obb_iou_matrix: null buffer");
    const int64_t tiles = (n + TILE - 1) / TILE;
    if (tiles > 65535) return ibl_set_error(IBL_ERR_ARG, "ibl_obb_iou_matrix: at most %d objects (got %lld)", 65535 * TILE, (long long)n);
    hipStream_t s = (hipStream_t)stream;
    ArenaMark mark(ctx);
    unsigned long long* cnt;
    IBL_ARENA(cnt, unsigned long long, 1);
    IBL_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(ibl_obb_iou_tile_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(THREADS), 0, s, boxes, valid, n, dist, cnt);
    IBL_LAUNCH_CHECK();
    if (n_overlapping) {
        unsigned long long h = 0;
        IBL_HIP_CHECK(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, s));
        IBL_HIP_CHECK(hipStreamSynchronize(s));
        *n_overlapping = (int64_t)h;
    }
    return IBL_OK;
}
