// reg_radius.hip -- radius-outlier counts on a batch grid (Open3D remove_radius_outlier, object_memory/object_memory.py:994-995).  A
// thread per point walks the cells in reach and stops at nb_points + 1: none of the neighbour selection is needed.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "reg_common.h"

// radius outlier: keep[i] = (#points with d2 < r2, self included) > nb_points.  Thread per point, early exit.
__global__ __launch_bounds__(256) void ibl_radius_count_kernel(BatchGrid g, const float4* __restrict__ pts, const int* __restrict__ seg_off,
                                                               float radius, float r2, int nb_points, unsigned char* __restrict__ keep) {
    const int n = seg_off[g.n_seg];
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= n) return;
    const SegGrid sg = g.seg[seg_of(seg_off, g.n_seg, qi)];
    const float4 q = pts[qi];
    int reach = (int)ceilf(radius * sg.inv);
    if (reach < 1) reach = 1;
    const int cx = cell_clamp(q.x, sg.minx, sg.inv, sg.nx), cy = cell_clamp(q.y, sg.miny, sg.inv, sg.ny),
              cz = cell_clamp(q.z, sg.minz, sg.inv, sg.nz);
    int cnt = 0;
    for (int z = max(cz - reach, 0); z <= min(cz + reach, sg.nz - 1) && cnt <= nb_points; ++z)
        for (int y = max(cy - reach, 0); y <= min(cy + reach, sg.ny - 1) && cnt <= nb_points; ++y) {
            const int row = sg.cell_base + (z * sg.ny + y) * sg.nx;
            const int b = g.cell_start[row + max(cx - reach, 0)], e = g.cell_start[row + min(cx + reach, sg.nx - 1) + 1];
            for (int j = b; j < e && cnt <= nb_points; j += 4) {         // four loads in flight (the walk is a chain of load latencies)
                float4 p[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) p[v] = g.sorted_pts[min(j + v, e - 1)];
#pragma unroll
                for (int v = 0; v < 4; ++v) cnt += (j + v < e && dist2f(q.x, q.y, q.z, p[v].x, p[v].y, p[v].z) < r2) ? 1 : 0;
            }
        }
    keep[qi] = cnt > nb_points ? 1 : 0;
}

int ibl_launch_radius_count(const BatchGrid& g, const float4* pts, const int* seg_off, int n, double radius, int nb_points,
                            unsigned char* keep, hipStream_t s) {
    if (n <= 0) return IBL_OK;
    hipLaunchKernelGGL(ibl_radius_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g, pts, seg_off, (float)radius,
                       (float)(radius * radius), nb_points, keep);
    IBL_LAUNCH_CHECK();
    return IBL_OK;
}
