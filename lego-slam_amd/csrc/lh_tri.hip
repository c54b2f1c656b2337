// lh_tri.hip — k_triangulate: legoslam::triangulation (include/legoslam/algorithm.h:11-34) for a batch of
// points, one lane per point, fp64 throughout (the arithmetic: lh_tri.h).
//
// A lane reads its views straight from global memory and streams their rows into a 4x4 triangular
// factor by Givens rotations, so any number of views costs the same registers; the one-sided Jacobi
// SVD of that factor is fully unrolled over its six column pairs (no register array is indexed at
// run time).  No lane reads another's data: a point's bits do not depend on its batch position or the
// batch size.  The pose table is small (2-3 poses at the frontend) and read-only: in the fixed-view
// layout its addresses are wave-uniform, in the CSR layout every lane's load hits the same few cache
// lines.  A lane whose sweeps have converged idles until its wave's last lane has.
#include <hip/hip_runtime.h>

#define LH_TRI_IMPL
#include "lh_launch.h"

#define TRI_BLOCK 64   // one wave per workgroup: frontend batches (~2000 points) then spread over 32 CUs

__global__ __launch_bounds__(TRI_BLOCK) void k_triangulate(lh_tri_args a) {
    const int64_t i = (int64_t)blockIdx.x * TRI_BLOCK + threadIdx.x;
    if (i >= a.n_points) return;
    lh_tri_point(a, i);
}

extern "C" hipError_t lh_launch_triangulate(hipStream_t st, const lh_tri_args* a) {
    if (a->n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)(((int64_t)a->n_points + TRI_BLOCK - 1) / TRI_BLOCK)), dim3(TRI_BLOCK),
                       0, st, *a);
    return hipGetLastError();
}
