// lh_probe.hip — test probes: the controllers' solves (lh_ldlt.h, lh_ctrl_g.hip) on a given system, the f64 MFMA
// lane layout.
// Not a unit of its own: lh_kernels.hip includes it (see there).

extern "C" {

// ---- LDL^T probe (tests): x = (S)^-1 b through k_ctrl's LDS layout and lds_ldlt_solve (natural
//      order, a dense envelope) or lds_pcg_solve, for a dense symmetric S (row-major n x n, n <= LH_NPAD) ----
__global__ __launch_bounds__(CT) void k_ldlt_probe(const double* __restrict__ S, const double* __restrict__ b, int n,
                                                   double* __restrict__ x, int solver, double tol, int max_it,
                                                   int* __restrict__ iters) {
    __shared__ double A[(NP + 1) * AS];
    __shared__ __attribute__((aligned(16))) double dg[NP];
    __shared__ __attribute__((aligned(16))) double xsol[NP];
    __shared__ uint16_t s_units[16 * LH_NSTEP];
    const int tid = threadIdx.x, NE = (n + 15) & ~15;
    if (tid == 0) {
        int32_t fcb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int order[15] = LH_ORDER_CTRL;
        lh_ctrl_units(n, fcb, order, 15, LH_NSTEP, s_units);
    }
    for (int e = tid; e < NE * NE; e += CT) {
        const int r = e / NE, c = e - NE * (e / NE);
        if (c <= r) A[r * AS + c] = (r < n) ? ((c < n) ? S[(size_t)r * n + c] : 0.0) : (r == c ? 1.0 : 0.0);
        else A[r * AS + c] = 0.0;
    }
    if (tid < NE) A[NP * AS + tid] = tid < n ? b[tid] : 0.0;
    lds_barrier();
    if (solver == 1) {
        __shared__ __attribute__((aligned(16))) double s_pcg[48];
        const int its = lds_pcg_solve(A, xsol, dg, s_pcg, n, tid, tol, (max_it > 0 ? max_it : 2 * n) + 1);
        if (tid == 0 && iters) *iters = its;
    } else {
        lds_ldlt_solve(A, xsol, n, NE, tid, nullptr, s_units);
    }
    lds_barrier();
    if (tid < n) x[tid] = xsol[tid];
}

// ---- the same probe through k_ctrl_g's global-memory solve (LH_NPAD < n <= 6 LH_PMAX_WIN):
//      gA: scratch of ceil32(n)^2 doubles ----
__global__ __launch_bounds__(GT) void k_ldlt_g_probe(const double* __restrict__ S, const double* __restrict__ b, int n,
                                                     double* __restrict__ x, double* __restrict__ gA) {
    __shared__ double pnl[GNMAX * GPS];
    __shared__ double dg[GNMAX], yv[GNMAX];
    __shared__ int perm[GNMAX], iperm[GNMAX];
    const int tid = threadIdx.x, NG = (n + GNB - 1) & ~(GNB - 1);
    for (int i = tid; i < n; i += GT) dg[i] = S[(size_t)i * n + i];
    lds_barrier();
    for (int row = tid; row < n; row += GT) {
        double di = fabs(dg[row]);
        if (!(di == di)) di = -1.0;
        int r = 0;
        for (int j = 0; j < n; ++j) {
            double d = fabs(dg[j]);
            if (!(d == d)) d = -1.0;
            r += (d > di) || (d == di && j < row);
        }
        perm[r] = row;
        iperm[row] = r;
    }
    lds_barrier();
    const bool all_zero = !(fabs(dg[perm[0]]) > 0.0);
    lds_barrier();
    if (all_zero)
        for (int i = tid; i < n; i += GT) { perm[i] = i; iperm[i] = i; }
    lds_barrier();
    for (int x2 = tid; x2 < NG * NG; x2 += GT) {
        const int r = x2 / NG, c = x2 - NG * (x2 / NG);
        double v = 0.0;
        if (r < n && c < n) v = (c <= r) ? S[(size_t)perm[r] * n + perm[c]] : 0.0;
        else if (r == c) v = 1.0;
        gA[x2] = v;
    }
    for (int i = tid; i < NG; i += GT) yv[i] = i < n ? b[perm[i]] : 0.0;
    __syncthreads();
    g_ldlt_solve(gA, NG, n, all_zero, yv, pnl);
    for (int i = tid; i < n; i += GT) x[perm[i]] = yv[i];
}

hipError_t lh_launch_ldlt_g_probe(const double* S, const double* b, int n, double* x, double* gA) {
    hipLaunchKernelGGL(k_ldlt_g_probe, dim3(1), dim3(GT), 0, 0, S, b, n, x, gA);
    return hipGetLastError();
}

hipError_t lh_launch_ldlt_probe(const double* S, const double* b, int n, double* x, int solver, double tol, int max_it,
                                int* iters) {
    if (n < 1 || n > LH_NPAD) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ldlt_probe, dim3(1), dim3(CT), 0, 0, S, b, n, x, solver, tol, max_it, iters);
    return hipGetLastError();
}

// ---- MFMA f64 layout probe (tests): D = A * B for 16x4 A, 4x16 B ----
__global__ void k_mfma_probe(const double* A, const double* B, double* D) {
    const int l = threadIdx.x;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i) D[((l >> 4) + 4 * i) * 16 + (l & 15)] = acc[i];
}

hipError_t lh_launch_mfma_probe(const double* A, const double* B, double* D) {
    hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, 0, A, B, D);
    return hipGetLastError();
}

}  // extern "C"
