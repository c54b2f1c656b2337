// lh_ctrl_g.hip — k_ctrl_g, the dense controller over global memory, with its solve g_ldlt_solve and k_dense.
// Not a unit of its own: lh_kernels.hip includes it (see there).

// ============================================================================
// k_ctrl_g: the controller for windows past LH_PMAX poses (21 < P <= LH_PMAX_WIN, 6P <= 384 rows).
// Same LM bookkeeping and pose tail as k_ctrl; the reduced system lives in global memory (gA,
// row-major, stride NG = ceil32(6P), L2-resident: <= 1.2 MB) instead of one CU's LDS.  Eigen's
// pivot order is the same static sort of |diag(S + lambda D)|.  The factorisation is a blocked
// right-looking LDL^T over 32-column panels:
//   (a) the panel (rows K.., columns K..K+31) into LDS;
//   (b) its 32x32 diagonal block by wave 0 in registers (lane r = row r; pivots and column
//       entries by lane broadcast);
//   (c) the panel rows below: one thread per row, 32 columns in registers;
//   (d) L and D back to gA;
//   (e) the trailing block, A_ij -= sum_k L_ik (D_k L_jk), as 16x16 f64 MFMA tiles (one wave per
//       tile, 8 MFMAs over the panel).
// Eigen semantics kept: a zero pivot skips the division (pivot_is_valid); if the largest |diag| is
// 0 there is no factorisation and the solves run on the raw matrix with identity transpositions.
// The triangular solves visit each row's terms in the oracle's order (ldlt_solve: ascending
// columns, 8-row panels whose zero entries skip in-panel updates; descending in L^T), so they
// are bitwise the oracle's solve of the same factor.  The factor's rounding differs from Eigen's
// left-looking dot products (parity to tolerance).
// ============================================================================
constexpr int GNB = 32;                 // panel width
constexpr int GNMAX = 6 * LH_PMAX_WIN;  // largest reduced system
constexpr int GPS = GNB + 1;            // LDS panel row stride (conflict-free column reads)
constexpr int GT = 512;                 // k_ctrl_g threads: 8 waves, 256 VGPRs (register rows in the factor)

// k_ctrl_g's reduced-system solve (shared with the probe): gA holds the permuted system's lower
// triangle (stride NG, identity padding to NG), yv the permuted right-hand side (LDS, n entries);
// on return yv holds the solution in pivot order and gA the factor.  All CT threads.
__device__ __forceinline__ void g_ldlt_solve(double* __restrict__ gA, int NG, int n, bool all_zero, double* yv,
                                             double* pnl) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ double ginv[GNB];   // 1/D of the current block's pivots (1 where the pivot is invalid)
    __shared__ double gdia[GNB];   // D of the current block's pivots
    CSTAMP(5);
    // ---------------- blocked right-looking LDL^T ----------------
    if (!all_zero) {
        for (int K = 0; K < NG; K += GNB) {
            const int m = NG - K;
            // (a) the panel into LDS (lower part of the diagonal block, all of the rows below)
            for (int x = tid; x < m * GNB; x += GT) {
                const int r = x / GNB, c = x - GNB * (x / GNB);
                pnl[r * GPS + c] = (r >= c) ? gA[(size_t)(K + r) * NG + K + c] : 0.0;
            }
            lds_barrier();
            CSTAMP(13);
            // (b) the diagonal block: wave 0, lane j holds column j of the full symmetric block in
            //     registers (c[i] = A(i, j)).  Step k: D_k and the column k entries come from lane k
            //     by readlane (uniform values); lane j's own L(j, k) is its register c[k] (the
            //     symmetric copy), so nothing is indexed per lane and nothing goes through memory.
            if (wave == 0) {
                const int j = lane & (GNB - 1);
                double c[GNB];
#pragma unroll
                for (int i = 0; i < GNB; ++i) c[i] = (i >= j) ? pnl[i * GPS + j] : pnl[j * GPS + i];
#pragma unroll
                for (int k = 0; k < GNB; ++k) {
                    const double d = readlane_d(c[k], k);
                    const double id = (fabs(d) > 0.0) ? fast_rcp(d) : 1.0;   // pivot_is_valid: no division
                    const double wj = d * (c[k] * id);                        // D_k L(j, k)
#pragma unroll
                    for (int i = k + 1; i < GNB; ++i) {
                        const double lik = readlane_d(c[i], k) * id;          // L(i, k), uniform
                        c[i] -= lik * wj;
                    }
                    // row j of column k becomes L(j, k) for j > k; lanes j <= k scale entries they never
                    // read again (the diagonal D_k is kept in gdia), so no lane masks are needed
                    c[k] *= id;
                    if (lane == 0) { ginv[k] = id; gdia[k] = d; }
                }
                // lane j ends with row j of the factor: c[i] = L(j, i) for i < j (its symmetric copies,
                // scaled at step i); the rest of its row is written too (the upper part is overwritten
                // by (c), the diagonal below)
                if (lane < GNB) {
#pragma unroll
                    for (int i = 0; i < GNB; ++i) pnl[j * GPS + i] = c[i];
                }
                wave_sync();
                if (lane < GNB) pnl[lane * GPS + lane] = gdia[lane];
            }
            lds_barrier();
            CSTAMP(14);
            // (c) the panel rows below the block.  W = D_k L(j, k) (j > k) into the diagonal block's
            //     free upper triangle; each row in registers, right-looking: the same operations and
            //     roundings as the diagonal block's rows.
            if (wave == 0 && lane < GNB)
                for (int j = lane + 1; j < GNB; ++j) pnl[lane * GPS + j] = pnl[lane * GPS + lane] * pnl[j * GPS + lane];
            lds_barrier();
            // the W rows' LDS addresses off an opaque zero: one base register and immediate offsets (with
            // constant addresses the compiler kept ~160 of them in VGPRs across the loop, and spilled)
            int z0 = 0;
            asm volatile("" : "+v"(z0));
            for (int r = GNB + tid; r < m; r += GT) {
                double a[GNB];
#pragma unroll
                for (int c = 0; c < GNB; ++c) a[c] = pnl[r * GPS + c];
#pragma unroll
                for (int k = 0; k < GNB; ++k) {
                    const double l = a[k] * ginv[k];
                    a[k] = l;
#pragma unroll
                    for (int j = k + 1; j < GNB; ++j) a[j] -= l * pnl[z0 + k * GPS + j];
                    __builtin_amdgcn_sched_barrier(0);   // one step's loads at a time (register budget)
                }
#pragma unroll
                for (int c = 0; c < GNB; ++c) pnl[r * GPS + c] = a[c];
            }
            lds_barrier();
            CSTAMP(15);
            // (d) L and D of the panel back to gA
            for (int x = tid; x < m * GNB; x += GT) {
                const int r = x / GNB, c = x - GNB * (x / GNB);
                if (r >= c) gA[(size_t)(K + r) * NG + K + c] = pnl[r * GPS + c];
            }
            // (e) trailing block: 16x16 tiles (I >= J), four per wave at a time (their loads in flight
            //     together), 8 f64 MFMAs per tile over the panel
            const int mt = (m - GNB) >> 4;
            const int ntiles = mt * (mt + 1) / 2;
            for (int t0 = 4 * wave; t0 < ntiles; t0 += 4 * (GT / 64)) {
                int I[4], J[4];
                v4d acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = min(t0 + u, ntiles - 1);
                    int ii = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                    while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
                    while (ii * (ii + 1) / 2 > t) --ii;
                    I[u] = ii;
                    J[u] = t - ii * (ii + 1) / 2;
                    const int r0 = K + GNB + 16 * I[u], c0 = K + GNB + 16 * J[u];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = gA[(size_t)(r0 + (lane >> 4) + 4 * v) * NG + c0 + (lane & 15)];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int kk = 0; kk < GNB; kk += 4) {
                        const int k = kk + (lane >> 4);
                        const double av = -pnl[(GNB + 16 * I[u] + (lane & 15)) * GPS + k];
                        const double bv = pnl[k * GPS + k] * pnl[(GNB + 16 * J[u] + (lane & 15)) * GPS + k];
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[u], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u >= ntiles) break;
                    const int r0 = K + GNB + 16 * I[u], c0 = K + GNB + 16 * J[u];
#pragma unroll
                    for (int v = 0; v < 4; ++v) gA[(size_t)(r0 + (lane >> 4) + 4 * v) * NG + c0 + (lane & 15)] = acc[u][v];
                }
            }
            __syncthreads();
            CSTAMP(16);
        }
    }

    CSTAMP(6);
    // the factor's diagonal blocks into LDS (the panel buffer is free now): block b's rows at
    // pnl[(32 b + r) * GPS + c], one round trip for all of them
    for (int x = tid; x < n * GNB; x += GT) {
        const int r = x / GNB, c = x - GNB * (x / GNB);
        const int K = r & ~(GNB - 1);
        pnl[r * GPS + c] = (K + c < n) ? gA[(size_t)r * NG + K + c] : 0.0;
    }
    lds_barrier();
    // ---------------- forward substitution (unit L), the oracle's order ----------------
    static_assert(GNMAX <= GT, "one row per thread in the solves' row updates");
    for (int K = 0; K < n; K += GNB) {
        const int kb = min(GNB, n - K);
        // the block's columns of the rows below: loaded first (they do not depend on the solve), so
        // their latency overlaps the diagonal block's chain
        const int ib = K + kb + tid;
        double Lb[GNB];
#pragma unroll
        for (int k = 0; k < GNB; ++k) Lb[k] = (ib < n && k < kb) ? gA[(size_t)ib * NG + K + k] : 0.0;
        if (wave == 0) {
            const int r = lane & (GNB - 1);
            double x = yv[K + r];
            double Lr[GNB];
#pragma unroll
            for (int k = 0; k < GNB; ++k) Lr[k] = (r > k && K + r < n) ? pnl[(K + r) * GPS + k] : 0.0;
#pragma unroll
            for (int k = 0; k < GNB; ++k) {
                const double xk = readlane_d(x, k);   // uniform: an SGPR pair, no LDS round trip
                if (k < kb && r > k && r < kb) {
                    const bool same_panel = (r >> 3) == (k >> 3);
                    if (!same_panel || xk != 0.0) x -= Lr[k] * xk;
                }
            }
            if (lane < kb) yv[K + lane] = x;
        }
        lds_barrier();
        if (ib < n) {   // the block's columns, ascending
            double x = yv[ib];
#pragma unroll
            for (int k = 0; k < GNB; ++k)
                if (k < kb) x -= Lb[k] * yv[K + k];
            yv[ib] = x;
        }
        lds_barrier();
    }
    // D^+ (tolerance: numeric_limits<double>::min())
    for (int i = tid; i < n; i += GT) {
        const double d = pnl[i * GPS + (i & (GNB - 1))];
        yv[i] = (fabs(d) > 2.2250738585072014e-308) ? yv[i] / d : 0.0;
    }
    lds_barrier();
    // ---------------- back substitution (L^T), descending ----------------
    for (int K = ((n - 1) / GNB) * GNB; K >= 0; K -= GNB) {
        const int kb = min(GNB, n - K);
        const int ia = tid;   // the rows above the block: their L^T entries, loaded ahead as above
        double La[GNB];
#pragma unroll
        for (int k = 0; k < GNB; ++k) La[k] = (ia < K && k < kb) ? gA[(size_t)(K + k) * NG + ia] : 0.0;
        if (wave == 0) {
            const int r = lane & (GNB - 1);
            double x = yv[K + r];
            double Lc[GNB];
#pragma unroll
            for (int k = 0; k < GNB; ++k) Lc[k] = (k > r && k < kb) ? pnl[(K + k) * GPS + r] : 0.0;
#pragma unroll
            for (int k = GNB - 1; k >= 0; --k) {
                const double xk = readlane_d(x, k);
                if (k < kb && r < k) x -= Lc[k] * xk;
            }
            if (lane < kb) yv[K + lane] = x;
        }
        lds_barrier();
        if (ia < K) {   // the block's rows, descending
            double x = yv[ia];
#pragma unroll
            for (int k = GNB - 1; k >= 0; --k)
                if (k < kb) x -= La[k] * yv[K + k];
            yv[ia] = x;
        }
        lds_barrier();
    }
    CSTAMP(7);
}

// k_dense: the reduced system's S blocks (packed per pose pair, p <= q) into the dense symmetric n x n
// matrix gS[1 - cur] (stride NG) that k_ctrl_g gathers from in pivot order.  One 64-thread block per
// pair, launched after the exchange (when there is one) and before k_ctrl_g; gS is double-buffered
// with the committed state (ctrl->cur), so a rejected trial keeps the committed copy.
__global__ __launch_bounds__(64) void k_dense(const double* __restrict__ rs, const uint16_t* __restrict__ pair_pq,
                                              const lh_ctrl* __restrict__ ctrl, double* __restrict__ gS, int P, int NG) {
    const int done = __builtin_amdgcn_readfirstlane(ctrl->done);
    const int evo = __builtin_amdgcn_readfirstlane(ctrl->evo);   // k_reduce wrote no S blocks
    const int cur = __builtin_amdgcn_readfirstlane(ctrl->cur);
    if (done || evo) return;
    const lh_rs_layout LY = lh_rs_make(P, P * (P + 1) / 2);   // the dense packed layout (P <= LH_PMAX_WIN)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int p = pair_pq[2 * b], q = pair_pq[2 * b + 1];
    if (lane >= 36) return;
    const int a = lane / 6, c = lane - 6 * (lane / 6);
    const double v = rs[LY.off_S + b * 36 + lane];
    double* g = gS + (size_t)(1 - cur) * NG * NG;
    g[(size_t)(6 * p + a) * NG + 6 * q + c] = v;
    if (p != q) g[(size_t)(6 * q + c) * NG + 6 * p + a] = v;   // a diagonal block has both halves already
}

__global__ __launch_bounds__(GT) void k_ctrl_g(lh_ctrl* __restrict__ ctrl, double* __restrict__ rs_commit,
                                               const double* __restrict__ rs_stage, const double* __restrict__ maxd_in,
                                               const uint32_t* __restrict__ rsmap,
                                               double* __restrict__ dxp, lh_params prm, int mode,
                                               volatile int* __restrict__ host_done, int seq, double* __restrict__ gA,
                                               const double* __restrict__ gS) {
    __shared__ double pnl[GNMAX * GPS];
    __shared__ double dg[GNMAX], bsv[GNMAX], bpv[GNMAX], hdv[GNMAX], xs[GNMAX], yv[GNMAX], gkey[GNMAX];
    __shared__ int perm[GNMAX], iperm[GNMAX];
    __shared__ double s_red[GT / 64];
    __shared__ CtrlDecLds s_dec;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = prm.P, n = 6 * P, NG = (n + GNB - 1) & ~(GNB - 1);
    const lh_rs_layout LY = lh_rs_make(P, prm.npairs);
    CSTAMP_START;

    // ---------------- the LM decision (workgroup `rung` > 0: a lambda-ladder rung with its own gA) ----------------
    const int rung = (int)blockIdx.x;
    const CtrlDec dec = ctrl_take_decision<GT>(ctrl, prm, mode, rs_stage, LY, maxd_in, host_done, seq, s_red, s_dec);
    if (!dec.run) return;
    const int accept = dec.accept, cur = dec.cur;
    const double lambda = dec.lambda;
    gA += (size_t)rung * prm.lad_stride;
    dxp += (size_t)rung * n;

    CSTAMP_LIVE();
    CSTAMP(1);

    // ---------------- diagonal + lambda and right-hand sides (one round trip) ----------------
    // S of the chosen system is k_dense's dense copy gS[cur] (cur after the decision: the candidate's
    // on accept, the committed one on reject); the right-hand sides come from the packed system.
    const double* __restrict__ src = accept ? rs_stage : rs_commit;
    const double* __restrict__ gSc = gS + (size_t)cur * NG * NG;
    for (int i = tid; i < n; i += GT) {
        const double v = gSc[(size_t)i * NG + i];
        dg[i] = (prm.strategy == 0) ? v + lambda : v + lambda * v;
        bsv[i] = src[LY.off_bs + i];
        bpv[i] = src[LY.off_bp + i];
        hdv[i] = src[LY.off_hd + i];
    }
    lds_barrier();
    CSTAMP(2);

    // ---------------- pivot order: |diag| descending, ties by index, NaN last (as k_ctrl) ----------------
    for (int i = tid; i < n; i += GT) {   // the sort keys once
        const double d = fabs(dg[i]);
        gkey[i] = (d == d) ? d : -1.0;
    }
    lds_barrier();
    for (int row = tid; row < n; row += GT) {
        const double di = gkey[row];
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < n; ++j) {
            const double d = gkey[j];
            r += (d > di) || (d == di && j < row);
        }
        perm[r] = row;
        iperm[row] = r;
    }
    lds_barrier();
    // Eigen's k = 0 test: the largest |diag| is not > 0 -> identity transpositions, no factorisation
    const bool all_zero = !(fabs(dg[perm[0]]) > 0.0);
    lds_barrier();
    if (all_zero)
        for (int i = tid; i < n; i += GT) { perm[i] = i; iperm[i] = i; }
    lds_barrier();
    CSTAMP(3);

    // ---------------- commit (the packed right-hand sides), gather gA (permuted lower triangle) ----------------
    // S itself is double-buffered as gS (the decision picked the buffer): only the part after it commits
    if (accept && rung == 0)
        for (int i = LY.off_bs + tid; i < LY.total; i += GT) rs_commit[i] = src[i];
    // gA(r, c) = S(perm r, perm c), r > c: a wave per row (lanes over columns), so its stores are
    // contiguous and its loads fall in one row of gS; eight rows per wave at a time, 48 loads in flight
    static_assert(GNMAX <= 6 * 64, "six 64-column chunks cover a row");
    for (int r0 = wave; r0 < NG; r0 += 8 * (GT / 64)) {
        double v[8][6];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = r0 + u * (GT / 64);
            const int pr = (r < n) ? perm[r] : 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int c = 64 * j + lane;
                v[u][j] = (c < r && r < n) ? gSc[(size_t)pr * NG + perm[c]] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = r0 + u * (GT / 64);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int c = 64 * j + lane;
                if (c < r && r < NG) gA[(size_t)r * NG + c] = v[u][j];
            }
        }
    }
    for (int i = tid; i < NG; i += GT) {
        gA[(size_t)i * NG + i] = i < n ? dg[perm[i]] : 1.0;
        yv[i] = i < n ? bsv[perm[i]] : 0.0;
    }
    __syncthreads();   // global stores before the panel loads
    CSTAMP(4);
    g_ldlt_solve(gA, NG, n, all_zero, yv, pnl);
    for (int i = tid; i < n; i += GT) { xs[perm[i]] = yv[i]; dxp[perm[i]] = yv[i]; }
    lds_barrier();
    CSTAMP(8);
    ctrl_step_tail<GT>(ctrl, prm, n, lambda, xs, bpv, hdv, s_red, nullptr, rung);
    CSTAMP(12);
    CSTAMP_END();
}
