// lh_ctrl_p.hip — k_ctrl_p, the PCG controller on the packed blocks, and its workgroup sum.
// Not a unit of its own: lh_kernels.hip includes it (see there).

// ============================================================================
// k_ctrl_p: the controller with the reduced pose system solved by PCG (lh_options.linear_solver =
// PCG) past LH_PMAX poses, up to LH_PMAX_ANY (windows of many keyframes).  One
// 1024-thread workgroup.  Same LM bookkeeping (ctrl_lm_step) and step tail (ctrl_step_tail) as the
// other controllers.  S stays in the packed blocks k_reduce wrote (rs: one 6x6 block per pose pair
// that some landmark couples, plus every diagonal block; lh_plan.cpp), never densified: the PCG's
// S p walks each pose's block row (Plan::brow_ent, ascending column) straight from the packed
// blocks, 6 rows per pose, one thread per row.  The algorithm is the reference's Problem::PCGSolver
// (problem.cpp:584-614) with its first-step bug fixed, as the oracle's pcg_solve restates it: Jacobi
// preconditioner on S + lambda D, stop when ||r|| <= pcg_tol ||b|| (1e-6, :597), at most 2 n steps
// after the first (:422); a zero diagonal preconditions with 0.  The dot products are fixed-order
// workgroup reductions (wave butterflies, then the 16 wave sums in order), so a solve is bitwise
// repeatable; the sums' order differs from the oracle's sequential loops (parity to tolerance).
// ============================================================================
constexpr int PNMAX = 6 * LH_PMAX_ANY;
constexpr int PRT = (PNMAX + CT - 1) / CT;   // rows per thread

// fixed-order workgroup sum of one value per thread (every thread gets the total); red: 16 doubles
__device__ __forceinline__ double wg_sum(double v, double* red, int lane, int wave) {
    double g[1] = {v};
    group_sum(g, 6);   // DPP and permlane butterflies, lane ^ 1 .. ^ 32
    v = g[0];
    if (lane == 0) red[wave] = v;
    lds_barrier();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < CT / 64; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(CT) void k_ctrl_p(lh_ctrl* __restrict__ ctrl, double* __restrict__ rs_commit,
                                               const double* __restrict__ rs_stage, const double* __restrict__ maxd_in,
                                               const int32_t* __restrict__ brow_ptr, const uint32_t* __restrict__ brow_ent,
                                               double* __restrict__ dxp, lh_params prm,
                                               int mode, volatile int* __restrict__ host_done, int seq,
                                               double* __restrict__ ell) {
    __shared__ double pv[PNMAX], bpv[PNMAX], hdv[PNMAX], xs[PNMAX];
    __shared__ __attribute__((aligned(16))) double s_red[3][CT / 64];
    __shared__ CtrlDecLds s_dec;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = prm.P, n = 6 * P;
    const lh_rs_layout LY = lh_rs_make(P, prm.npairs);

    // ---------------- the LM decision (workgroup `rung` > 0: a lambda-ladder rung with its own row copy of S) ----------------
    const int rung = (int)blockIdx.x;
    const CtrlDec dec = ctrl_take_decision<CT>(ctrl, prm, mode, rs_stage, LY, maxd_in, host_done, seq, s_red[0], s_dec);
    if (!dec.run) return;
    const int accept = dec.accept;
    const double lambda = dec.lambda;
    ell += (size_t)rung * prm.lad_stride;
    dxp += (size_t)rung * n;

    // ---------------- the chosen system (the candidate's on accept, committed on it; else the committed one) ----------------
    const double* __restrict__ src = accept ? rs_stage : rs_commit;
    if (accept && rung == 0)
        for (int i = tid; i < LY.total; i += CT) rs_commit[i] = rs_stage[i];
    const double* __restrict__ Sb = src + LY.off_S;
    // per thread rows r = tid + CT u: damped diagonal, Jacobi preconditioner, right-hand side
    double dr[PRT], minv[PRT], x[PRT], rr[PRT], z[PRT], pp[PRT];
    int e0[PRT], e1[PRT];
#pragma unroll
    for (int u = 0; u < PRT; ++u) {
        const int r = tid + CT * u;
        const bool in = r < n;
        const int p = in ? r / 6 : 0, a = r - 6 * p;
        e0[u] = in ? brow_ptr[p] : 0;
        e1[u] = in ? brow_ptr[p + 1] : 0;
        double sd = 0.0;
        for (int e = e0[u]; e < e1[u]; ++e) {   // the diagonal block: the entry whose column is p itself
            const uint32_t en = brow_ent[e];
            if ((int)((en >> 1) & 0xFFF) == p && !(en & 1u)) sd = Sb[(size_t)(en >> 13) * 36 + 7 * a];
        }
        dr[u] = (prm.strategy == 0) ? sd + lambda : sd + lambda * sd;   // problem.cpp:408-418
        minv[u] = (in && dr[u] != 0.0) ? 1.0 / dr[u] : 0.0;
        rr[u] = in ? src[LY.off_bs + r] : 0.0;
        x[u] = 0.0;
        z[u] = minv[u] * rr[u];
        pp[u] = z[u];
        if (in) { bpv[r] = src[LY.off_bp + r]; hdv[r] = src[LY.off_hd + r]; }
    }
    // Each row's entries gathered once per solve into row-contiguous scratch: entry e of pose p's block
    // row holds S(6p + a, 6q + c) at ell[(6 e + a) * 6 + c], the damped diagonal in place.  A step's
    // S p then reads 48 contiguous bytes per entry, at addresses that need no index word first (the
    // walk over the packed blocks put two dependent L2 round trips per entry on the chain).
#pragma unroll
    for (int u = 0; u < PRT; ++u) {
        const int r = tid + CT * u;
        if (r >= n) continue;
        const int p = r / 6, a = r - 6 * p;
        for (int e = e0[u]; e < e1[u]; ++e) {
            const uint32_t en = brow_ent[e];
            const int q = (int)((en >> 1) & 0xFFF);
            const double* blk = Sb + (size_t)(en >> 13) * 36;
            double* dst = ell + ((size_t)6 * e + a) * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                double val = (en & 1u) ? blk[6 * c + a] : blk[6 * a + c];   // (q, p) read transposed
                if (!(en & 1u) && q == p && c == a) val = dr[u];              // the damped diagonal
                dst[c] = val;
            }
        }
    }
    __syncthreads();   // the scratch is read back by the same threads: global stores visible to the loads below
    // Two barriers per step: z is published in pv and one product serves the step, q = (S + lambda D) z +
    // beta q_prev and p = z + beta p_prev (the same recurrence regrouped, as k_ctrl's PCG).  The dot
    // products are fixed-order sums (wave butterflies, then the 16 wave partials in order).
    double2* red2 = reinterpret_cast<double2*>(&s_red[1][0]);   // [16] (r.z, r.r) partials (s_red[1..2])
    double* red_pq = s_red[0];
    auto total2 = [&](double& tz, double& tr) {
        tz = 0.0;
        tr = 0.0;
#pragma unroll
        for (int w = 0; w < CT / 64; ++w) {
            const double2 t = red2[w];
            tz += t.x;
            tr += t.y;
        }
    };
    {
        double t2[2] = {0.0, 0.0};
#pragma unroll
        for (int u = 0; u < PRT; ++u) {
            t2[0] += rr[u] * z[u];
            t2[1] += rr[u] * rr[u];
            pp[u] = 0.0;
            if (tid + CT * u < n) pv[tid + CT * u] = z[u];
        }
        group_sum(t2, 6);
        if (lane == 0) red2[wave] = double2{t2[0], t2[1]};
    }
    lds_barrier();
    double rz, bb;
    total2(rz, bb);
    const double thr = prm.pcg_tol * sqrt(bb);
    const int maxit = prm.pcg_max_it > 0 ? prm.pcg_max_it : 2 * n;
    int steps = 0;
    double w[PRT], beta = 0.0;
#pragma unroll
    for (int u = 0; u < PRT; ++u) w[u] = 0.0;
    if (bb > 0.0) {
        for (;;) {
            // s = (S + lambda D) z, row by row over the block row, columns ascending
            double pw[1] = {0.0};
#pragma unroll
            for (int u = 0; u < PRT; ++u) {
                const int r = tid + CT * u;
                const int a = r - 6 * (r / 6);
                double acc = 0.0;
#pragma unroll 2
                for (int e = e0[u]; e < e1[u]; ++e) {
                    const int q = (int)((brow_ent[e] >> 1) & 0xFFF);
                    const double2* row = reinterpret_cast<const double2*>(ell + ((size_t)6 * e + a) * 6);
                    const double2 v0 = row[0], v1 = row[1], v2 = row[2];
                    const double* pq = pv + 6 * q;
                    acc += v0.x * pq[0];
                    acc += v0.y * pq[1];
                    acc += v1.x * pq[2];
                    acc += v1.y * pq[3];
                    acc += v2.x * pq[4];
                    acc += v2.y * pq[5];
                }
                w[u] = acc + beta * w[u];
                pp[u] = z[u] + beta * pp[u];
                pw[0] += pp[u] * w[u];
            }
            group_sum(pw, 6);
            if (lane == 0) red_pq[wave] = pw[0];
            lds_barrier();
            double tpw = 0.0;
#pragma unroll
            for (int wv = 0; wv < CT / 64; ++wv) tpw += red_pq[wv];
            const double alpha = rz / tpw;
            double a2[2] = {0.0, 0.0};
#pragma unroll
            for (int u = 0; u < PRT; ++u) {
                x[u] += alpha * pp[u];
                rr[u] -= alpha * w[u];
                z[u] = minv[u] * rr[u];
                a2[0] += rr[u] * z[u];
                a2[1] += rr[u] * rr[u];
                if (tid + CT * u < n) pv[tid + CT * u] = z[u];
            }
            group_sum(a2, 6);
            if (lane == 0) red2[wave] = double2{a2[0], a2[1]};
            lds_barrier();
            double rzn, rrn;
            total2(rzn, rrn);
            ++steps;
            if (!(sqrt(rrn) > thr) || steps >= maxit + 1) break;   // also stops on NaN
            beta = rzn / rz;
            rz = rzn;
        }
    }
#pragma unroll
    for (int u = 0; u < PRT; ++u) {
        const int r = tid + CT * u;
        if (r < n) { xs[r] = x[u]; dxp[r] = x[u]; }
    }
    if (tid == 0) {
        ctrl->lad_its[rung] = steps;
        if (rung == 0) ctrl->pcg_iters += steps;   // a higher rung's count is added when a rejection uses it
    }
    lds_barrier();
    ctrl_step_tail<CT>(ctrl, prm, n, lambda, xs, bpv, hdv, s_red[0], nullptr, rung);
}
