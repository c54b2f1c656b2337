// lh_frames.hip — k_frames: pose-only optimisation of single frames.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lh_launch.h"
#include "lh_dev.h"
#include "lh_edge.h"

// ============================================================================
// k_frames: the frontend's pose-only LM, Frontend::EstimateCurrentPose
// (src/frontend_lego.cpp:157-250), one workgroup per frame, the whole thing in
// one launch: four rounds of problem.solve(10) on one VertexPose with
// EdgeProjectionPoseOnly edges (lego_types.h:116-180), each round restarting
// from the frame's pose, then the outlier flags (:205-226); the edges lose the
// Huber cost after round three (:223-225).  Edges are never removed (the
// reference's setLevel is commented out).  n = 6: the Schur complement is H_pp
// itself (problem.cpp:380-430 with no landmark vertex), solved by wave 0 in
// registers with Eigen's pivoted LDLT (po_ldlt6_wave).  Per-edge arithmetic is the bitwise mirror of
// oracle/lego_oracle.c (po_residual / po_jacobian); sums have a fixed order
// (thread-strided, then a fixed tree), so a batch is bitwise reproducible.
// ============================================================================
#define FT 256                 // threads per frame
#define FV 28                  // per-edge sums: H_pp upper (21) | b (6) | rho0
#pragma clang fp contract(off)

// EdgeProjectionPoseOnly residual + Jacobian at pos_cam = T X (one transform for both)
__device__ __forceinline__ void po_edge(const double* q, const double* t, const double X[3], double u, double v,
                                        const double* K, double& r0, double& r1, double J[12], bool want_j) {
    double Pc[3];
    d_q_rotate(q, X, Pc);
#pragma unroll
    for (int i = 0; i < 3; ++i) Pc[i] = Pc[i] + t[i];
    double p0 = K[0] * Pc[0] + K[2] * Pc[2];
    double p1 = K[1] * Pc[1] + K[3] * Pc[2];
    const double den = Pc[2] + 1e-18;
    p0 /= den;
    p1 /= den;
    r0 = u - p0;
    r1 = v - p1;
    if (want_j) {
        const double fx = K[0], fy = K[1];
        const double x = Pc[0], y = Pc[1], z = Pc[2];
        const double zi = 1.0 / (z + 1e-18);
        const double zi2 = zi * zi;
        J[0] = -fx * zi;              J[1] = 0.0;                  J[2] = fx * x * zi2;
        J[3] = fx * x * y * zi2;      J[4] = -fx - fx * x * x * zi2; J[5] = fx * y * zi;
        J[6] = 0.0;                   J[7] = -fy * zi;             J[8] = fy * y * zi2;
        J[9] = fy + fy * y * y * zi2; J[10] = -fy * x * y * zi2;   J[11] = -fy * x * zi;
    }
}

__device__ __forceinline__ double po_rho0(double r0, double r1, double delta) {
    const double e2 = r0 * r0 + r1 * r1;
    if (delta > 0.0) {
        const double d2 = delta * delta;
        if (e2 <= d2) return e2;
        const double s = sqrt(e2);
        return 2 * s * delta - d2;
    }
    return e2;
}

// one edge's contributions: (J^T W) J upper triangle, -(rho1 J)^T r, rho0  (problem.cpp:300-330).
// The products contract to FMAs: these sums are parity-to-tolerance (their order differs from the oracle's
// anyway); edge_robust keeps the bitwise-mirrored gate (contraction is fixed where an expression is written).
#pragma clang fp contract(fast)
__device__ __forceinline__ void po_accumulate(double r0, double r1, const double J[12], double delta, double acc[FV]) {
    EdgeEval E;
    E.r0 = r0; E.r1 = r1;
    lh_params pr{};
    pr.huber_delta = delta;
    edge_robust(E, pr);
    double JtW[12];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        JtW[2 * a] = J[a] * E.W00 + J[6 + a] * E.W10;
        JtW[2 * a + 1] = J[a] * E.W01 + J[6 + a] * E.W11;
    }
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = a; c < 6; ++c) acc[k++] += JtW[2 * a] * J[c] + JtW[2 * a + 1] * J[6 + c];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] -= (E.rho1 * J[a]) * r0 + (E.rho1 * J[6 + a]) * r1;
    acc[27] += E.rho0;
}
#pragma clang fp contract(off)

// The oracle's ldlt_solve (Eigen ldlt_inplace with diagonal pivoting + LDLT::_solve_impl) for n = 6,
// in registers: every lane holds the whole symmetric system and runs the oracle's operations in the
// oracle's order, so no value crosses lanes.  Two changes: multiply-adds contract to FMAs, and a division
// by a pivot is its reciprocal (fast_rcp, one per pivot) times the element, as the k_ctrl LDL^T does.  The
// frontend's sums of H and b already differ from the oracle's order, so its parity is to tolerance
// either way (tests/test_frontend.py), and the 21 IEEE divisions were the longest part of the step.
// The damped system is read from LDS (H full symmetric, b), with Eigen's pivot sequence found first: Eigen's left-looking ldlt_inplace compares diagonal entries no earlier step has changed, so its
// transpositions depend on the damped diagonal alone.  They are replayed on six (key, row) pairs, the
// permuted system is loaded from LDS at the permuted addresses, the factorisation and the solves run
// without swaps (the same operations on the same values as Eigen's in-place swapping loop, so the same
// bits as a swapping version), and x goes back to pose order through LDS.  This keeps the 36-element row
// and column exchanges (a branch per candidate row per step) off the chain.
#pragma clang fp contract(fast)   // the 6x6 solve is parity-to-tolerance (see above): FMAs halve its chains
__device__ __forceinline__ void po_ldlt6_lds(const double* H, const double* bv, double lam, int strategy,
                                             double* xs, double (&x)[6]) {
    double key[6];
    int pos[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double h = H[7 * i];
        key[i] = h + ((strategy == 0) ? lam : lam * h);
        pos[i] = i;
    }
    bool all_zero = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int idx = k;
        double big = fabs(key[k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double di = fabs(key[i]);
            if (di > big) { big = di; idx = i; }
        }
        idx = __builtin_amdgcn_readfirstlane(idx);
        if (k == 0 && !(big > 0.0)) { all_zero = true; break; }   // Eigen: identity transpositions
#pragma unroll
        for (int m = k + 1; m < 6; ++m)
            if (m == idx) {
                const double t = key[k]; key[k] = key[m]; key[m] = t;
                const int u = pos[k]; pos[k] = pos[m]; pos[m] = u;
            }
    }
    double A[6][6], y[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) A[r][c] = H[6 * pos[r] + pos[c]];
        A[r][r] += (strategy == 0) ? lam : lam * A[r][r];
        y[r] = bv[pos[r]];
    }
    if (!all_zero) {
        double dd[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (k > 0) {
                double temp[6];
#pragma unroll
                for (int j = 0; j < k; ++j) temp[j] = dd[j] * A[k][j];
#pragma unroll
                for (int r = k; r < 6; ++r) {
                    double si = 0.0;
#pragma unroll
                    for (int j = 0; j < k; ++j) si += A[r][j] * temp[j];
                    A[r][k] -= si;
                }
            }
            const double akk = A[k][k];
            dd[k] = akk;
            if (k < 5 && fabs(akk) > 0.0) {
                const double inv = fast_rcp(akk);
#pragma unroll
                for (int r = k + 1; r < 6; ++r) A[r][k] *= inv;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (y[k] != 0.0)
#pragma unroll
            for (int i = k + 1; i < 6; ++i) y[i] -= A[i][k] * y[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double d = A[i][i];
        y[i] = (fabs(d) > 2.2250738585072014e-308) ? y[i] * fast_rcp(d) : 0.0;
    }
#pragma unroll
    for (int k = 5; k >= 0; --k)
#pragma unroll
        for (int i = 0; i < k; ++i) y[i] -= A[k][i] * y[k];
#pragma unroll
    for (int r = 0; r < 6; ++r) xs[pos[r]] = y[r];   // every lane writes the same value
    wave_sync();
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = xs[j];
}

#pragma clang fp contract(off)
// sin and cos of |x| <= 0.8 by their Taylor series to x^17 / x^18 in Horner form on x^2 (the next terms are
// below 1e-19): within 1 ulp of the host libm's sin / cos (2e7 samples, 1-2 % of them 1 ulp apart; the
// device library's sincos is not bitwise the host's either).  A frame's pose step is small, so its angle
// takes this path; larger ones take the library's sincos.
__device__ __forceinline__ void po_sincos_small(double x, double& s, double& c) {
    const double x2 = x * x;
    double p = -8.22063524662433e-18;
    p = __builtin_fma(p, x2, 2.8114572543455206e-15);
    p = __builtin_fma(p, x2, -7.647163731819816e-13);
    p = __builtin_fma(p, x2, 1.6059043836821613e-10);
    p = __builtin_fma(p, x2, -2.505210838544172e-08);
    p = __builtin_fma(p, x2, 2.7557319223985893e-06);
    p = __builtin_fma(p, x2, -0.0001984126984126984);
    p = __builtin_fma(p, x2, 0.008333333333333333);
    p = __builtin_fma(p, x2, -0.16666666666666666);
    s = __builtin_fma(x * x2, p, x);
    double q = 4.110317623312165e-19;
    q = __builtin_fma(q, x2, -1.5619206968586225e-16);
    q = __builtin_fma(q, x2, 4.779477332387385e-14);
    q = __builtin_fma(q, x2, -1.1470745597729725e-11);
    q = __builtin_fma(q, x2, 2.08767569878681e-09);
    q = __builtin_fma(q, x2, -2.755731922398589e-07);
    q = __builtin_fma(q, x2, 2.48015873015873e-05);
    q = __builtin_fma(q, x2, -0.001388888888888889);
    q = __builtin_fma(q, x2, 0.041666666666666664);
    q = __builtin_fma(q, x2, -0.5);
    c = __builtin_fma(x2, q, 1.0);
}
// the library's sincos out of line (its registers are not live across the frame's pose update)
__device__ __attribute__((noinline)) double2 po_sincos_libm(double x) {
    double s, c;
    sincos(x, &s, &c);
    return double2{s, c};
}
// VertexPose::add: T12 <- (SE3::exp(d) * SE3(T12)).matrix(), NaN/Inf step -> zero (lego_types.h:61-91),
// on one wave: every lane computes the same result, except that lane 0 takes sin/cos(theta/2) and
// lane 1 sin/cos(theta) in one sincos pass.  qT = the quaternion of SE3(T12) (d_q_from_R of its
// rotation), cached by the caller.  out12: the new pose matrix (every lane), q/t: its SE3 table.
__device__ __forceinline__ void po_pose_add_wave(const double (&d_in)[6], const double* T12, const double* qT,
                                                 double (&out12)[12], double (&qo)[4], double (&to)[3], int lane) {
    double d[6];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 6; ++a) { d[a] = d_in[a]; bad |= !isfinite(d[a]); }
    if (bad) {
#pragma unroll
        for (int a = 0; a < 6; ++a) d[a] = 0.0;
    }
    const double th = d_twist_theta(d);
    double sn, cs;
    const double ang = lane == 1 ? th : 0.5 * th;
#ifndef LH_PO_LIBM_SINCOS
    if (__builtin_amdgcn_readfirstlane((int)(th <= 0.8)))   // th: the same in every lane
        po_sincos_small(ang, sn, cs);
    else
    {
        const double2 r = po_sincos_libm(ang);
        sn = r.x;
        cs = r.y;
    }
#else
    sincos(ang, &sn, &cs);
#endif
    const double sh = readlane_d(sn, 0), ch = readlane_d(cs, 0), st = readlane_d(sn, 1), ct = readlane_d(cs, 1);
    double qe[4], te[3], qn[4], tr[3], Rn[9];
    d_se3_exp_trig(d, sh, ch, st, ct, qe, te);
    const double qTr[4] = {qT[0], qT[1], qT[2], qT[3]};
    const double tc[3] = {T12[3], T12[7], T12[11]};
    d_q_mul(qe, qTr, qn);
    d_q_rotate(qe, tc, tr);
    d_R_from_q(qn, Rn);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out12[4 * i] = Rn[3 * i]; out12[4 * i + 1] = Rn[3 * i + 1]; out12[4 * i + 2] = Rn[3 * i + 2];
        out12[4 * i + 3] = te[i] + tr[i];
    }
    // SE3(estimate_) of the new matrix, as the next linearisation reads it
    const double R[9] = {out12[0], out12[1], out12[2], out12[4], out12[5], out12[6], out12[8], out12[9], out12[10]};
    d_q_from_R(R, qo);
    to[0] = out12[3]; to[1] = out12[7]; to[2] = out12[11];
}

#pragma clang fp contract(fast)

struct PoShared {
    double pose[12], cand[12], q[4], t[3], qp[4], K[4];   // q/t: the table being linearised; qp: SE3(pose)'s q
    double H[36], b[6], dx[6], xs[6];   // xs: the 6x6 solution on its way back to pose order
    double part[FT / 64][FV];
    double sum[FV];
    double rows[FT][FV + 1];   // one thread's per-edge sums per row (odd stride: column reads spread over banks)
    double chi, lam, ni, last, delta;
    int iter, fc, cont;        // completed iterations, rejected trials in the iteration, another trial follows
};

// all FT threads: each thread's acc[FV] through LDS rows; per wave, lane 2k + h (k < FV) sums column k
// over the wave's rows of parity h (four interleaved chains, fixed order), and the two halves are added: S.part[wave].
// The caller's barrier follows.  Fixed order: a batch is bitwise reproducible.
__device__ __forceinline__ void po_rows_to_parts(const double (&acc)[FV], PoShared& S, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < FV; ++k) S.rows[tid][k] = acc[k];
    wave_sync();
    if (lane < 2 * FV) {
        const int k = lane >> 1, h = lane & 1;
        // four interleaved chains (rows i mod 4), then ((c0 + c1) + (c2 + c3)): a fixed order, a quarter of the
        // dependent adds
        double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 32; ++i) c[i & 3] += S.rows[64 * wave + 2 * i + h][k];
        double s = (c[0] + c[1]) + (c[2] + c[3]);
        s += dpp_d<0xB1>(s);   // quad_perm [1,0,3,2]: the other parity's half
        if (h == 0) S.part[wave][k] = s;
    }
}

// SE3(estimate_) of T12 into q / t (d_q_from_R of its rotation)
__device__ __forceinline__ void po_table_regs(const double* T12, double (&q)[4], double (&t)[3]) {
    const double R[9] = {T12[0], T12[1], T12[2], T12[4], T12[5], T12[6], T12[8], T12[9], T12[10]};
    d_q_from_R(R, q);
    t[0] = T12[3]; t[1] = T12[7]; t[2] = T12[11];
}

// One workgroup per frame.  Per LM trial there are two barriers: after the linearisation's per-wave
// sums, and after wave 0 has finished the sums, taken the LM decision (lane 0) and, when another
// trial follows, solved the 6x6 step and composed the candidate pose (all of wave 0).
__global__ __launch_bounds__(FT) void k_frames(const int64_t* __restrict__ obs_ptr, const double* __restrict__ pose_in,
                                               const double* __restrict__ pts, const double* __restrict__ uv,
                                               const uint8_t* __restrict__ flag_in, lh_params prm,
                                               double* __restrict__ res, double* __restrict__ pose_out,
                                               uint8_t* __restrict__ flag_out, double* __restrict__ rchi2_out,
                                               int32_t* __restrict__ iters_out, int32_t* __restrict__ inliers_out) {
    __shared__ PoShared S;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t o0 = obs_ptr[f];
    const int O = (int)(obs_ptr[f + 1] - o0);
    const double* X = pts + 3 * o0;
    const double* Z = uv + 2 * o0;
    double* R = res + 2 * o0;
    uint8_t* flag = flag_out + o0;
    for (int e = tid; e < O; e += FT) flag[e] = flag_in ? (flag_in[o0 + e] != 0) : 0;
    if (tid < 4) S.K[tid] = prm.K[tid];
    if (tid == 0) S.delta = prm.huber_delta;
    int its = 0;
    STAMP_DECL   // diagnostic build: per-phase wave-cycles into lh_stamps[24..29]
    // this thread's first edge, in registers for the whole launch (a frame of <= FT edges then reads
    // no edge input from memory after this; further edges are read per pass)
    double X0[3] = {0.0, 0.0, 0.0}, Z0[2] = {0.0, 0.0};
    if (tid < O) {
        X0[0] = X[3 * tid]; X0[1] = X[3 * tid + 1]; X0[2] = X[3 * tid + 2];
        Z0[0] = Z[2 * tid]; Z0[1] = Z[2 * tid + 1];
    }
    auto edge_in = [&](int e, double (&Xe)[3], double& u, double& v) __attribute__((always_inline)) {
        if (e == tid) {
            Xe[0] = X0[0]; Xe[1] = X0[1]; Xe[2] = X0[2]; u = Z0[0]; v = Z0[1];
        } else {
            Xe[0] = X[3 * e]; Xe[1] = X[3 * e + 1]; Xe[2] = X[3 * e + 2]; u = Z[2 * e]; v = Z[2 * e + 1];
        }
    };

    // linearise at the table S.q / S.t: residuals -> R, per-wave sums -> S.part (then a barrier)
    auto linearise = [&]() __attribute__((always_inline)) {
        double acc[FV];
#pragma unroll
        for (int k = 0; k < FV; ++k) acc[k] = 0.0;
        const double delta = S.delta;
        for (int e = tid; e < O; e += FT) {
            double r0, r1, J[12], Xe[3], u, v;
            edge_in(e, Xe, u, v);
            po_edge(S.q, S.t, Xe, u, v, S.K, r0, r1, J, true);
            R[2 * e] = r0;
            R[2 * e + 1] = r1;
            po_accumulate(r0, r1, J, delta, acc);
        }
        STAMP(24);
        po_rows_to_parts(acc, S, tid);
        STAMP(25);
        lds_barrier();
        STAMP(26);
    };
    // wave 0: the four waves' parts -> S.sum (lane k < FV)
    auto finish_sums = [&]() __attribute__((always_inline)) {
        if (lane < FV) S.sum[lane] = ((S.part[0][lane] + S.part[1][lane]) + S.part[2][lane]) + S.part[3][lane];
        wave_sync();
    };
    auto load_system = [&]() __attribute__((always_inline)) {   // lane 0: S.sum -> H (full symmetric), b
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) { S.H[6 * a + c] = S.sum[k]; S.H[6 * c + a] = S.sum[k]; ++k; }
        for (int a = 0; a < 6; ++a) S.b[a] = S.sum[21 + a];
    };
    // wave 0: (H + lambda D) dx = b, then the candidate pose and its table
    auto solve_step = [&]() __attribute__((always_inline)) {
        double x[6];
        const double lam = S.lam;
        STAMP(30);
        po_ldlt6_lds(S.H, S.b, lam, prm.strategy, S.xs, x);
        STAMP(31);
        double cand[12], q[4], t[3];
        po_pose_add_wave(x, S.pose, S.qp, cand, q, t, lane);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 6; ++j) S.dx[j] = x[j];
#pragma unroll
            for (int i = 0; i < 12; ++i) S.cand[i] = cand[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) S.q[i] = q[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) S.t[i] = t[i];
        }
    };

    for (int round = 0; round < 4; ++round) {
        if (tid < 12) S.pose[tid] = pose_in[12 * (size_t)f + tid];   // setEstimate(current_frame_->Pose()) :201
        lds_barrier();
        if (O > 0) {   // Problem::solve returns false with no edge (problem.cpp:157-161)
            if (tid == 0) {
                double q[4], t[3];
                po_table_regs(S.pose, q, t);
                for (int i = 0; i < 4; ++i) { S.q[i] = q[i]; S.qp[i] = q[i]; }
                for (int i = 0; i < 3; ++i) S.t[i] = t[i];
            }
            lds_barrier();
            linearise();
            if (wave == 0) {
                finish_sums();
                if (lane == 0) {
                    load_system();
                    // computeLambdaInitLM (problem.cpp:470-504)
                    S.ni = 2.0;
                    S.chi = 0.5 * S.sum[27];
                    if (prm.strategy == 0) {
                        if (prm.lambda_given) {
                            S.lam = prm.lambda_init;
                        } else {
                            double m = 0.0;
                            for (int i = 0; i < 6; ++i) m = fmax(fabs(S.H[7 * i]), m);
                            S.lam = prm.tau * fmin(prm.lambda_cap, m);
                        }
                    } else {
                        S.lam = 1e-5;
                    }
                    S.last = 1e20;
                    S.iter = 0;
                    S.fc = 0;
                    S.cont = prm.max_iters > 0;
                }
                wave_sync();
                if (S.cont) solve_step();
            }
            lds_barrier();
            while (S.cont) {
                linearise();   // isGoodStepInLM's residuals (:524) and, if accepted, buildHessian's
                if (wave == 0) {
                    finish_sums();
                    if (lane == 0) {
                        // the controller's words into registers first (one batch of LDS loads), the
                        // isGoodStepInLM arithmetic on them, the words back at the end
                        const double tchi = 0.5 * S.sum[27];
                        double lam = S.lam, ni = S.ni, chi = S.chi, last = S.last;
                        int iter = S.iter, fc = S.fc;
                        double dx[6], bv[6], hd[6];
                        for (int i = 0; i < 6; ++i) { dx[i] = S.dx[i]; bv[i] = S.b[i]; hd[i] = S.H[7 * i]; }
                        double scale = 0.0;
                        for (int i = 0; i < 6; ++i)
                            scale += (prm.strategy == 0) ? dx[i] * (lam * dx[i] + bv[i])
                                                         : dx[i] * (lam * hd[i] * dx[i] + bv[i]);
                        scale = 0.5 * scale;
                        scale += 1e-10;
                        const double rho = (chi - tchi) / scale;
                        const bool ok = rho > 0 && isfinite(tchi);
                        if (prm.strategy == 0) {
                            if (ok) {
                                const double m = 2 * rho - 1;
                                double alpha = 1.0 - m * m * m;
                                alpha = fmin(alpha, 2.0 / 3.0);
                                lam *= fmax(1.0 / 3.0, alpha);
                                ni = 2;
                                chi = tchi;
                            } else {
                                lam *= ni;
                                ni *= 2;
                            }
                        } else {
                            if (ok) { lam = fmax(lam / 9.0, 1e-7); chi = tchi; }
                            else lam = fmin(lam * 11.0, 1e7);
                        }
                        bool inner_end;
                        if (ok) {
                            for (int i = 0; i < 12; ++i) S.pose[i] = S.cand[i];
                            for (int i = 0; i < 4; ++i) S.qp[i] = S.q[i];   // the candidate's table is SE3(pose)'s
                            load_system();
                            inner_end = true;
                        } else {
                            fc += 1;                           // rollbackStates: S.pose untouched
                            inner_end = fc >= prm.max_trials;
                        }
                        int cont = 1;
                        if (inner_end) {
                            iter += 1;
                            if (last - chi < prm.stop_dchi2 || iter >= prm.max_iters) cont = 0;
                            last = chi;
                            fc = 0;
                        }
                        S.lam = lam; S.ni = ni; S.chi = chi; S.last = last; S.iter = iter; S.fc = fc;
                        S.cont = cont;
                    }
                    wave_sync();
                    STAMP(27);
                    if (S.cont) solve_step();
                    STAMP(28);
                }
                lds_barrier();
                STAMP(29);
            }
            its += S.iter;
        }
        // outlier flags (frontend_lego.cpp:205-226); residual_ is "as last evaluated" except for the
        // features already flagged, which are recomputed at the final estimate
        if (tid == 0) {
            double q[4], t[3];
            po_table_regs(S.pose, q, t);
            for (int i = 0; i < 4; ++i) S.q[i] = q[i];
            for (int i = 0; i < 3; ++i) S.t[i] = t[i];
        }
        lds_barrier();
        const double delta = S.delta;
        for (int e = tid; e < O; e += FT) {
            double r0 = R[2 * e], r1 = R[2 * e + 1];
            if (flag[e]) {
                double J[12], Xe[3], u, v;
                edge_in(e, Xe, u, v);
                po_edge(S.q, S.t, Xe, u, v, S.K, r0, r1, J, false);
                R[2 * e] = r0;
                R[2 * e + 1] = r1;
            }
            const double rc = po_rho0(r0, r1, delta);
            flag[e] = rc > 5.991;                       // chi2_th (frontend_lego.cpp:171)
            if (round == 3 && rchi2_out) rchi2_out[o0 + e] = rc;
        }
        lds_barrier();
        if (round == 2 && tid == 0) S.delta = 0.0;     // setCostFunction(nullptr) (:223-225)
        lds_barrier();
    }
    STAMP_FLUSH(24, 8);
    if (tid < 12) pose_out[12 * (size_t)f + tid] = S.pose[tid];
    // inliers: features.size() - cnt_outlier (:249)
    int cnt = 0;
    for (int e = tid; e < O; e += FT) cnt += flag[e] ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    __shared__ int s_cnt[FT / 64];
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    lds_barrier();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < FT / 64; ++w) c += s_cnt[w];
        if (inliers_out) inliers_out[f] = O - c;
        if (iters_out) iters_out[f] = its;
    }
}

extern "C" {

hipError_t lh_launch_frames(hipStream_t st, int n_frames, const int64_t* obs_ptr, const double* pose_in,
                            const double* pts, const double* uv, const uint8_t* flag_in, lh_params prm, double* res,
                            double* pose_out, uint8_t* flag_out, double* rchi2_out, int32_t* iters_out,
                            int32_t* inliers_out) {
    if (n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_frames, dim3(n_frames), dim3(FT), 0, st, obs_ptr, pose_in, pts, uv, flag_in, prm, res, pose_out,
                       flag_out, rchi2_out, iters_out, inliers_out);
    return hipGetLastError();
}

}  // extern "C"
