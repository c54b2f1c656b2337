// lh_edge.h — the Eigen / Sophus mirror and the per-edge path (residual, robust weight, Jacobians, the edge's
// blocks) of k_lin (lh_lin.hip) and k_frames (lh_frames.hip).
#pragma once
#include "lh_common.h"
#include "lh_dev.h"

// ============================================================================
// Eigen / Sophus arithmetic and the per-edge path, in the reference's
// expression order with contraction off.  This is a bitwise mirror of the
// oracle's restatement (oracle/lego_oracle.c): the Huber gate
// (base_edge.cpp:55) tests the sign of a rounding residue, so the residual
// must be computed exactly as the reference computes it.
// ============================================================================
#pragma clang fp contract(off)

// Eigen Quaternion(Matrix3): q = {w, x, y, z}, R row-major
__device__ __forceinline__ void d_q_from_R(const double* R, double q[4]) {
    double t = R[0] + R[4] + R[8];
    double w, x, y, z;     // scalars, not an indexed array: keeps the pose code out of scratch
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        x = (R[7] - R[5]) * t;
        y = (R[2] - R[6]) * t;
        z = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        // Eigen's c[i], c[j], c[k] with j = (i+1)%3, k = (j+1)%3, written out per case
        if (i == 0) {
            t = sqrt(R[0] - R[4] - R[8] + 1.0);
            x = 0.5 * t; t = 0.5 / t;
            w = (R[7] - R[5]) * t;
            y = (R[3] + R[1]) * t;
            z = (R[6] + R[2]) * t;
        } else if (i == 1) {
            t = sqrt(R[4] - R[8] - R[0] + 1.0);
            y = 0.5 * t; t = 0.5 / t;
            w = (R[2] - R[6]) * t;
            z = (R[7] + R[5]) * t;
            x = (R[1] + R[3]) * t;
        } else {
            t = sqrt(R[8] - R[0] - R[4] + 1.0);
            z = 0.5 * t; t = 0.5 / t;
            w = (R[3] - R[1]) * t;
            x = (R[2] + R[6]) * t;
            y = (R[5] + R[7]) * t;
        }
    }
    q[0] = w; q[1] = x; q[2] = y; q[3] = z;
}

// Eigen QuaternionBase::toRotationMatrix
__device__ __forceinline__ void d_R_from_q(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;          R[2] = txz + twy;
    R[3] = txy + twz;          R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;          R[7] = tyz + twx;          R[8] = 1.0 - (txx + tyy);
}

__device__ __forceinline__ void d_cross(const double a[3], const double b[3], double c[3]) {
    const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
    c[0] = c0; c[1] = c1; c[2] = c2;
}

// Eigen QuaternionBase::_transformVector (Sophus SO3 * point)
__device__ __forceinline__ void d_q_rotate(const double* q, const double v[3], double o[3]) {
    double uv[3], uv2[3];
    d_cross(q + 1, v, uv);
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    d_cross(q + 1, uv, uv2);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = v[i] + q[0] * uv[i] + uv2[i];
}

// Eigen quaternion product + Sophus SO3Base::operator*= renormalisation
__device__ __forceinline__ void d_q_mul(const double* a, const double* b, double o[4]) {
    double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    double y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    double z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
    const double sq = w * w + x * x + y * y + z * z;
    if (sq != 1.0) {
        const double sc = 2.0 / (1.0 + sq);
        w *= sc; x *= sc; y *= sc; z *= sc;
    }
    o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}

// rotation angle of a twist (upsilon, omega): theta = |omega|
__device__ __forceinline__ double d_twist_theta(const double a[6]) {
    return sqrt(a[3] * a[3] + a[4] * a[4] + a[5] * a[5]);
}

// Sophus SE3::exp, twist (upsilon, omega) -> (q, t)   (Sophus 1.0 se3.hpp), with the
// transcendentals given: sh, ch = sin, cos(theta / 2) and st, ct = sin, cos(theta)
__device__ __forceinline__ void d_se3_exp_trig(const double a[6], double sh, double ch, double st, double ct, double q[4],
                                      double t[3]) {
    const double eps = 1e-10;
    const double* w = a + 3;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    double im, re;
    if (th < eps) {
        const double th4 = th2 * th2;
        im = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4;
        re = 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th4;
    } else {
        im = sh / th;
        re = ch;
    }
    q[0] = re; q[1] = im * w[0]; q[2] = im * w[1]; q[3] = im * w[2];
    double V[9];
    if (th < eps) {
        d_R_from_q(q, V);
    } else {
        const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        double Om2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
        const double c1 = (1.0 - ct) / th2;
        const double c2 = (th - st) / (th2 * th);
        for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + c1 * Om[i] + c2 * Om2[i];
    }
    for (int i = 0; i < 3; ++i) t[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2];
}


// estimate_ (row-major [R|t]) -> pose table entry for camera extrinsic e (LH_EXT layout)
__device__ inline void d_pose_table(const double* T12, const double* __restrict__ e, double* pt) {
    const double R[9] = {T12[0], T12[1], T12[2], T12[4], T12[5], T12[6], T12[8], T12[9], T12[10]};
    double q[4];
    d_q_from_R(R, q);                                   // SE3(estimate_)
    const double t[3] = {T12[3], T12[7], T12[11]};
    for (int i = 0; i < 4; ++i) pt[LH_PT_QT + i] = q[i];
    for (int i = 0; i < 3; ++i) pt[LH_PT_TT + i] = t[i];
    double qet[4], rt[3];
    d_q_mul(e, q, qet);                                 // _cam_ext * T
    d_q_rotate(e, t, rt);
    for (int i = 0; i < 4; ++i) pt[LH_PT_QET + i] = qet[i];
    for (int i = 0; i < 3; ++i) pt[LH_PT_TET + i] = e[4 + i] + rt[i];
    double Rt[9];
    d_R_from_q(q, Rt);                                  // T.rotationMatrix()
    for (int i = 0; i < 9; ++i) pt[LH_PT_RT + i] = Rt[i];
    pt[23] = 0.0;
}

// VertexPose::add (lego_types.h, problem.cpp:433-455): estimate_ = (SE3::exp(dx) * SE3(estimate_)).matrix(),
// the candidate [R|t] (row-major, 12) from the committed one Tc and the pose step dx (translation-first
// twist; a non-finite step is skipped, as VertexPose::add's guard does).
__device__ __forceinline__ void d_pose_candidate(const double (&Tc)[12], const double* dx, double (&To)[12]) {
    double up[6];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 6; ++a) { up[a] = dx[a]; bad |= !isfinite(up[a]); }
    if (bad) {
#pragma unroll
        for (int a = 0; a < 6; ++a) up[a] = 0.0;
    }
    const double th = d_twist_theta(up);
    double sh, ch, st, ct;
    sincos(0.5 * th, &sh, &ch);
    sincos(th, &st, &ct);
    double qe[4], te[3], qT[4], qn[4], tr[3], Rn[9];
    d_se3_exp_trig(up, sh, ch, st, ct, qe, te);
    const double Rc[9] = {Tc[0], Tc[1], Tc[2], Tc[4], Tc[5], Tc[6], Tc[8], Tc[9], Tc[10]};
    d_q_from_R(Rc, qT);
    const double tc[3] = {Tc[3], Tc[7], Tc[11]};
    d_q_mul(qe, qT, qn);
    d_q_rotate(qe, tc, tr);
    d_R_from_q(qn, Rn);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        To[4 * i] = Rn[3 * i]; To[4 * i + 1] = Rn[3 * i + 1]; To[4 * i + 2] = Rn[3 * i + 2];
        To[4 * i + 3] = te[i] + tr[i];
    }
}

struct EdgeEval {
    double r0, r1, e2, rho0, rho1, rho2;
    double W00, W01, W10, W11;
    double Jp[12];   // 2 x 6, translation-first twist (lego_types.h:246-248)
    double Jl[6];    // 2 x 3
};

// the camera point ext (T X) of computeResidual (lego_types.h:213).  An extrinsic rotation that is
// exactly the identity is skipped: the quaternion rotation by (1, 0, 0, 0) returns its input exactly.
__device__ __forceinline__ void edge_pc(const double* __restrict__ pt, const double* __restrict__ e, bool ext_id,
                                        bool ext_rot, const double X[3], double Pc[3]) {
    double Pb[3];
    d_q_rotate(pt + LH_PT_QT, X, Pb);
#pragma unroll
    for (int i = 0; i < 3; ++i) Pb[i] = Pb[i] + pt[LH_PT_TT + i];
    if (ext_id) {
#pragma unroll
        for (int i = 0; i < 3; ++i) Pc[i] = Pb[i];       // identity quaternion and zero t: exact
    } else if (ext_rot) {
#pragma unroll
        for (int i = 0; i < 3; ++i) Pc[i] = Pb[i] + e[4 + i];
    } else {
        d_q_rotate(e, Pb, Pc);
#pragma unroll
        for (int i = 0; i < 3; ++i) Pc[i] = Pc[i] + e[4 + i];
    }
}

// residual_ = z - pi(K Pc), pi(q) = q / (q_z + 1e-18)   (lego_types.h:200-216), from the camera point
__device__ __forceinline__ void edge_res_pc(const double Pc[3], double u, double v, const lh_params& prm, double& r0,
                                            double& r1) {
    const double fx = prm.K[0], fy = prm.K[1], cx = prm.K[2], cy = prm.K[3];
    double p0 = fx * Pc[0] + cx * Pc[2];                  // + 0 * Pc[1]: exact
    double p1 = fy * Pc[1] + cy * Pc[2];
    const double den = Pc[2] + 1e-18;
    p0 /= den;
    p1 /= den;
    r0 = u - p0;
    r1 = v - p1;
}
// the whole residual, Pc = ext (T X) returned
__device__ __forceinline__ void edge_residual(const double* __restrict__ pt, const double* __restrict__ e, bool ext_id,
                                              bool ext_rot, const double X[3], double u, double v, const lh_params& prm,
                                              double& r0, double& r1, double Pc[3]) {
    edge_pc(pt, e, ext_id, ext_rot, X, Pc);
    edge_res_pc(Pc, u, v, prm, r0, r1);
}

// HuberCost::compute (cost_function.cpp:5-17) + computeRobustInformation (base_edge.cpp:44-64)
__device__ __forceinline__ void edge_robust(EdgeEval& E, const lh_params& prm) {
    E.e2 = E.r0 * E.r0 + E.r1 * E.r1;
    const double delta = prm.huber_delta;
    if (delta > 0.0) {
        const double d2 = delta * delta;
        if (E.e2 <= d2) {
            E.rho0 = E.e2; E.rho1 = 1.0; E.rho2 = 0.0;
        } else {
            const double s = sqrt(E.e2);
            E.rho0 = 2 * s * delta - d2;
            E.rho1 = delta / s;
            E.rho2 = -0.5 * E.rho1 / E.e2;
        }
        E.W00 = E.rho1; E.W01 = 0.0; E.W10 = 0.0; E.W11 = E.rho1;
        // gate_mode 1 (diagnostic): the analytically-zero residue of an outlier edge counts as 0
        if (E.rho1 + 2 * E.rho2 * E.e2 > 0.0 && !(prm.gate_mode == 1 && E.e2 > d2)) {
            const double s2 = 2 * E.rho2;
            E.W00 += s2 * E.r0 * E.r0;
            E.W01 += s2 * E.r0 * E.r1;
            E.W10 += s2 * E.r1 * E.r0;
            E.W11 += s2 * E.r1 * E.r1;
        }
    } else {
        E.rho0 = E.e2; E.rho1 = 1.0; E.rho2 = 0.0;
        E.W00 = 1.0; E.W01 = 0.0; E.W10 = 0.0; E.W11 = 1.0;
    }
}

#pragma clang fp contract(fast)

// EdgeProjection::computeJacobians (lego_types.h:218-254).  The reference evaluates them at
// ((ext T) X) and the residual at (ext (T X)); here both use the residual's point, which differs
// in rounding only (the Jacobians are not on the bitwise-mirrored path, and the back substitution
// re-derives exactly the Jacobians its linearisation used).  j_i's structural zeros J(0,1) and
// J(1,0) (lego_types.h:247-248) are left out of every product (lin_blocks); Jp[1], Jp[6] unset.
__device__ __forceinline__ void edge_jac_pc(const double Pc[3], const double* __restrict__ Rt,
                                            const double* __restrict__ e, bool ext_rot, const lh_params& prm,
                                            double Jp[12], double Jl[6]) {
    const double fx = prm.K[0], fy = prm.K[1];
    const double x = Pc[0], y = Pc[1], z = Pc[2];
    const double zi = fast_rcp(z + 1e-18);
    const double zi2 = zi * zi;
    Jp[0] = -fx * zi;              Jp[1] = 0.0;                  Jp[2] = fx * x * zi2;
    Jp[3] = fx * x * y * zi2;      Jp[4] = -fx - fx * x * x * zi2; Jp[5] = fx * y * zi;
    Jp[6] = 0.0;                   Jp[7] = -fy * zi;             Jp[8] = fy * y * zi2;
    Jp[9] = fy + fy * y * y * zi2; Jp[10] = -fy * x * y * zi2;   Jp[11] = -fy * x * zi;
    // j_j = (j_i(:, 0:3) * ext.rotationMatrix()) * T.rotationMatrix()
    double A[6];
    if (ext_rot) {   // J * I: exact
        A[0] = Jp[0]; A[1] = 0.0; A[2] = Jp[2]; A[3] = 0.0; A[4] = Jp[7]; A[5] = Jp[8];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Jl[j] = A[0] * Rt[j] + A[2] * Rt[6 + j];
            Jl[3 + j] = A[4] * Rt[3 + j] + A[5] * Rt[6 + j];
        }
    } else {
        const double* Re = e + 7;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            A[j] = Jp[0] * Re[j] + Jp[2] * Re[6 + j];
            A[3 + j] = Jp[7] * Re[3 + j] + Jp[8] * Re[6 + j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Jl[3 * i + j] = A[3 * i] * Rt[j] + A[3 * i + 1] * Rt[3 + j] + A[3 * i + 2] * Rt[6 + j];
    }
}

// ---- lh_options.precision = LH_PREC_FP32_RESID (BASELINE config 3's "fp32 residuals + fp64
//      accumulate"): the Jacobians (camera point, projection derivative, chain through the extrinsic and
//      the pose rotation) in float, widened to double before any product that is summed.  The residual,
//      the Huber weight, rho0, chi2, b and the gain ratio stay the fp64 mirror of the reference's
//      arithmetic: a float residual carries ~3e-5 px of rounding, which decides LM
//      steps on weakly conditioned windows.  The step is Gauss-Newton on a Jacobian
//      rounded to float: parity to tolerance (tests/test_precision.py). ----
__device__ __forceinline__ void q_rotate_f(const double* q, const float v[3], float o[3]) {
    const float w = (float)q[0], x = (float)q[1], y = (float)q[2], z = (float)q[3];
    const float u0 = 2.0f * (y * v[2] - z * v[1]), u1 = 2.0f * (z * v[0] - x * v[2]), u2 = 2.0f * (x * v[1] - y * v[0]);
    o[0] = v[0] + w * u0 + (y * u2 - z * u1);
    o[1] = v[1] + w * u1 + (z * u0 - x * u2);
    o[2] = v[2] + w * u2 + (x * u1 - y * u0);
}

// RES: residual and robust weight into E (else E's W is the caller's); JAC: Jacobians into E
template <bool RES, bool JAC>
__device__ __forceinline__ void edge_eval_f(const double* __restrict__ pt, const double* __restrict__ e, bool ext_id,
                                            bool ext_rot, const double X[3], double u, double v, const lh_params& prm,
                                            EdgeEval& E) {
    const float Xf[3] = {(float)X[0], (float)X[1], (float)X[2]};
    float Pc[3];
    q_rotate_f(pt + LH_PT_QT, Xf, Pc);
#pragma unroll
    for (int i = 0; i < 3; ++i) Pc[i] += (float)pt[LH_PT_TT + i];
    if (!ext_id) {
        if (!ext_rot) {
            const float Pb[3] = {Pc[0], Pc[1], Pc[2]};
            q_rotate_f(e, Pb, Pc);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) Pc[i] += (float)e[4 + i];
    }
    const float fx = (float)prm.K[0], fy = (float)prm.K[1];
    const float zi = 1.0f / (Pc[2] + 1e-18f);
    if (RES) {
        const float cx = (float)prm.K[2], cy = (float)prm.K[3];
        const float r0 = (float)u - (fx * Pc[0] + cx * Pc[2]) * zi, r1 = (float)v - (fy * Pc[1] + cy * Pc[2]) * zi;
        const float e2 = r0 * r0 + r1 * r1;
        float rho0 = e2, rho1 = 1.0f, rho2 = 0.0f, W00 = 1.0f, W01 = 0.0f, W11 = 1.0f;
        const float delta = (float)prm.huber_delta;
        if (prm.huber_delta > 0.0) {
            const float d2 = delta * delta;
            if (!(e2 <= d2)) {
                const float sq = sqrtf(e2);
                rho0 = 2.0f * sq * delta - d2;
                rho1 = delta / sq;
                rho2 = -0.5f * rho1 / e2;
            }
            W00 = rho1; W11 = rho1;
            if (rho1 + 2.0f * rho2 * e2 > 0.0f && !(prm.gate_mode == 1 && e2 > d2)) {
                const float s2 = 2.0f * rho2;
                W00 += s2 * r0 * r0;
                W01 = s2 * r0 * r1;
                W11 += s2 * r1 * r1;
            }
        }
        E.r0 = r0; E.r1 = r1; E.e2 = e2; E.rho0 = rho0; E.rho1 = rho1; E.rho2 = rho2;
        E.W00 = W00; E.W01 = W01; E.W10 = W01; E.W11 = W11;
    }
    if (JAC) {
        const float x = Pc[0], y = Pc[1], zi2 = zi * zi;
        float J[12];
        J[0] = -fx * zi;               J[1] = 0.0f;                   J[2] = fx * x * zi2;
        J[3] = fx * x * y * zi2;       J[4] = -fx - fx * x * x * zi2; J[5] = fx * y * zi;
        J[6] = 0.0f;                   J[7] = -fy * zi;               J[8] = fy * y * zi2;
        J[9] = fy + fy * y * y * zi2;  J[10] = -fy * x * y * zi2;    J[11] = -fy * x * zi;
        float A[6];
        if (ext_rot) {
            A[0] = J[0]; A[1] = 0.0f; A[2] = J[2]; A[3] = 0.0f; A[4] = J[7]; A[5] = J[8];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                A[j] = J[0] * (float)e[7 + j] + J[2] * (float)e[13 + j];
                A[3 + j] = J[7] * (float)e[10 + j] + J[8] * (float)e[13 + j];
            }
        }
        const double* Rt = pt + LH_PT_RT;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                E.Jl[3 * i + j] = (double)(A[3 * i] * (float)Rt[j] + A[3 * i + 1] * (float)Rt[3 + j] + A[3 * i + 2] * (float)Rt[6 + j]);
#pragma unroll
        for (int k = 0; k < 12; ++k) E.Jp[k] = (double)J[k];
    }
}

// J(r, a) of j_i (2 x 6) is structurally zero: J(0, 1), J(1, 0)
__device__ __forceinline__ constexpr bool jz(int r, int a) { return (r == 0 && a == 1) || (r == 1 && a == 0); }

// Jp(:, a) . (x0, x1) without the structural zero
__device__ __forceinline__ double jdot(const double* Jp, int a, double x0, double x1) {
    if (jz(0, a)) return Jp[6 + a] * x1;
    if (jz(1, a)) return Jp[a] * x0;
    return Jp[a] * x0 + Jp[6 + a] * x1;
}

// The per-edge blocks of the linearisation (problem.cpp:285-331): H_ll, b_l, H_pl into registers,
// H_pp (21) and b_p (6) into the lane's row of the pose-sum image.  WI: every live edge of the wave
// is an inlier, so W = I and dr = 1 exactly, and W J = J.
template <bool WI>
__device__ __forceinline__ void lin_blocks(const EdgeEval& E, bool pfixed, double dr, double (&hll)[6],
                                           double (&bl)[3], double (&hpl)[18], double* __restrict__ trow) {
    const double* Jp = E.Jp;
    const double* Jl = E.Jl;
    double WJl[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        WJl[c] = WI ? Jl[c] : E.W00 * Jl[c] + E.W01 * Jl[3 + c];
        WJl[3 + c] = WI ? Jl[3 + c] : E.W10 * Jl[c] + E.W11 * Jl[3 + c];
    }
    hll[0] = Jl[0] * WJl[0] + Jl[3] * WJl[3];
    hll[1] = Jl[0] * WJl[1] + Jl[3] * WJl[4];
    hll[2] = Jl[0] * WJl[2] + Jl[3] * WJl[5];
    hll[3] = Jl[1] * WJl[1] + Jl[4] * WJl[4];
    hll[4] = Jl[1] * WJl[2] + Jl[4] * WJl[5];
    hll[5] = Jl[2] * WJl[2] + Jl[5] * WJl[5];
    const double dr0 = WI ? E.r0 : dr * E.r0, dr1 = WI ? E.r1 : dr * E.r1;   // rho' r
#pragma unroll
    for (int c = 0; c < 3; ++c) bl[c] = -(Jl[c] * dr0 + Jl[3 + c] * dr1);
    if (pfixed) return;
    if (WI) {
        // H_pp(a, b) = sum over the rows r where neither J(r, a) nor J(r, b) is a structural zero
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) {
                const bool u0 = !jz(0, a) && !jz(0, b), u1 = !jz(1, a) && !jz(1, b);
                trow[k++] = u0 && u1 ? Jp[a] * Jp[b] + Jp[6 + a] * Jp[6 + b]
                                     : (u0 ? Jp[a] * Jp[b] : (u1 ? Jp[6 + a] * Jp[6 + b] : 0.0));
            }
    } else {
        double WJp[12];   // W J_p, column b: W (J(0, b), J(1, b)) with J's zero left out
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            WJp[b] = jz(1, b) ? E.W00 * Jp[b] : (jz(0, b) ? E.W01 * Jp[6 + b] : E.W00 * Jp[b] + E.W01 * Jp[6 + b]);
            WJp[6 + b] = jz(1, b) ? E.W10 * Jp[b] : (jz(0, b) ? E.W11 * Jp[6 + b] : E.W10 * Jp[b] + E.W11 * Jp[6 + b]);
        }
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) trow[k++] = jdot(Jp, a, WJp[b], WJp[6 + b]);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hpl[3 * a + c] = jdot(Jp, a, WJl[c], WJl[3 + c]);
        trow[21 + a] = -jdot(Jp, a, dr0, dr1);
    }
}
