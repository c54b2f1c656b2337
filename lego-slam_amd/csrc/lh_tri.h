// lh_tri.h — batched SVD triangulation (legoslam::triangulation, include/legoslam/algorithm.h:11-34):
// k_triangulate's arguments, shared with the host side, and the per-point arithmetic.
//
// The arithmetic is plain fp64 C++ on one point's own data, written once for the kernel (lh_tri.hip)
// and for any host compiler (a CPU probe can run the very same operations).  Contraction is off in
// this file: a product and a sum stay two roundings wherever they are inlined, so a point's bits do
// not depend on the code around it (its batch position, the view layout, the stereo entry point).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LH_TRI_FN __host__ __device__ inline
#else
#define LH_TRI_FN inline
#endif

// lh_tri_result.flags
#define LH_TRI_F_NONFINITE 1   // a component of pt is NaN or infinite           algorithm.h:26-28
#define LH_TRI_F_RATIO 2       // !(sigma3 / sigma2 < sing_ratio_thr)            algorithm.h:30-33
#define LH_TRI_F_Y 4           // gate: !(pt[1] <= y_max)                        frontend_lego.cpp:134
#define LH_TRI_F_Z 8           // gate: !(pt[2] > z_min && pt[2] <= z_max)       frontend_lego.cpp:135
#define LH_TRI_F_TRACK 16      // lh_stereo_landmarks: the LK track failed, nothing triangulated
#define LH_TRI_F_HAS_POINT 32  // lh_insert_keyframe: the feature has a map point already, nothing triangulated (k_kf_finish)

#define LH_TRI_SWEEPS 16       // cap of the Jacobi sweeps (noisy stereo input settles in ~5)

struct lh_tri_args {
    int32_t n_points, n_poses;
    const double* pose;         // [n_poses][12]
    const double* cam_K;        // [n_poses][4] or null
    const int64_t* view_ptr;    // [n_points + 1] or null: n_poses views per point, view v on pose v
    const uint32_t* view_pose;  // [n_views] (with view_ptr)
    const double* view_xy;      // [n_views][2], or null: the stereo pair below
    const float* kp1;           // [n_points][2] view 0 (pose 0) and
    const float* kp2;           //               view 1 (pose 1) of every point, floats widened (toVec2)
    const uint8_t* success;     // [n_points] LK success: 0 = flag LH_TRI_F_TRACK, not triangulated
    double thr;
    int32_t gate, has_T;
    double y_max, z_min, z_max;
    double T[12];
    double* pt;                 // [n_points][3]
    uint8_t* flags;             // [n_points]
    double* ratio;              // [n_points] or null
};

#ifdef LH_TRI_IMPL   // the arithmetic: lh_tri.hip (and a CPU probe) define it; the host side needs the struct alone
#pragma clang fp contract(off)

// Rotate the new row r into row K of the upper-triangular R (Givens): zeroes r[K].
template <int K>
LH_TRI_FN void lh_tri_givens(double (&R)[4][4], double (&r)[4]) {
    const double b = r[K];
    if (b != 0.0) {
        const double a = R[K][K];
        const double h = sqrt(a * a + b * b);
        const double c = a / h, s = b / h;
#pragma unroll
        for (int j = K; j < 4; ++j) {
            const double t = c * R[K][j] + s * r[j];
            r[j] = c * r[j] - s * R[K][j];
            R[K][j] = t;
        }
    }
}

// One view's two rows of A (algorithm.h:18-22), streamed into R.  m: the view's 3x4 [R|t], row-major.
LH_TRI_FN void lh_tri_add_view(double (&R)[4][4], const double* m, double x, double y) {
    double r0[4], r1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r0[j] = x * m[8 + j] - m[j];
        r1[j] = y * m[8 + j] - m[4 + j];
    }
    lh_tri_givens<0>(R, r0); lh_tri_givens<1>(R, r0); lh_tri_givens<2>(R, r0); lh_tri_givens<3>(R, r0);
    lh_tri_givens<0>(R, r1); lh_tri_givens<1>(R, r1); lh_tri_givens<2>(R, r1); lh_tri_givens<3>(R, r1);
}

// Camera::pixel2camera at depth 1 (camera.cpp:21-25): (u - cx) / fx, (v - cy) / fy
LH_TRI_FN void lh_tri_normalise(const double* K, double& x, double& y) {
    x = (x - K[2]) / K[0];
    y = (y - K[3]) / K[1];
}

// One-sided (Hestenes) Jacobi rotation of columns P, Q of U, accumulated into V.  Converged when
// |g| <= tol sqrt(a b) (tol = sqrt(4) eps, as LAPACK's dgesvj takes it for 4 rows) or a b == 0: the test
// never divides by a column norm, which an exact correspondence leaves at ~1e-16 of the largest.
template <int P, int Q>
LH_TRI_FN bool lh_tri_rotate(double (&U)[4][4], double (&V)[4][4]) {
    double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a += U[i][P] * U[i][P];
        b += U[i][Q] * U[i][Q];
        g += U[i][P] * U[i][Q];
    }
    const double ab = a * b;
    if (ab == 0.0 || fabs(g) <= 2.0 * 2.220446049250313e-16 * sqrt(ab)) return false;
    const double zeta = (b - a) / (2.0 * g);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double up = U[i][P], uq = U[i][Q];
        U[i][P] = c * up - s * uq;
        U[i][Q] = s * up + c * uq;
        const double vp = V[i][P], vq = V[i][Q];
        V[i][P] = c * vp - s * vq;
        V[i][Q] = s * vp + c * vq;
    }
    return true;
}

// SVD of the triangular factor: v = the right singular vector of the smallest singular value, as
// pt = v[0..2] / v[3], and ratio = sigma3 / sigma2.  A^T A is never formed (sigma3 / sigma2 is compared with
// 1e-3; the eigenvalue route loses sigma3 below ~1e-8 sigma0).
LH_TRI_FN void lh_tri_svd(double (&U)[4][4], double pt[3], double& ratio) {
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < LH_TRI_SWEEPS; ++sweep) {
        bool rot = lh_tri_rotate<0, 1>(U, V);
        rot |= lh_tri_rotate<0, 2>(U, V);
        rot |= lh_tri_rotate<0, 3>(U, V);
        rot |= lh_tri_rotate<1, 2>(U, V);
        rot |= lh_tri_rotate<1, 3>(U, V);
        rot |= lh_tri_rotate<2, 3>(U, V);
        if (!rot) break;
    }
    double n[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) n[j] = U[0][j] * U[0][j] + U[1][j] * U[1][j] + U[2][j] * U[2][j] + U[3][j] * U[3][j];
    // the two smallest squared norms, and the column of V of the smallest
    double m1 = n[0], m2 = INFINITY;
    double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (n[j] < m1) {
            m2 = m1;
            m1 = n[j];
            v0 = V[0][j]; v1 = V[1][j]; v2 = V[2][j]; v3 = V[3][j];
        } else if (n[j] < m2) {
            m2 = n[j];
        }
    }
    pt[0] = v0 / v3;
    pt[1] = v1 / v3;
    pt[2] = v2 / v3;
    ratio = sqrt(m1) / sqrt(m2);
    // sigma2 <= 4 eps sigma0: A has two null directions to working precision (two identical views), and both
    // small singular values are rounding noise whose quotient means nothing (the reference's is then an arbitrary
    // number, usually of order 1).  The ratio is NaN, which fails the threshold test.
    const double mx = fmax(fmax(n[0], n[1]), fmax(n[2], n[3]));
    if (m2 <= (4.0 * 2.220446049250313e-16) * (4.0 * 2.220446049250313e-16) * mx) ratio = NAN;
    const double nsum = (n[0] + n[1]) + (n[2] + n[3]);
    if (nsum != nsum) ratio = nsum;   // a NaN norm compares false above: the ratio is NaN, as the reference's
}

// The reference's tests in its order (algorithm.h:26-33), the caller's gate in the rig frame
// (frontend_lego.cpp:133-136), then T_out on an accepted point (:138).
LH_TRI_FN uint8_t lh_tri_classify(const lh_tri_args& a, double pt[3], double ratio) {
    uint8_t f = 0;
    if (!(isfinite(pt[0]) && isfinite(pt[1]) && isfinite(pt[2]))) f |= LH_TRI_F_NONFINITE;
    if (!(ratio < a.thr)) f |= LH_TRI_F_RATIO;
    if (a.gate) {
        if (!(pt[1] <= a.y_max)) f |= LH_TRI_F_Y;
        if (!(pt[2] > a.z_min && pt[2] <= a.z_max)) f |= LH_TRI_F_Z;
    }
    if (a.has_T && f == 0) {
        const double x = pt[0], y = pt[1], z = pt[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) pt[i] = ((a.T[4 * i] * x + a.T[4 * i + 1] * y) + a.T[4 * i + 2] * z) + a.T[4 * i + 3];
    }
    return f;
}

// Point i of the batch, start to finish.
LH_TRI_FN void lh_tri_point(const lh_tri_args& a, int64_t i) {
    double R[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) R[r][c] = 0.0;
    if (!a.view_xy) {   // the stereo pair: tracked keypoints, still on the device
        if (!a.success[i]) {
            a.pt[3 * i] = a.pt[3 * i + 1] = a.pt[3 * i + 2] = 0.0;
            a.flags[i] = LH_TRI_F_TRACK;
            if (a.ratio) a.ratio[i] = 0.0;
            return;
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const float* kp = v ? a.kp2 : a.kp1;
            double x = (double)kp[2 * i], y = (double)kp[2 * i + 1];
            if (a.cam_K) lh_tri_normalise(a.cam_K + 4 * v, x, y);
            lh_tri_add_view(R, a.pose + 12 * v, x, y);
        }
    } else {
        const int64_t beg = a.view_ptr ? a.view_ptr[i] : i * a.n_poses;
        const int64_t end = a.view_ptr ? a.view_ptr[i + 1] : beg + a.n_poses;
        for (int64_t v = beg; v < end; ++v) {
            const int64_t p = a.view_ptr ? (int64_t)a.view_pose[v] : v - beg;
            double x = a.view_xy[2 * v], y = a.view_xy[2 * v + 1];
            if (a.cam_K) lh_tri_normalise(a.cam_K + 4 * p, x, y);
            lh_tri_add_view(R, a.pose + 12 * p, x, y);
        }
    }
    double pt[3], ratio;
    lh_tri_svd(R, pt, ratio);
    const uint8_t f = lh_tri_classify(a, pt, ratio);
    a.pt[3 * i] = pt[0];
    a.pt[3 * i + 1] = pt[1];
    a.pt[3 * i + 2] = pt[2];
    a.flags[i] = f;
    if (a.ratio) a.ratio[i] = ratio;
}
#endif  // LH_TRI_IMPL
