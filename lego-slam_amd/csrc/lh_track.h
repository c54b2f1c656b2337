// lh_track.h — one frame of Frontend::Track on the device (lh_track_frame, include/lego_ba.h): the
// arguments of k_track_guess and k_track_pack, shared with the host side, and the guess arithmetic
// (Camera::world2pixel, src/camera.cpp:8-29, as TrackLastFrameLKOpticalFlowOpenCV calls it, frontend_lego.cpp:383-398).
//
// The arithmetic is plain fp64 C++ on one feature's own data, written once for the kernel (lh_track.hip) and for any
// host compiler (tests/track_probe.cpp runs the very same operations).  Contraction is off in this file: a product
// and a sum stay two roundings wherever they are inlined.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LH_TRACK_FN __host__ __device__ inline
#else
#define LH_TRACK_FN inline
#endif

struct lh_track_args {
    int32_t n_points;
    const float* kp1;           // [n_points][2]
    const double* pts_w;        // [n_points][3]; read only where has_point
    const uint8_t* has_point;   // [n_points] or null: every feature has a point
    double pose[12];            // the predicted T_cw, row-major [R|t]
    double ext[12];             // the camera's extrinsic, row-major [R|t]
    double K[4];                // fx, fy, cx, cy
    float* kp2;                 // [n_points][2] k_track_guess: the tracker's guesses; k_track_pack: its result
    const uint8_t* success;     // [n_points] the tracker's (k_track_pack)
    // k_track_pack's outputs: k_frames' inputs for the one frame, and what the host scatters its outputs with
    int64_t* obs_ptr;           // [2] {0, n_edges}
    double* pts;                // [n_edges][3]
    double* uv;                 // [n_edges][2] kp2 widened (toVec2)
    int32_t* edge_feature;      // [n_edges] the feature of each edge, ascending
    int32_t* counts;            // [2] n_tracked, n_edges
};

#ifdef LH_TRACK_IMPL   // the arithmetic: lh_track.hip and the CPU probe define it; the host side needs the struct alone
#pragma clang fp contract(off)

// y = [R|t] x, each row ((m0 x0 + m1 x1) + m2 x2) + m3
LH_TRACK_FN void lh_track_rigid(const double* m, const double* x, double* y) {
    for (int r = 0; r < 3; ++r) y[r] = ((m[4 * r] * x[0] + m[4 * r + 1] * x[1]) + m[4 * r + 2] * x[2]) + m[4 * r + 3];
}

// The pixel of world point X in the camera with extrinsic E and intrinsics K of a body at pose T (world2camera then
// camera2pixel, camera.cpp:8-19), as floats (round to nearest even; past FLT_MAX: +-inf).  The reference forms E * T
// first; this is E (T X).
LH_TRACK_FN void lh_track_guess(const double* T, const double* E, const double* K, const double* X, float* gu, float* gv) {
    double Pb[3], Pc[3];
    lh_track_rigid(T, X, Pb);
    lh_track_rigid(E, Pb, Pc);
    const double u = (K[0] * Pc[0]) / Pc[2] + K[2];
    const double v = (K[1] * Pc[1]) / Pc[2] + K[3];
    *gu = (float)u;
    *gv = (float)v;
}
#endif  // LH_TRACK_IMPL
