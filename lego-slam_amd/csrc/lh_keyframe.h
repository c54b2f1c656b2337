// lh_keyframe.h — a keyframe's half of the frame on the device (lh_insert_keyframe, include/lego_ba.h):
// the arguments of k_kf_assemble and k_kf_finish, shared with the host side.  The arithmetic is other files': the
// detector's (lh_gftt.h), the guess (lh_track.h), the tracker's (lh_klt.h) and the triangulation's (lh_tri.h).
//
// The feature list has a capacity known on the host, n_have + max_corners, and a length known on the device alone until
// the call's one download: n = n_have + m, m = min(ctl->n_acc, max_corners).  Every buffer below holds the capacity,
// every launch is sized for it, and a slot at or past n is given NaN keypoints, which the tracker answers with
// success 0 before it reads an image (lh_klt.h: the range test fails at every level).
#pragma once
#include <stdint.h>

#include "lh_gftt.h"

#define LH_KF_MAX_FEATURES (1 << 24)   // n_have + max_corners at most: twice a slot's index stays far inside int32

// lh_kf_args.state: one byte per slot
#define LH_KF_S_UNUSED 0      // at or past n
#define LH_KF_S_NEW 1         // no map point yet: triangulated if it tracks
#define LH_KF_S_HAS_POINT 2   // carries a map point: tracked, not triangulated

struct lh_kf_args {
    int32_t n_have, max_corners;
    const lh_gftt_ctl* ctl;     // the detector's counts, final once k_gftt_rank has run
    const double* pts_w;        // [n_have][3]; read only where has_point
    const uint8_t* has_point;   // [n_have] or null: every feature of have_kp has a point
    double pose[12];            // the frame's T_cw, row-major [R|t]
    double ext[12];             // the right camera's extrinsic
    double K[4];                // and its intrinsics
    float* kl;                  // [capacity][2] in: have_kp, then the corners as k_gftt_rank wrote them; out: NaN past n
    float* kp_right;            // [capacity][2] k_kf_assemble: the tracker's guesses; then its result
    uint8_t* state;             // [capacity] LH_KF_S_*
    float* kp_new;              // [max_corners][2] the corners again, for the download
    // k_kf_finish, behind the tracker and k_triangulate
    const uint8_t* success;     // [capacity]
    double* pt;                 // [capacity][3]
    uint8_t* flags;             // [capacity]
    int32_t* counts;            // [4] n_new, n_candidates (k_kf_assemble); n_right, n_accepted (k_kf_finish)
    double* lambda_max;         // [1]
};
