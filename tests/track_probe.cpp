// track_probe.cpp — lego-slam_amd/csrc/lh_track.h compiled for the host (tests/test_track_cpu.py builds it with
// -ffp-contract=off): k_track_guess's arithmetic with a serial loop where the device has lanes.
#define LH_TRACK_IMPL
#include "lh_track.h"

extern "C" void track_guess(int n, const double* pts_w, const uint8_t* has_point, const float* kp1, const double* T,
                            const double* E, const double* K, float* out) {
    for (int i = 0; i < n; ++i) {
        out[2 * i] = kp1[2 * i];
        out[2 * i + 1] = kp1[2 * i + 1];
        if (!has_point || has_point[i]) lh_track_guess(T, E, K, pts_w + 3 * i, &out[2 * i], &out[2 * i + 1]);
    }
}
