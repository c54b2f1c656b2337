// lh_keyframe.hip — the two kernels lh_insert_keyframe (include/lego_ba.h) puts between the detector,
// the tracker and the triangulation, so that a keyframe's chain needs no host step in between:
//   k_kf_assemble  one lane per slot of the feature list, behind k_gftt_rank.  It reads the corner count where the
//                  detector left it (lh_gftt_ctl), clamps it to max_corners, and makes the tracker's inputs: the guess of
//                  a feature with a point (lh_track.h's arithmetic, the right camera's extrinsic), the keypoint itself
//                  as the guess of one without, NaN keypoints and guesses in the slots past the list's end, and the
//                  slot's state.  The keypoints are in place already: have_kp as uploaded, the corners behind it where
//                  k_gftt_rank wrote them.  It also copies the corners and the detector's counts for the download.
//   k_kf_finish    one workgroup, behind k_triangulate: a feature with a point gets flag LH_TRI_F_HAS_POINT and pt = 0
//                  whatever the triangulation made of it; the tracked and the accepted features are counted (integer
//                  sums: a wave's by shuffles, the waves' through LDS).
// Neither touches memory past the capacity n_have + max_corners, whatever count the device holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LH_TRACK_IMPL
#include "lh_launch.h"

#define KA_BLOCK 64    // one wave per workgroup, as k_track_guess
#define KF_BLOCK 256   // the finish's one workgroup
#define KF_WAVES (KF_BLOCK / 64)

namespace {

// the corners in the list: the detector's count, never more than the room behind have_kp
__device__ __forceinline__ int kf_new_corners(const lh_kf_args& a) {
    const uint32_t acc = a.ctl->n_acc;
    return acc < (uint32_t)a.max_corners ? (int)acc : a.max_corners;
}

}  // namespace

__global__ __launch_bounds__(KA_BLOCK) void k_kf_assemble(lh_kf_args a) {
    const int i = blockIdx.x * KA_BLOCK + threadIdx.x;
    const int m = kf_new_corners(a);
    if (i == 0) {
        const unsigned long long mk = a.ctl->max_key;
        a.counts[0] = m;
        a.counts[1] = (int32_t)a.ctl->n_cand;
        *a.lambda_max = mk ? lh_gftt_unkey(mk) : 0.0;
    }
    if (i >= a.n_have + a.max_corners) return;
    float gu, gv;
    uint8_t state;
    if (i < a.n_have + m) {
        gu = a.kl[2 * i];
        gv = a.kl[2 * i + 1];
        state = LH_KF_S_NEW;
        if (i >= a.n_have) {
            a.kp_new[2 * (i - a.n_have)] = gu;
            a.kp_new[2 * (i - a.n_have) + 1] = gv;
        } else if (!a.has_point || a.has_point[i]) {
            const double X[3] = {a.pts_w[3 * (int64_t)i], a.pts_w[3 * (int64_t)i + 1], a.pts_w[3 * (int64_t)i + 2]};
            lh_track_guess(a.pose, a.ext, a.K, X, &gu, &gv);
            state = LH_KF_S_HAS_POINT;
        }
    } else {
        gu = gv = __builtin_nanf("");
        a.kl[2 * i] = gu;
        a.kl[2 * i + 1] = gv;
        state = LH_KF_S_UNUSED;
    }
    a.kp_right[2 * i] = gu;
    a.kp_right[2 * i + 1] = gv;
    a.state[i] = state;
}

__global__ __launch_bounds__(KF_BLOCK) void k_kf_finish(lh_kf_args a) {
    __shared__ int s_right[KF_WAVES], s_acc[KF_WAVES];
    const int tid = threadIdx.x;
    const int n = a.n_have + kf_new_corners(a);
    int right = 0, acc = 0;
    for (int i = tid; i < n; i += KF_BLOCK) {
        uint8_t f = a.flags[i];
        if (a.state[i] == LH_KF_S_HAS_POINT) {
            f = LH_TRI_F_HAS_POINT;
            a.flags[i] = f;
            a.pt[3 * (int64_t)i] = a.pt[3 * (int64_t)i + 1] = a.pt[3 * (int64_t)i + 2] = 0.0;
        }
        right += a.success[i] != 0;
        acc += f == 0;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        right += __shfl_xor(right, k, 64);
        acc += __shfl_xor(acc, k, 64);
    }
    if ((tid & 63) == 0) {
        s_right[tid >> 6] = right;
        s_acc[tid >> 6] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        right = acc = 0;
#pragma unroll
        for (int w = 0; w < KF_WAVES; ++w) {
            right += s_right[w];
            acc += s_acc[w];
        }
        a.counts[2] = right;
        a.counts[3] = acc;
    }
}

extern "C" {

hipError_t lh_launch_kf_assemble(hipStream_t st, const lh_kf_args* a) {
    const int cap = a->n_have + a->max_corners;
    if (cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kf_assemble, dim3((unsigned)((cap + KA_BLOCK - 1) / KA_BLOCK)), dim3(KA_BLOCK), 0, st, *a);
    return hipGetLastError();
}

hipError_t lh_launch_kf_finish(hipStream_t st, const lh_kf_args* a) {
    if (a->n_have + a->max_corners <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_kf_finish, dim3(1), dim3(KF_BLOCK), 0, st, *a);
    return hipGetLastError();
}

}  // extern "C"
