// lh_track.hip — the two kernels lh_track_frame (include/lego_ba.h) puts around k_klt_track and
// k_frames, so that one frame of Frontend::Track needs no host step in between:
//   k_track_guess  one lane per feature: the tracker's initial guess, the map point projected with the predicted
//                  pose (lh_track.h) or kp1 where the feature has none, written where k_klt_track reads its guesses;
//   k_track_pack   the features with success and a point, in ascending feature index, as k_frames' one frame
//                  (obs_ptr = {0, m}, points, pixels), the edge -> feature list and the two counts.  One workgroup
//                  walks the features in tiles of TP_BLOCK: a wave ranks its lanes by a ballot and a popcount of the
//                  lower lanes, the wave totals meet in LDS, and a base carried from tile to tile (the same in every
//                  thread) places the tile.  No atomic claims a slot: the order is the feature order for any count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LH_TRACK_IMPL
#include "lh_launch.h"

#define TG_BLOCK 64    // one wave per workgroup: a frame's features (150 .. 2000) then spread over the CUs
#define TP_BLOCK 256   // the pack's one workgroup
#define TP_WAVES (TP_BLOCK / 64)

__global__ __launch_bounds__(TG_BLOCK) void k_track_guess(lh_track_args a) {
    const int i = blockIdx.x * TG_BLOCK + threadIdx.x;
    if (i >= a.n_points) return;
    float gu = a.kp1[2 * i], gv = a.kp1[2 * i + 1];
    if (!a.has_point || a.has_point[i]) {
        const double X[3] = {a.pts_w[3 * (int64_t)i], a.pts_w[3 * (int64_t)i + 1], a.pts_w[3 * (int64_t)i + 2]};
        lh_track_guess(a.pose, a.ext, a.K, X, &gu, &gv);
    }
    a.kp2[2 * i] = gu;
    a.kp2[2 * i + 1] = gv;
}

__global__ __launch_bounds__(TP_BLOCK) void k_track_pack(lh_track_args a) {
    __shared__ int s_edges[TP_WAVES], s_tracked[TP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, tracked = 0;   // edges and tracked features of the tiles before this one
    for (int t0 = 0; t0 < a.n_points; t0 += TP_BLOCK) {
        const int i = t0 + tid;
        const bool ok = i < a.n_points && a.success[i] != 0;
        const bool edge = ok && (!a.has_point || a.has_point[i] != 0);
        const unsigned long long m_edge = __ballot(edge), m_ok = __ballot(ok);
        if (lane == 0) {
            s_edges[wave] = __popcll(m_edge);
            s_tracked[wave] = __popcll(m_ok);
        }
        __syncthreads();
        int before = 0, tile_edges = 0, tile_tracked = 0;
#pragma unroll
        for (int w = 0; w < TP_WAVES; ++w) {
            before += w < wave ? s_edges[w] : 0;
            tile_edges += s_edges[w];
            tile_tracked += s_tracked[w];
        }
        if (edge) {
            const int64_t e = base + before + __popcll(m_edge & ((1ull << lane) - 1ull));   // e <= i < n_points
            a.pts[3 * e] = a.pts_w[3 * (int64_t)i];
            a.pts[3 * e + 1] = a.pts_w[3 * (int64_t)i + 1];
            a.pts[3 * e + 2] = a.pts_w[3 * (int64_t)i + 2];
            a.uv[2 * e] = (double)a.kp2[2 * i];
            a.uv[2 * e + 1] = (double)a.kp2[2 * i + 1];
            a.edge_feature[e] = i;
        }
        base += tile_edges;
        tracked += tile_tracked;
        __syncthreads();   // the next tile overwrites the wave totals
    }
    if (tid == 0) {
        a.obs_ptr[0] = 0;
        a.obs_ptr[1] = base;
        a.counts[0] = tracked;
        a.counts[1] = base;
    }
}

extern "C" {

hipError_t lh_launch_track_guess(hipStream_t st, const lh_track_args* a) {
    if (a->n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_track_guess, dim3((unsigned)((a->n_points + TG_BLOCK - 1) / TG_BLOCK)), dim3(TG_BLOCK), 0, st, *a);
    return hipGetLastError();
}

hipError_t lh_launch_track_pack(hipStream_t st, const lh_track_args* a) {
    if (a->n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_track_pack, dim3(1), dim3(TP_BLOCK), 0, st, *a);
    return hipGetLastError();
}

}  // extern "C"
