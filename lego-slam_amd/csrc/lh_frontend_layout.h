// lh_frontend_layout.h — the byte layouts of the frontend's arenas (lh_frontend.cpp, lh_frame.cpp), each a plain struct
// of offsets computed from counts alone.  No HIP type and no handle: any host compiler builds it, and
// tests/frontend_layout_probe.cpp prints every offset for tests/test_frontend_layout_cpu.py.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lh {

// Segments behind one another in one allocation: take() returns the current end and moves it on by `bytes` rounded up
// to `align` (a power of two), so a segment that begins aligned leaves the next one aligned
struct Arena {
    size_t end = 0;
    size_t take(size_t bytes, size_t align = 16) {
        const size_t at = end;
        end += (bytes + align - 1) & ~(align - 1);
        return at;
    }
};

// lh_estimate_pose, F frames with O observations in all.  The upload: obs_ptr int64 [F + 1], poses double [F][12],
// points double [O][3], pixels double [O][2], the outlier flags [O] when given.  The download: poses, the edges' chi2
// double [O], iterations and inlier counts int32 [F], flags [O]
struct FramesLayout {
    size_t i_ptr, i_pose, i_pts, i_uv, i_flag, i_end;
    size_t o_pose, o_rchi2, o_iters, o_inl, o_flag, o_end;
    FramesLayout(size_t F, size_t O, bool has_flag) {
        Arena i, o;
        i_ptr = i.take(sizeof(int64_t) * (F + 1));
        i_pose = i.take(sizeof(double) * 12 * F);
        i_pts = i.take(sizeof(double) * 3 * O);
        i_uv = i.take(sizeof(double) * 2 * O);
        i_flag = i.take(has_flag ? O : 0);
        i_end = i.end;
        o_pose = o.take(sizeof(double) * 12 * F);
        o_rchi2 = o.take(sizeof(double) * O);
        o_iters = o.take(sizeof(int32_t) * F);
        o_inl = o.take(sizeof(int32_t) * F);
        o_flag = o.take(O);
        o_end = o.end;
    }
};

// lh_track_frame, n features.  The upload: the pose double [12], points double [n][3], kp1 float [n][2], the has_point
// bytes [n] when given.  The download: the pose, four int32 counts, kp2 float [n][2], success [n], the edge -> feature
// list int32 [n], the edges' flags [n] and chi2 double [n].  The work arena, k_frames' inputs as k_track_pack writes
// them: obs_ptr int64 [2], points double [n][3], pixels double [n][2]
struct TrackLayout {
    size_t i_pose, i_pts, i_kp1, i_hp, i_end;
    size_t o_pose, o_cnt, o_kp2, o_succ, o_idx, o_flag, o_chi, o_end;
    size_t w_ptr, w_pts, w_uv, w_end;
    TrackLayout(size_t n, bool has_point) {
        Arena i, o, w;
        i_pose = i.take(sizeof(double) * 12);
        i_pts = i.take(sizeof(double) * 3 * n);
        i_kp1 = i.take(sizeof(float) * 2 * n);
        i_hp = i.take(has_point ? n : 0);
        i_end = i.end;
        o_pose = o.take(sizeof(double) * 12);
        o_cnt = o.take(sizeof(int32_t) * 4);
        o_kp2 = o.take(sizeof(float) * 2 * n);
        o_succ = o.take(n);
        o_idx = o.take(sizeof(int32_t) * n);
        o_flag = o.take(n);
        o_chi = o.take(sizeof(double) * n);
        o_end = o.end;
        w_ptr = w.take(sizeof(int64_t) * 2);
        w_pts = w.take(sizeof(double) * 3 * n);
        w_uv = w.take(sizeof(double) * 2 * n);
        w_end = w.end;
    }
};

// lh_insert_keyframe, n_have features and room for max_corners more.  The input arena: both cameras' poses double
// [2][12] and intrinsics double [2][4] (neither padded), the features' points double [n_have][3], their has_point bytes
// [n_have] when given, then the feature list float [n_have + max_corners][2].  The upload ends at i_up, behind have_kp,
// the list's head; the device arena goes on to i_end for the corners behind it (neither is padded).  The download:
// four int32 counts, lambda_max (a double at 16), pt double [cap][3] at 32, kp_right float [cap][2], the corners float
// [max_corners][2], success [cap], flags [cap]
struct KeyframeLayout {
    size_t i_cam, i_K, i_pts, i_hp, i_kl, i_up, i_end;
    size_t o_cnt, o_lam, o_pt, o_kpr, o_new, o_succ, o_flag, o_end;
    KeyframeLayout(size_t n_have, size_t max_corners, bool has_point) {
        const size_t cap = n_have + max_corners;
        Arena i, o;
        i_cam = i.take(sizeof(double) * 24, 1);
        i_K = i.take(sizeof(double) * 8, 1);
        i_pts = i.take(sizeof(double) * 3 * n_have);
        i_hp = i.take(has_point ? n_have : 0);
        i_kl = i.end;
        i_up = i_kl + sizeof(float) * 2 * n_have;
        i_end = i_kl + sizeof(float) * 2 * cap;
        o_cnt = o.take(sizeof(int32_t) * 4, 1);
        o_lam = o.take(sizeof(double));
        o_pt = o.take(sizeof(double) * 3 * cap);
        o_kpr = o.take(sizeof(float) * 2 * cap);
        o_new = o.take(sizeof(float) * 2 * max_corners);
        o_succ = o.take(cap);
        o_flag = o.take(cap);
        o_end = o.end;
    }
};

// k_triangulate's output arena for n points (lh_triangulate, the two stereo calls): pt double [n][3], sing_ratio
// double [n], flags [n], none padded
struct TriOut {
    size_t o_pt, o_ratio, o_flag, o_end;
    explicit TriOut(size_t n) {
        Arena o;
        o_pt = o.take(sizeof(double) * 3 * n, 1);
        o_ratio = o.take(sizeof(double) * n, 1);
        o_flag = o.take(n, 1);
        o_end = o.end;
    }
};

}  // namespace lh
