// Prints every offset of the frontend's arena layouts (lego-slam_amd/csrc/lh_frontend_layout.h, plain C++) for the
// counts tests/test_frontend_layout_cpu.py compares against the formulas they were written from.  One line per layout:
//   <kind> <count> <count> <flag> <name>=<offset> ...
#include <cstdio>

#include "lh_frontend_layout.h"

#define F(name) printf(" " #name "=%zu", ly.name)

static void frames(size_t nf, size_t no, int has_flag) {
    const lh::FramesLayout ly(nf, no, has_flag != 0);
    printf("frames %zu %zu %d", nf, no, has_flag);
    F(i_ptr); F(i_pose); F(i_pts); F(i_uv); F(i_flag); F(i_end);
    F(o_pose); F(o_rchi2); F(o_iters); F(o_inl); F(o_flag); F(o_end);
    printf("\n");
}

static void track(size_t n, int has_point) {
    const lh::TrackLayout ly(n, has_point != 0);
    printf("track %zu 0 %d", n, has_point);
    F(i_pose); F(i_pts); F(i_kp1); F(i_hp); F(i_end);
    F(o_pose); F(o_cnt); F(o_kp2); F(o_succ); F(o_idx); F(o_flag); F(o_chi); F(o_end);
    F(w_ptr); F(w_pts); F(w_uv); F(w_end);
    printf("\n");
}

static void keyframe(size_t n_have, size_t max_corners, int has_point) {
    const lh::KeyframeLayout ly(n_have, max_corners, has_point != 0);
    printf("keyframe %zu %zu %d", n_have, max_corners, has_point);
    F(i_cam); F(i_K); F(i_pts); F(i_hp); F(i_kl); F(i_up); F(i_end);
    F(o_cnt); F(o_lam); F(o_pt); F(o_kpr); F(o_new); F(o_succ); F(o_flag); F(o_end);
    printf("\n");
}

static void tri(size_t n) {
    const lh::TriOut ly(n);
    printf("tri %zu 0 0", n);
    F(o_pt); F(o_ratio); F(o_flag); F(o_end);
    printf("\n");
}

int main() {
    const size_t track_n[] = {0, 1, 2, 3, 5, 63, 64, 65, 257};
    const size_t kf[][2] = {{0, 7}, {1, 7}, {63, 7}, {64, 7}, {65, 7}, {257, 7}, {250, 40}};
    const size_t frames_f[] = {1, 3}, frames_o[] = {0, 1, 7, 40};
    for (int flag = 0; flag < 2; ++flag) {
        for (size_t n : track_n) track(n, flag);
        for (const auto& p : kf) keyframe(p[0], p[1], flag);
        for (size_t nf : frames_f)
            for (size_t no : frames_o) frames(nf, no, flag);
    }
    for (size_t n : track_n) tri(n);
    return 0;
}
