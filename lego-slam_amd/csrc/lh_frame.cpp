// lh_frame.cpp — the two fused frontend calls of the C ABI (include/lego_ba.h), lh_track_frame and lh_insert_keyframe,
// each a short list of stages of a per-call context: check, buffers, upload, bind the kernels' arguments, enqueue,
// download, scatter, commit the resident image (lh_handle.h ResidentImage).  The arenas' layouts are
// lh_frontend_layout.h's; the pieces shared with the single-purpose calls are lh_frontend.cpp's (lh_frontend.h).
#include "lh_frontend.h"

using namespace lh;

namespace {

// ---- lh_track_frame: Frontend::Track (frontend_lego.cpp:48-75) in one call (include/lego_ba.h) ----
// Upload img2 (and img1, unless the resident image stands in for it) and one arena; k_track_guess, the tracker's
// kernels, k_track_pack and k_frames behind one another on the device buffers; one download; one synchronise.  The edge
// count stays on the device until then: k_frames reads it from the obs_ptr k_track_pack wrote.
struct TrackCall {
    lh_handle* h;
    const lh_track_input* in;
    lh_track_result* out;
    const lh_klt_input& k;
    const int n;
    const size_t N;
    const TrackLayout ly;
    FrontendCall call;
    hipStream_t s;
    FrontendState& fe;
    const int slot_I, slot_J;   // the resident image, read as img1, and the buffer in which img2 becomes the next one
    const int have_I;           // I's first level to build (n == 0: no I)
    lh_klt_args a{};
    lh_track_args t{};
    TrackCall(lh_handle* hh, const lh_track_input* i, lh_track_result* o)
        : h(hh), in(i), out(o), k(i->klt), n(k.n_points), N((size_t)n), ly(N, i->has_point != nullptr), call(hh),
          s(call.s), fe(hh->fe), slot_I(fe.res.slot()), slot_J(1 - slot_I),
          have_I(n == 0 ? LH_KLT_MAX_LEVELS : fe.res.first_level_to_build(k.img1 != nullptr)) {}
    int buffers();
    int upload();
    void bind();
    int enqueue();
    int download();
    int scatter();
};

int track_check(const ResidentImage& res, const lh_track_input* in, const lh_track_result* out) {
    lh_klt_input chk = in->klt;   // lh_klt_track's argument checks; a null img1 is the resident image
    if (!chk.img1) chk.img1 = chk.img2;
    STAGE(klt_check(&chk, out->kp2, out->success));
    if (!points_optional_ok(chk.n_points, in->pts_w, in->has_point)) return LH_E_BADARG;
    if (chk.n_points > 0 && !in->klt.img1 && !res.matches(chk.cols, chk.rows)) return LH_E_STATE;
    return LH_OK;
}

// From here on the resident image is in the making: valid again once the call has succeeded
int TrackCall::buffers() {
    fe.res.invalidate();
    const size_t bytes = pyramid_bytes(k.cols, k.rows);   // every level, whatever max_level a call asks for
    HIPCHK(fe.res.img[slot_J].ensure(bytes));
    if (n == 0) return LH_OK;
    HIPCHK(fe.res.img[slot_I].ensure(bytes));   // no change of a resident image: its size is this one
    HIPCHK(fe.tk_in.ensure(ly.i_end));
    HIPCHK(fe.tk_out.ensure(ly.o_end));
    HIPCHK(fe.tk_work.ensure(ly.w_end));
    HIPCHK(fe.f_res.ensure(2 * N));
    HIPCHK(fe.s_tkin.ensure(ly.i_end));
    HIPCHK(fe.s_tkout.ensure(ly.o_end));
    return LH_OK;
}

int TrackCall::upload() {
    HIPCHK(upload_rows(s, fe.res.img[slot_J].p, k.img2, k.cols, k.rows, k.step));
    if (n == 0) return LH_OK;
    if (k.img1) HIPCHK(upload_rows(s, fe.res.img[slot_I].p, k.img1, k.cols, k.rows, k.step));
    uint8_t* st = fe.s_tkin.p;
    const ByteSeg seg[4] = {{st + ly.i_pose, in->pose_Tcw, sizeof(double) * 12},
                            {st + ly.i_pts, in->pts_w, in->pts_w ? sizeof(double) * 3 * N : 0},
                            {st + ly.i_kp1, k.kp1, sizeof(float) * 2 * N},
                            {st + ly.i_hp, in->has_point, in->has_point ? N : 0}};
    par_copy(h, seg, 4);
    HIPCHK(hipMemcpyAsync(fe.tk_in.p, st, ly.i_end, hipMemcpyHostToDevice, s));
    return LH_OK;
}

void TrackCall::bind() {
    a = klt_args(k, fe.res.img[slot_I].p, fe.res.img[slot_J].p, k.cols, 1);
    if (n == 0) return;   // no launch but those of J's pyramid
    uint8_t *ti = fe.tk_in.p, *to = fe.tk_out.p, *tw = fe.tk_work.p;
    t.n_points = n;
    t.kp1 = (const float*)(ti + ly.i_kp1);
    t.pts_w = (const double*)(ti + ly.i_pts);
    t.has_point = in->has_point ? ti + ly.i_hp : nullptr;
    for (int i = 0; i < 12; ++i) { t.pose[i] = in->pose_Tcw[i]; t.ext[i] = in->cam_ext[i]; }
    for (int i = 0; i < 4; ++i) t.K[i] = in->K[i];
    t.kp2 = (float*)(to + ly.o_kp2);
    t.success = to + ly.o_succ;
    t.obs_ptr = (int64_t*)(tw + ly.w_ptr);
    t.pts = (double*)(tw + ly.w_pts);
    t.uv = (double*)(tw + ly.w_uv);
    t.edge_feature = (int32_t*)(to + ly.o_idx);
    t.counts = (int32_t*)(to + ly.o_cnt);
    a.n_points = n;
    a.kp1 = t.kp1;
    a.kp2 = t.kp2;
    a.success = to + ly.o_succ;
}

int TrackCall::enqueue() {
    uint8_t *ti = fe.tk_in.p, *to = fe.tk_out.p;
    STAGE(call.start());
    HIPCHK(lh_launch_track_guess(s, &t));
    STAGE(klt_pyr_track(s, a, have_I));
    if (n > 0) {
        HIPCHK(lh_launch_track_pack(s, &t));
        HIPCHK(lh_launch_frames(s, 1, t.obs_ptr, (const double*)(ti + ly.i_pose), t.pts, t.uv, nullptr, frames_params(h, in->K),
                                fe.f_res.p, (double*)(to + ly.o_pose), to + ly.o_flag, (double*)(to + ly.o_chi), t.counts + 2,
                                t.counts + 3));
    }
    return call.stop();
}

// one download, up to the last output the caller asked for, and the call's one synchronise
int TrackCall::download() {
    const size_t want = out->edge_chi2 ? ly.o_end : out->is_outlier ? ly.o_chi : ly.o_idx;
    if (n > 0) HIPCHK(hipMemcpyAsync(fe.s_tkout.p, fe.tk_out.p, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return LH_OK;
}

// the staging to the caller (n > 0): the features' outputs as they are, the edges' outputs back to their features
int TrackCall::scatter() {
    const uint8_t* st = fe.s_tkout.p;
    const int32_t* cnt = (const int32_t*)(st + ly.o_cnt);
    const int32_t m = cnt[1];
    if (m < 0 || m > n) return LH_E_HIP;
    const ByteSeg seg[3] = {{out->pose_Tcw, st + ly.o_pose, sizeof(double) * 12},
                            {out->kp2, st + ly.o_kp2, sizeof(float) * 2 * N},
                            {out->success, st + ly.o_succ, N}};
    par_copy(h, seg, 3);
    out->n_tracked = cnt[0];
    out->n_edges = m;
    out->iterations = cnt[2];
    out->n_inliers = cnt[3];
    const int32_t* idx = (const int32_t*)(st + ly.o_idx);
    if (out->is_outlier) {
        std::fill(out->is_outlier, out->is_outlier + n, (uint8_t)0);
        for (int32_t e = 0; e < m; ++e) out->is_outlier[idx[e]] = st[ly.o_flag + e];
    }
    if (out->edge_chi2) {
        std::fill(out->edge_chi2, out->edge_chi2 + n, 0.0);
        const double* chi = (const double*)(st + ly.o_chi);
        for (int32_t e = 0; e < m; ++e) out->edge_chi2[idx[e]] = chi[e];
    }
    return LH_OK;
}

int track_frame_impl(lh_handle* h, const lh_track_input* in, lh_track_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    STAGE(track_check(h->fe.res, in, out));
    for (int i = 0; i < 12; ++i) out->pose_Tcw[i] = in->pose_Tcw[i];
    out->n_tracked = out->n_edges = out->n_inliers = out->iterations = 0;
    out->time_ms = 0.0;
    if (in->klt.n_points == 0 && !in->klt.img2) return LH_OK;
    TrackCall c(h, in, out);
    STAGE(c.call.select());
    STAGE(c.buffers());
    STAGE(c.upload());
    c.bind();
    STAGE(c.enqueue());
    STAGE(c.download());
    if (c.n > 0) STAGE(c.scatter());
    STAGE(c.call.time(&out->time_ms));
    h->fe.res.commit(c.slot_J, c.k.cols, c.k.rows, c.a.n_levels);
    return LH_OK;
}

// ---- lh_insert_keyframe: Frontend::InsertKeyframe's and StereoInit's chain (frontend_lego.cpp:77-102, :323-362) in
// one call (include/lego_ba.h) ----
// Upload img_right (and img_left, unless the resident image stands in for it) and one arena; the detector on level 0 of
// the resident pyramid, k_kf_assemble, the tracker's kernels, k_triangulate and k_kf_finish behind one another on the
// device buffers; one download.  The corner count stays on the device until then: every launch behind the detector is
// sized for n_have + max_corners slots (lh_keyframe.h).  The host waits where the detector always has, between batches
// of selection rounds, and once at the end.
struct KeyframeCall {
    lh_handle* h;
    const lh_keyframe_input* in;
    lh_keyframe_result* out;
    const lh_klt_input k;       // the call as lh_klt_track's input (keyframe_klt)
    const int nh, mc, cap;
    const size_t NH;
    const KeyframeLayout ly;
    FrontendCall call;
    hipStream_t s;
    FrontendState& fe;
    const int slot;             // the resident image: the left one
    const int have_I;           // the left pyramid's first level to build
    lh_gftt_args g{};
    lh_kf_args f{};
    lh_klt_args a{};
    lh_tri_args t{};
    KeyframeCall(lh_handle* hh, const lh_keyframe_input* i, lh_keyframe_result* o, const lh_klt_input& kk)
        : h(hh), in(i), out(o), k(kk), nh(i->n_have), mc(i->max_corners), cap(nh + mc), NH((size_t)nh),
          ly(NH, (size_t)mc, i->have_point != nullptr), call(hh), s(call.s), fe(hh->fe), slot(fe.res.slot()),
          have_I(fe.res.first_level_to_build(i->img_left != nullptr)) {}
    int buffers();
    int upload();
    void bind();
    int enqueue();
    int download();
    int scatter();
};

// the tracker's view of the call, for lh_klt_track's checks and its argument block
lh_klt_input keyframe_klt(const lh_keyframe_input* in, const lh_keyframe_result* out) {
    lh_klt_input k{};
    k.cols = in->cols; k.rows = in->rows; k.step = in->step;
    k.img1 = k.img2 = in->img_right;   // a null img_left is the resident image
    k.n_points = in->n_have + in->max_corners;
    k.kp1 = out->kp_right;             // (the list is made on the device: any non-null pointer passes the check)
    k.max_level = in->max_level; k.max_iters = in->max_iters;
    k.epsilon = in->epsilon; k.min_eig_threshold = in->min_eig_threshold;
    return k;
}

// lh_detect_features' argument errors (mask == NULL), then lh_klt_track's (k: keyframe_klt once these have passed)
int keyframe_check(const ResidentImage& res, const lh_keyframe_input* in, const lh_keyframe_result* out, lh_klt_input* k) {
    const int nh = in->n_have, mc = in->max_corners;
    if (!image_ok(in->cols, in->rows, in->step)) return LH_E_BADARG;
    if (nh < 0 || (nh > 0 && !in->have_kp) || mc <= 0 || (int64_t)nh + mc > LH_KF_MAX_FEATURES) return LH_E_BADARG;
    if (!(in->quality_level >= 0.0) || !(in->min_distance >= 0.0)) return LH_E_BADARG;
    if (!in->img_right || !out->kp_new || !out->kp_right || !out->success || !out->pt || !out->flags) return LH_E_BADARG;
    *k = keyframe_klt(in, out);
    STAGE(klt_check(k, out->kp_right, out->success));
    if (!points_optional_ok(nh, in->have_pts_w, in->have_point)) return LH_E_BADARG;
    if (!in->img_left && !res.matches(in->cols, in->rows)) return LH_E_STATE;
    return LH_OK;
}

// Once every buffer of the call's own is there, the resident image is in the making (a given img_left replaces it, its
// buffer first if that has to grow; then the enqueueing begins): valid again once the call has succeeded.  A resident
// image that stays has this call's size, and its buffer every level's room.
int KeyframeCall::buffers() {
    const size_t pyr_bytes = pyramid_bytes(in->cols, in->rows);
    HIPCHK(fe.kf_right.ensure(pyr_bytes));
    HIPCHK(fe.kf_in.ensure(ly.i_end));
    HIPCHK(fe.kf_out.ensure(ly.o_end));
    HIPCHK(fe.kf_state.ensure((size_t)cap));
    HIPCHK(fe.s_kfin.ensure(ly.i_up));
    HIPCHK(fe.s_kfout.ensure(ly.o_end));
    STAGE(gftt_prepare(fe, in->cols, in->rows, in->quality_level, in->min_distance, mc, &g));
    fe.res.invalidate();
    if (in->img_left) HIPCHK(fe.res.img[slot].ensure(pyr_bytes));
    return LH_OK;
}

// The upload ends with have_kp, the head of the feature list; the device arena goes on for the corners behind it
int KeyframeCall::upload() {
    HIPCHK(upload_rows(s, fe.kf_right.p, in->img_right, in->cols, in->rows, in->step));
    if (in->img_left) HIPCHK(upload_rows(s, fe.res.img[slot].p, in->img_left, in->cols, in->rows, in->step));
    uint8_t* st = fe.s_kfin.p;
    const ByteSeg seg[5] = {{st + ly.i_cam, in->cam_pose, sizeof(double) * 24},
                            {st + ly.i_K, in->cam_K, sizeof(double) * 8},
                            {st + ly.i_pts, in->have_pts_w, in->have_pts_w ? sizeof(double) * 3 * NH : 0},
                            {st + ly.i_hp, in->have_point, in->have_point ? NH : 0},
                            {st + ly.i_kl, in->have_kp, sizeof(float) * 2 * NH}};
    par_copy(h, seg, 5);
    HIPCHK(hipMemcpyAsync(fe.kf_in.p, st, ly.i_up, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(fe.g_allow.p, 1, (size_t)in->rows * (size_t)in->cols, s));
    HIPCHK(hipMemsetAsync(fe.g_ctl.p, 0, sizeof(lh_gftt_ctl), s));
    return LH_OK;
}

void KeyframeCall::bind() {
    uint8_t *ki = fe.kf_in.p, *ko = fe.kf_out.p, *left = fe.res.img[slot].p;
    float* kl = (float*)(ki + ly.i_kl);
    g.img = left;         // level 0 of the resident pyramid: rows packed to cols, the layout g_img has
    g.n_exclude = nh; g.exclude_pt = kl; g.exclude_half = in->exclude_half;
    g.kp = kl + 2 * NH;   // the corners straight into the feature list, behind have_kp
    f.n_have = nh; f.max_corners = mc;
    f.ctl = g.ctl;
    f.pts_w = (const double*)(ki + ly.i_pts);
    f.has_point = in->have_point ? ki + ly.i_hp : nullptr;
    for (int i = 0; i < 12; ++i) { f.pose[i] = in->pose_Tcw[i]; f.ext[i] = in->cam_pose[1][i]; }
    for (int i = 0; i < 4; ++i) f.K[i] = in->cam_K[1][i];
    f.kl = kl;
    f.kp_right = (float*)(ko + ly.o_kpr);
    f.state = fe.kf_state.p;
    f.kp_new = (float*)(ko + ly.o_new);
    f.success = ko + ly.o_succ;
    f.pt = (double*)(ko + ly.o_pt);
    f.flags = ko + ly.o_flag;
    f.counts = (int32_t*)(ko + ly.o_cnt);
    f.lambda_max = (double*)(ko + ly.o_lam);
    a = klt_args(k, left, fe.kf_right.p, in->cols, 1);
    a.n_points = cap;
    a.kp1 = kl;
    a.kp2 = f.kp_right;
    a.success = ko + ly.o_succ;
    tri_tests(&t, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out);
    t.n_points = cap; t.n_poses = 2;
    t.pose = (const double*)(ki + ly.i_cam);
    t.cam_K = (const double*)(ki + ly.i_K);
    t.kp1 = kl; t.kp2 = f.kp_right; t.success = f.success;
    t.pt = f.pt; t.flags = f.flags;
}

int KeyframeCall::enqueue() {
    STAGE(call.start());
    STAGE(gftt_select(call, g));
    HIPCHK(lh_launch_kf_assemble(s, &f));
    STAGE(klt_pyr_track(s, a, have_I));
    HIPCHK(lh_launch_triangulate(s, &t));
    HIPCHK(lh_launch_kf_finish(s, &f));
    return call.stop();
}

int KeyframeCall::download() {
    HIPCHK(hipMemcpyAsync(fe.s_kfout.p, fe.kf_out.p, ly.o_end, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return LH_OK;
}

int KeyframeCall::scatter() {
    const uint8_t* st = fe.s_kfout.p;
    const int32_t* cnt = (const int32_t*)(st + ly.o_cnt);
    const int32_t m = cnt[0];
    if (m < 0 || m > mc) return LH_E_HIP;
    const size_t n = NH + (size_t)m;
    const ByteSeg seg[5] = {{out->kp_new, st + ly.o_new, sizeof(float) * 2 * (size_t)m},
                            {out->kp_right, st + ly.o_kpr, sizeof(float) * 2 * n},
                            {out->success, st + ly.o_succ, n},
                            {out->pt, st + ly.o_pt, sizeof(double) * 3 * n},
                            {out->flags, st + ly.o_flag, n}};
    par_copy(h, seg, 5);
    out->n_new = m;
    out->n_candidates = cnt[1];
    out->n_right = cnt[2];
    out->n_accepted = cnt[3];
    out->lambda_max = *(const double*)(st + ly.o_lam);
    return LH_OK;
}

int insert_keyframe_impl(lh_handle* h, const lh_keyframe_input* in, lh_keyframe_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    lh_klt_input k;
    STAGE(keyframe_check(h->fe.res, in, out, &k));
    out->n_new = out->n_candidates = out->n_right = out->n_accepted = 0;
    out->lambda_max = 0.0;
    out->time_ms = 0.0;
    KeyframeCall c(h, in, out, k);
    STAGE(c.call.select());
    STAGE(c.buffers());
    STAGE(c.upload());
    c.bind();
    STAGE(c.enqueue());
    STAGE(c.download());
    STAGE(c.scatter());
    STAGE(c.call.time(&out->time_ms));
    // the left pyramid's levels: those this call built, and those a resident image that stayed had before
    h->fe.res.commit(c.slot, in->cols, in->rows, std::max(c.have_I, c.a.n_levels));
    return LH_OK;
}

}  // namespace

extern "C" {

int lh_track_frame(lh_handle* h, const lh_track_input* in, lh_track_result* out) {
    return no_throw(track_frame_impl, h, in, out);
}
int lh_insert_keyframe(lh_handle* h, const lh_keyframe_input* in, lh_keyframe_result* out) {
    return no_throw(insert_keyframe_impl, h, in, out);
}

}  // extern "C"
