// lh_frontend.cpp — the frontend entry points of the C ABI (include/lego_ba.h) on the solver's handle and stream:
// lh_estimate_pose, lh_lk_track, lh_klt_track, lh_triangulate, lh_stereo_landmarks, lh_klt_stereo_landmarks,
// lh_detect_features.  Each checks its arguments, grows its buffers (lh_handle.h FrontendState), enqueues copies and
// kernels, synchronises and copies out.  The pieces that the fused calls of lh_frame.cpp (lh_track_frame,
// lh_insert_keyframe) are also made of come first, as lh:: functions (lh_frontend.h).
#include <cmath>

#include "lh_frontend.h"

using namespace lh;

namespace lh {

// an 8-bit image to the device with its rows packed to `cols` bytes: only `cols` bytes of a caller's row are readable
// (a cv::Mat ROI has step > cols)
hipError_t upload_rows(hipStream_t s, uint8_t* dst, const uint8_t* src, int cols, int rows, int64_t step) {
    if (step == cols) return hipMemcpyAsync(dst, src, (size_t)rows * (size_t)cols, hipMemcpyHostToDevice, s);
    return hipMemcpy2DAsync(dst, (size_t)cols, src, (size_t)step, (size_t)cols, (size_t)rows, hipMemcpyHostToDevice, s);
}

// lh_params of the handle's options with a frame's intrinsics (k_frames)
lh_params frames_params(const lh_handle* h, const double* K) {
    lh_params prm{};
    prm.max_iters = h->opt.max_iters;
    prm.max_trials = h->opt.max_trials;
    prm.strategy = h->opt.strategy;
    prm.lambda_given = h->opt.lambda_init >= 0.0;
    prm.gate_mode = h->opt.gate_mode;
    prm.precision = h->opt.precision;
    prm.huber_delta = h->opt.huber_delta;
    prm.stop_dchi2 = h->opt.stop_dchi2;
    prm.tau = h->opt.tau;
    prm.lambda_cap = h->opt.lambda_cap;
    prm.lambda_init = h->opt.lambda_init;
    for (int i = 0; i < 4; ++i) prm.K[i] = K[i];
    return prm;
}

// n features' world points may be missing (pts_w null) only if has_point says that no feature has one
bool points_optional_ok(int n, const double* pts_w, const uint8_t* has_point) {
    if (n <= 0 || pts_w) return true;
    return has_point && std::all_of(has_point, has_point + n, [](uint8_t b) { return b == 0; });
}

// the detector's image: 3 x 3 at least, rows `step` bytes apart, pixel indices that fit 32 bits
bool image_ok(int cols, int rows, int64_t step) {
    return cols >= 3 && rows >= 3 && step >= cols && (int64_t)rows * cols <= INT32_MAX;
}

// legoslam::triangulation (algorithm.h:11-34) for a batch of points (k_triangulate, lh_tri.hip).
// The tests lh_triangulate, the stereo calls and lh_insert_keyframe share: threshold, gate, T_out.
void tri_tests(lh_tri_args* a, double thr, int gate, double y_max, double z_min, double z_max, const double* T_out) {
    a->thr = thr;
    a->gate = gate ? 1 : 0;
    a->y_max = y_max; a->z_min = z_min; a->z_max = z_max;
    a->has_T = T_out ? 1 : 0;
    for (int i = 0; i < 12; ++i) a->T[i] = T_out ? T_out[i] : 0.0;
}

// cv::calcOpticalFlowPyrLK as lh_klt.h defines it (include/lego_ba.h).  klt_check: the argument errors.
int klt_check(const lh_klt_input* in, const float* kp2, const uint8_t* success) {
    if (in->cols < LH_KLT_MIN_SIZE || in->rows < LH_KLT_MIN_SIZE || in->step < in->cols || in->n_points < 0) return LH_E_BADARG;
    if (in->max_level < 0 || in->max_level > LH_KLT_MAX_LEVELS - 1 || in->max_iters < 1) return LH_E_BADARG;
    if (!(in->epsilon > 0.0) || !(in->min_eig_threshold >= 0.0)) return LH_E_BADARG;
    if (in->n_points > 0 && (!in->img1 || !in->img2 || !in->kp1 || !kp2 || !success)) return LH_E_BADARG;
    return LH_OK;
}

// One image's pyramid in a buffer: level 0 with rows `step` bytes apart, levels 1 .. n_levels - 1 packed behind it.
// Fills v's step and (with a buffer) data from its cols and rows; returns the bytes.
int64_t klt_pyramid_layout(lh_klt_levels* v, int n_levels, uint8_t* buf, int64_t step) {
    int64_t total = (int64_t)v->rows[0] * step;
    v->step[0] = step;
    v->data[0] = buf;
    for (int l = 1; l < n_levels; ++l) {
        v->step[l] = v->cols[l];
        v->data[l] = buf ? buf + total : nullptr;
        total += (int64_t)v->cols[l] * v->rows[l];
    }
    return total;
}

// that layout's bytes for a cols x rows image with the levels max_level asks for
static size_t klt_pyramid_bytes(int cols, int rows, int max_level, int64_t step) {
    lh_klt_levels v{};
    return (size_t)klt_pyramid_layout(&v, lh_klt_level_sizes(cols, rows, max_level, v.cols, v.rows), nullptr, step);
}

// the resident layout (rows packed to cols) with every level: what the fused calls' pyramid buffers hold, whatever
// max_level a call asks for
size_t pyramid_bytes(int cols, int rows) { return klt_pyramid_bytes(cols, rows, LH_KLT_MAX_LEVELS - 1, cols); }

// The tracker's argument block but for its point lists (n_points, kp1, kp2, success): k's image size and levels with
// both pyramids laid out at I and J, level-0 rows `step` bytes apart, and k's iteration parameters.
lh_klt_args klt_args(const lh_klt_input& k, uint8_t* I, uint8_t* J, int64_t step, int has_initial) {
    lh_klt_args a{};
    a.n_levels = lh_klt_level_sizes(k.cols, k.rows, k.max_level, a.I.cols, a.I.rows);
    a.J = a.I;
    klt_pyramid_layout(&a.I, a.n_levels, I, step);
    klt_pyramid_layout(&a.J, a.n_levels, J, step);
    a.has_initial = has_initial;
    a.max_iters = k.max_iters;
    a.eps2 = k.epsilon * k.epsilon;
    a.min_eig = k.min_eig_threshold;
    return a;
}

// The tracker's kernels on images, keypoints and guesses that are on the device (a: both pyramids laid out): the levels
// first_I .. of I and 1 .. of J (k_klt_pyr, level by level, I before J), then k_klt_track.
int klt_pyr_track(hipStream_t s, const lh_klt_args& a, int first_I) {
    for (int l = 1; l < a.n_levels; ++l)
        for (int im = l < first_I ? 1 : 0; im < 2; ++im) {
            const lh_klt_levels& v = im ? a.J : a.I;
            HIPCHK(lh_launch_klt_pyr(s, v.data[l - 1], v.cols[l - 1], v.rows[l - 1], v.step[l - 1], const_cast<uint8_t*>(v.data[l]),
                                     v.cols[l], v.rows[l]));
        }
    HIPCHK(lh_launch_klt_track(s, &a));
    return LH_OK;
}

// Frontend::DetectFeatures (frontend_lego.cpp:292-310): the mask's exclusion boxes, then cv::GFTTDetector's
// corners, defined in exact arithmetic (lh_gftt.h).  The image, lambda and every list stay on
// the device; the host reads one lh_gftt_ctl per batch of selection rounds, to know when none is left open.
#define LH_GFTT_ROUND_BATCH 8   // a round that finds nothing open costs a launch; a check costs a synchronise

// The detector's working buffers for a cols x rows image and `limit` corners, and its arguments but for the image, the
// exclusion list and the corner list, which are the caller's (lh_insert_keyframe has all three elsewhere).
int gftt_prepare(FrontendState& fe, int cols, int rows, double quality_level, double min_distance, int limit, lh_gftt_args* a) {
    const size_t px = (size_t)rows * (size_t)cols;
    HIPCHK(fe.g_allow.ensure(px));
    HIPCHK(fe.g_state.ensure(px + 4));   // k_gftt_round reads it by aligned words
    HIPCHK(fe.g_eig.ensure(px));
    HIPCHK(fe.g_cand.ensure(px));
    HIPCHK(fe.g_acc_idx.ensure(px));
    HIPCHK(fe.g_acc_lam.ensure(px));
    HIPCHK(fe.g_resp.ensure((size_t)std::max(limit, 1)));
    HIPCHK(fe.g_ctl.ensure(1));
    HIPCHK(fe.s_gctl.ensure(1));
    a->cols = cols; a->rows = rows;
    a->allow = fe.g_allow.p;
    a->quality = quality_level;
    a->min_dist2 = min_distance * min_distance;
    // candidates nearer than min_distance differ by at most ceil(min_distance) - 1 pixels along an axis
    a->reach = min_distance < 1.0 ? -1 : (int)std::min(std::ceil(min_distance) - 1.0, (double)std::max(cols, rows));
    a->limit = limit;
    a->eig = fe.g_eig.p; a->state = fe.g_state.p; a->cand = fe.g_cand.p;
    a->acc_idx = fe.g_acc_idx.p; a->acc_lam = fe.g_acc_lam.p;
    a->response = fe.g_resp.p; a->ctl = fe.g_ctl.p;
    return LH_OK;
}

// The detector's kernels on an image, an allow image and a zeroed lh_gftt_ctl that are on the device: the front, the
// selection rounds in batches with a read of the control block after each, the ordered corner list.  On return the
// stream has drained up to the last batch of rounds; k_gftt_accepted and k_gftt_rank are enqueued behind it.
int gftt_select(FrontendCall& call, const lh_gftt_args& a) {
    hipStream_t s = call.s;
    FrontendState& fe = call.h->fe;
    HIPCHK(lh_launch_gftt_front(s, &a));
    const lh_gftt_ctl& ctl = *fe.s_gctl.p;
    if (a.reach >= 0)
        for (int r = 0;; r += LH_GFTT_ROUND_BATCH) {   // a round decides at least the strongest open candidate
            HIPCHK(lh_launch_gftt_rounds(s, &a, r, LH_GFTT_ROUND_BATCH));
            HIPCHK(hipMemcpyAsync(fe.s_gctl.p, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (ctl.open[(r + LH_GFTT_ROUND_BATCH - 1) % 3] == 0) break;
        }
    HIPCHK(lh_launch_gftt_order(s, &a));
    return LH_OK;
}

}  // namespace lh

namespace {

// Frontend::EstimateCurrentPose for a batch of frames (frontend_lego.cpp:157-250): upload, one
// k_frames launch (one workgroup per frame), download.
int estimate_pose_impl(lh_handle* h, const lh_frames* in, lh_frames_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const int F = in->n_frames;
    if (F < 0 || (F > 0 && (!in->obs_ptr || !in->pose_Tcw))) return LH_E_BADARG;
    if (F == 0) { out->time_ms = 0.0; return LH_OK; }
    if (in->obs_ptr[0] != 0) return LH_E_BADARG;
    for (int f = 0; f < F; ++f)
        if (in->obs_ptr[f + 1] < in->obs_ptr[f] || in->obs_ptr[f + 1] - in->obs_ptr[f] > (int64_t)INT32_MAX)
            return LH_E_BADARG;
    const int64_t O = in->obs_ptr[F];
    if (O > 0 && (!in->pts_w || !in->obs_uv)) return LH_E_BADARG;
    if (!out->pose_Tcw) return LH_E_BADARG;
    FrontendCall call(h);
    STAGE(call.select());
    hipStream_t s = call.s;
    FrontendState& fe = h->fe;
    const bool has_flag = in->is_outlier && O > 0;
    const FramesLayout ly((size_t)F, (size_t)O, has_flag);
    HIPCHK(fe.f_in.ensure(ly.i_end));
    HIPCHK(fe.f_out.ensure(ly.o_end));
    HIPCHK(fe.f_res.ensure(2 * (size_t)O));
    HIPCHK(fe.s_fin.ensure(ly.i_end));
    HIPCHK(fe.s_fout.ensure(ly.o_end));
    {
        uint8_t* st = fe.s_fin.p;
        const ByteSeg seg[5] = {{st + ly.i_ptr, in->obs_ptr, sizeof(int64_t) * (F + 1)},
                                {st + ly.i_pose, in->pose_Tcw, sizeof(double) * 12 * (size_t)F},
                                {st + ly.i_pts, in->pts_w, sizeof(double) * 3 * (size_t)O},
                                {st + ly.i_uv, in->obs_uv, sizeof(double) * 2 * (size_t)O},
                                {st + ly.i_flag, in->is_outlier, has_flag ? (size_t)O : 0}};
        par_copy(h, seg, 5);
    }
    HIPCHK(hipMemcpyAsync(fe.f_in.p, fe.s_fin.p, ly.i_end, hipMemcpyHostToDevice, s));
    uint8_t *fi = fe.f_in.p, *fo = fe.f_out.p;
    const lh_params prm = frames_params(h, in->K);
    STAGE(call.start());
    HIPCHK(lh_launch_frames(s, F, (const int64_t*)(fi + ly.i_ptr), (const double*)(fi + ly.i_pose),
                            (const double*)(fi + ly.i_pts), (const double*)(fi + ly.i_uv), has_flag ? fi + ly.i_flag : nullptr,
                            prm, fe.f_res.p, (double*)(fo + ly.o_pose), fo + ly.o_flag, (double*)(fo + ly.o_rchi2),
                            (int32_t*)(fo + ly.o_iters), (int32_t*)(fo + ly.o_inl)));
    STAGE(call.stop());
    // one download of what the caller asked for: the pose block always, the rest up to the last wanted
    const size_t want = out->is_outlier && O > 0 ? ly.o_end
                        : out->n_inliers         ? ly.o_flag
                        : out->iterations        ? ly.o_inl
                        : out->edge_chi2 && O > 0 ? ly.o_iters
                                                 : ly.o_rchi2;
    HIPCHK(hipMemcpyAsync(fe.s_fout.p, fo, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    {
        const uint8_t* st = fe.s_fout.p;
        const ByteSeg seg[5] = {{out->pose_Tcw, st + ly.o_pose, sizeof(double) * 12 * (size_t)F},
                                {out->edge_chi2, st + ly.o_rchi2, out->edge_chi2 ? sizeof(double) * (size_t)O : 0},
                                {out->iterations, st + ly.o_iters, out->iterations ? sizeof(int32_t) * (size_t)F : 0},
                                {out->n_inliers, st + ly.o_inl, out->n_inliers ? sizeof(int32_t) * (size_t)F : 0},
                                {out->is_outlier, st + ly.o_flag, out->is_outlier ? (size_t)O : 0}};
        par_copy(h, seg, 5);
    }
    return call.time(&out->time_ms);
}

// LKOpticalFlow4Layer / LKOpticalFlow1Layer (algorithm.cpp:11-206): upload both images, build the
// pyramids (k_lk_pyr per level and image), track every keypoint (k_lk_track), download.
// lk_enqueue: everything up to and including the tracking launch, on the call's stream; it starts the call's
// timing in front of the first kernel.  kp2 (host): the initial guess when in->has_initial.
int lk_enqueue(FrontendCall& call, const lh_lk_input* in, const float* kp2, const uint8_t* success) {
    if (in->levels != 1 && in->levels != LH_LK_MAX_LEVELS) return LH_E_BADARG;
    if (in->cols < 1 || in->rows < 1 || in->step < in->cols || in->n_points < 0) return LH_E_BADARG;
    if (!in->img1 || !in->img2) return LH_E_BADARG;
    const int n = in->n_points;
    if (n > 0 && (!in->kp1 || !kp2 || !success)) return LH_E_BADARG;
    STAGE(call.select());
    // level sizes: cv::Size(cols * 0.5, rows * 0.5) truncated (algorithm.cpp:146-153)
    int cols[LH_LK_MAX_LEVELS], rows[LH_LK_MAX_LEVELS];
    int64_t step[LH_LK_MAX_LEVELS], off[LH_LK_MAX_LEVELS];
    cols[0] = in->cols; rows[0] = in->rows; step[0] = in->step; off[0] = 0;
    int64_t total = (int64_t)in->rows * in->step;
    for (int l = 1; l < in->levels; ++l) {
        cols[l] = (int)(cols[l - 1] * 0.5);
        rows[l] = (int)(rows[l - 1] * 0.5);
        if (cols[l] < 1 || rows[l] < 1) return LH_E_BADARG;
        step[l] = cols[l];
        off[l] = total;
        total += (int64_t)cols[l] * rows[l];
    }
    hipStream_t s = call.s;
    FrontendState& fe = call.h->fe;
    HIPCHK(fe.k_img[0].ensure((size_t)total));
    HIPCHK(fe.k_img[1].ensure((size_t)total));
    HIPCHK(fe.k_kp1.ensure(2 * (size_t)std::max(n, 1)));
    HIPCHK(fe.k_kp2.ensure(2 * (size_t)std::max(n, 1)));
    HIPCHK(fe.k_succ.ensure((size_t)std::max(n, 1)));
    // the caller's last row guarantees only `cols` readable bytes (a cv::Mat ROI has step > cols):
    // copy (rows - 1) * step + cols bytes and zero the rest of that row, which no tap reads as image
    // data (GetPixelValue's out-of-buffer taps read 0, lh_lk.hip)
    const size_t img_bytes = (size_t)(in->rows - 1) * (size_t)in->step + (size_t)in->cols;
    const size_t tail = (size_t)in->rows * (size_t)in->step - img_bytes;
    for (int im = 0; im < 2; ++im) {
        HIPCHK(hipMemcpyAsync(fe.k_img[im].p, im ? in->img2 : in->img1, img_bytes, hipMemcpyHostToDevice, s));
        if (tail) HIPCHK(hipMemsetAsync(fe.k_img[im].p + img_bytes, 0, tail, s));
    }
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(fe.k_kp1.p, in->kp1, 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
        // without an initial guess kp2 is scaled but never read (dx = dy = 0 at the top level)
        if (in->has_initial) HIPCHK(hipMemcpyAsync(fe.k_kp2.p, kp2, 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
        else HIPCHK(hipMemsetAsync(fe.k_kp2.p, 0, 2 * sizeof(float) * (size_t)n, s));
    }
    lh_lk_levels L[2];
    for (int im = 0; im < 2; ++im)
        for (int l = 0; l < LH_LK_MAX_LEVELS; ++l) {
            const int ll = l < in->levels ? l : 0;
            L[im].data[l] = fe.k_img[im].p + off[ll];
            L[im].cols[l] = cols[ll];
            L[im].rows[l] = rows[ll];
            L[im].step[l] = step[ll];
        }
    STAGE(call.start());
    for (int l = 1; l < in->levels; ++l)
        for (int im = 0; im < 2; ++im)
            HIPCHK(lh_launch_lk_pyr(s, L[im].data[l - 1], cols[l - 1], rows[l - 1], step[l - 1],
                                    fe.k_img[im].p + off[l], cols[l], rows[l]));
    HIPCHK(lh_launch_lk_track(s, &L[0], &L[1], in->levels, n, fe.k_kp1.p, fe.k_kp2.p, fe.k_kp2.p, fe.k_succ.p,
                              in->inverse ? 1 : 0, in->has_initial ? 1 : 0));
    return LH_OK;
}

// the tracker's keypoints and success bytes to the caller (n > 0)
int lk_download(FrontendCall& call, int n, float* kp2, uint8_t* success) {
    const FrontendState& fe = call.h->fe;
    HIPCHK(hipMemcpyAsync(kp2, fe.k_kp2.p, 2 * sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, call.s));
    HIPCHK(hipMemcpyAsync(success, fe.k_succ.p, (size_t)n, hipMemcpyDeviceToHost, call.s));
    return LH_OK;
}

int lk_track_impl(lh_handle* h, const lh_lk_input* in, lh_lk_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    FrontendCall call(h);
    STAGE(lk_enqueue(call, in, out->kp2, out->success));
    STAGE(call.stop());
    if (in->n_points > 0) STAGE(lk_download(call, in->n_points, out->kp2, out->success));
    HIPCHK(hipStreamSynchronize(call.s));
    return call.time(&out->time_ms);
}

// the tests and the output arena t_out (o: TriOut of the call's points) of lh_triangulate and the stereo calls
int tri_outputs(lh_handle* h, lh_tri_args* a, double thr, int gate, double y_max, double z_min, double z_max,
                const double* T_out, const TriOut& o) {
    HIPCHK(h->fe.t_out.ensure(o.o_end));
    tri_tests(a, thr, gate, y_max, z_min, z_max, T_out);
    a->pt = (double*)(h->fe.t_out.p + o.o_pt);
    a->ratio = (double*)(h->fe.t_out.p + o.o_ratio);
    a->flags = h->fe.t_out.p + o.o_flag;
    return LH_OK;
}

// P poses [P][12], then (if given) their intrinsics [P][4], to the head of the input arena t_in
int tri_poses(FrontendCall& call, lh_tri_args* a, int P, const double* pose_Tcw, const double* cam_K) {
    uint8_t* ti = call.h->fe.t_in.p;
    const size_t i_K = sizeof(double) * 12 * (size_t)P;
    HIPCHK(hipMemcpyAsync(ti, pose_Tcw, i_K, hipMemcpyHostToDevice, call.s));
    if (cam_K) HIPCHK(hipMemcpyAsync(ti + i_K, cam_K, sizeof(double) * 4 * (size_t)P, hipMemcpyHostToDevice, call.s));
    a->n_poses = P;
    a->pose = (const double*)ti;
    a->cam_K = cam_K ? (const double*)(ti + i_K) : nullptr;
    return LH_OK;
}

int32_t tri_count_accepted(const uint8_t* flags, int n) {
    int32_t c = 0;
    for (int i = 0; i < n; ++i) c += flags[i] == 0;
    return c;
}

int triangulate_impl(lh_handle* h, const lh_tri_input* in, lh_tri_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const int n = in->n_points, P = in->n_poses;
    if (n < 0) return LH_E_BADARG;
    out->n_accepted = 0;
    out->time_ms = 0.0;
    if (n == 0) return LH_OK;
    if (P < 1 || !in->pose_Tcw || !in->view_xy || !out->pt || !out->flags) return LH_E_BADARG;
    if (in->view_ptr && !in->view_pose) return LH_E_BADARG;
    int64_t nv;
    if (in->view_ptr) {
        if (in->view_ptr[0] < 0) return LH_E_BADARG;
        for (int i = 0; i < n; ++i)
            if (in->view_ptr[i + 1] - in->view_ptr[i] < 2) return LH_E_BADARG;   // fewer than 2 views, or decreasing
        nv = in->view_ptr[n];
        for (int64_t v = in->view_ptr[0]; v < nv; ++v)
            if (in->view_pose[v] >= (uint32_t)P) return LH_E_BADARG;
    } else {
        if (P < 2) return LH_E_BADARG;
        nv = (int64_t)n * P;
    }
    FrontendCall call(h);
    STAGE(call.select());
    hipStream_t s = call.s;
    // input arena: doubles first, then the int64 CSR, then the 32-bit pose indices
    const size_t i_K = sizeof(double) * 12 * (size_t)P;
    const size_t i_xy = i_K + sizeof(double) * 4 * (size_t)P;
    const size_t i_ptr = i_xy + sizeof(double) * 2 * (size_t)nv;
    const size_t i_vp = i_ptr + (in->view_ptr ? sizeof(int64_t) * ((size_t)n + 1) : 0);
    const size_t i_end = i_vp + (in->view_ptr ? sizeof(uint32_t) * (size_t)nv : 0);
    HIPCHK(h->fe.t_in.ensure(i_end));
    uint8_t* ti = h->fe.t_in.p;
    lh_tri_args a{};
    const TriOut o((size_t)n);
    STAGE(tri_outputs(h, &a, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out, o));
    STAGE(tri_poses(call, &a, P, in->pose_Tcw, in->cam_K));
    HIPCHK(hipMemcpyAsync(ti + i_xy, in->view_xy, i_ptr - i_xy, hipMemcpyHostToDevice, s));
    if (in->view_ptr) {
        HIPCHK(hipMemcpyAsync(ti + i_ptr, in->view_ptr, i_vp - i_ptr, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ti + i_vp, in->view_pose, i_end - i_vp, hipMemcpyHostToDevice, s));
    }
    a.n_points = n;
    a.view_xy = (const double*)(ti + i_xy);
    a.view_ptr = in->view_ptr ? (const int64_t*)(ti + i_ptr) : nullptr;
    a.view_pose = in->view_ptr ? (const uint32_t*)(ti + i_vp) : nullptr;
    STAGE(call.start());
    HIPCHK(lh_launch_triangulate(s, &a));
    STAGE(call.stop());
    HIPCHK(hipMemcpyAsync(out->pt, a.pt, o.o_ratio, hipMemcpyDeviceToHost, s));
    if (out->sing_ratio) HIPCHK(hipMemcpyAsync(out->sing_ratio, a.ratio, o.o_flag - o.o_ratio, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->flags, a.flags, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    STAGE(call.time(&out->time_ms));
    out->n_accepted = tri_count_accepted(out->flags, n);
    return LH_OK;
}

// a tracker's launches (lk_enqueue or klt_enqueue) left -> right are enqueued: k_triangulate on kp1 / kp2 / success where
// the tracker left them, then one download.  In: lh_stereo_input or lh_klt_stereo_input (one set of field names)
template <typename In>
int stereo_finish(FrontendCall& call, int n, const In* in, lh_stereo_result* out) {
    lh_handle* h = call.h;
    hipStream_t s = call.s;
    HIPCHK(h->fe.t_in.ensure(sizeof(double) * (12 + 4) * 2));
    lh_tri_args a{};
    const TriOut o((size_t)n);
    STAGE(tri_outputs(h, &a, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out, o));
    STAGE(tri_poses(call, &a, 2, in->pose_Tcw, in->cam_K));
    a.n_points = n;
    a.kp1 = h->fe.k_kp1.p;
    a.kp2 = h->fe.k_kp2.p;
    a.success = h->fe.k_succ.p;
    HIPCHK(lh_launch_triangulate(s, &a));
    STAGE(call.stop());
    if (n > 0) {
        STAGE(lk_download(call, n, out->kp2, out->success));
        HIPCHK(hipMemcpyAsync(out->pt, a.pt, o.o_ratio, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->flags, a.flags, (size_t)n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    STAGE(call.time(&out->time_ms));
    out->n_accepted = tri_count_accepted(out->flags, n);
    return LH_OK;
}

// lh_lk_track left -> right, then the triangulation
int stereo_landmarks_impl(lh_handle* h, const lh_stereo_input* in, lh_stereo_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const int n = in->lk.n_points;
    if (!in->pose_Tcw || (n > 0 && (!out->pt || !out->flags))) return LH_E_BADARG;
    out->n_accepted = 0;
    FrontendCall call(h);
    STAGE(lk_enqueue(call, &in->lk, out->kp2, out->success));
    return stereo_finish(call, n, in, out);
}

// lh_klt_track (n_points > 0): upload both images and the keypoints into the tracker's buffers (lh_lk_track's: a handle
// runs one tracker at a time), build the pyramids (k_klt_pyr per level and image, levels 1.. packed), track
// (k_klt_track); it starts the call's timing in front of the first kernel.  kp2 (host): the guess when in->has_initial.
int klt_enqueue(FrontendCall& call, const lh_klt_input* in, const float* kp2) {
    const int n = in->n_points;
    STAGE(call.select());
    const size_t total = klt_pyramid_bytes(in->cols, in->rows, in->max_level, in->step);
    hipStream_t s = call.s;
    FrontendState& fe = call.h->fe;
    HIPCHK(fe.k_img[0].ensure(total));
    HIPCHK(fe.k_img[1].ensure(total));
    HIPCHK(fe.k_kp1.ensure(2 * (size_t)n));
    HIPCHK(fe.k_kp2.ensure(2 * (size_t)n));
    HIPCHK(fe.k_succ.ensure((size_t)n));
    // as lk_enqueue: the caller's last row guarantees only `cols` readable bytes.  No tap reads a row's padding (every
    // read is at a REFLECT_101 index inside [0, cols)), so the last row's tail stays as the buffer has it
    const size_t img_bytes = (size_t)(in->rows - 1) * (size_t)in->step + (size_t)in->cols;
    for (int im = 0; im < 2; ++im)
        HIPCHK(hipMemcpyAsync(fe.k_img[im].p, im ? in->img2 : in->img1, img_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(fe.k_kp1.p, in->kp1, 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    if (in->has_initial) HIPCHK(hipMemcpyAsync(fe.k_kp2.p, kp2, 2 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    lh_klt_args a = klt_args(*in, fe.k_img[0].p, fe.k_img[1].p, in->step, in->has_initial ? 1 : 0);
    a.n_points = n;
    a.kp1 = fe.k_kp1.p;
    a.kp2 = fe.k_kp2.p;
    a.success = fe.k_succ.p;
    STAGE(call.start());
    return klt_pyr_track(s, a, 1);
}

int klt_track_impl(lh_handle* h, const lh_klt_input* in, lh_lk_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    STAGE(klt_check(in, out->kp2, out->success));
    out->time_ms = 0.0;
    if (in->n_points == 0) return LH_OK;
    FrontendCall call(h);
    STAGE(klt_enqueue(call, in, out->kp2));
    STAGE(call.stop());
    STAGE(lk_download(call, in->n_points, out->kp2, out->success));
    HIPCHK(hipStreamSynchronize(call.s));
    return call.time(&out->time_ms);
}

// lh_klt_track left -> right, then the triangulation
int klt_stereo_landmarks_impl(lh_handle* h, const lh_klt_stereo_input* in, lh_stereo_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const int n = in->klt.n_points;
    STAGE(klt_check(&in->klt, out->kp2, out->success));
    if (!in->pose_Tcw || (n > 0 && (!out->pt || !out->flags))) return LH_E_BADARG;
    out->n_accepted = 0;
    out->time_ms = 0.0;
    if (n == 0) return LH_OK;
    FrontendCall call(h);
    STAGE(klt_enqueue(call, &in->klt, out->kp2));
    return stereo_finish(call, n, in, out);
}

int detect_features_impl(lh_handle* h, const lh_detect_input* in, lh_detect_result* out) {
    if (!h || !in || !out || !in->img) return LH_E_BADARG;
    const int cols = in->cols, rows = in->rows;
    if (!image_ok(cols, rows, in->step)) return LH_E_BADARG;
    if (in->mask && in->mask_step < cols) return LH_E_BADARG;
    if (in->n_exclude < 0 || (in->n_exclude > 0 && !in->exclude_pt)) return LH_E_BADARG;
    if (out->kp_capacity < 0 || (out->kp_capacity > 0 && !out->kp)) return LH_E_BADARG;
    if (in->max_corners > 0 && out->kp_capacity < in->max_corners) return LH_E_BADARG;
    if (!(in->quality_level >= 0.0) || !(in->min_distance >= 0.0)) return LH_E_BADARG;
    out->n_corners = out->n_candidates = 0;
    out->lambda_max = 0.0;
    out->time_ms = 0.0;
    FrontendCall call(h);
    STAGE(call.select());
    hipStream_t s = call.s;
    FrontendState& fe = h->fe;
    const size_t px = (size_t)rows * (size_t)cols;
    const int limit = in->max_corners > 0 ? in->max_corners : out->kp_capacity;
    lh_gftt_args a{};
    STAGE(gftt_prepare(fe, cols, rows, in->quality_level, in->min_distance, limit, &a));
    HIPCHK(fe.g_img.ensure(px));
    HIPCHK(fe.g_excl.ensure(2 * (size_t)std::max(in->n_exclude, 1)));
    HIPCHK(fe.g_kp.ensure(2 * (size_t)std::max(limit, 1)));
    HIPCHK(upload_rows(s, fe.g_img.p, in->img, cols, rows, in->step));
    if (in->mask)
        HIPCHK(upload_rows(s, fe.g_allow.p, in->mask, cols, rows, in->mask_step));
    else
        HIPCHK(hipMemsetAsync(fe.g_allow.p, 1, px, s));
    if (in->n_exclude > 0)
        HIPCHK(hipMemcpyAsync(fe.g_excl.p, in->exclude_pt, 2 * sizeof(float) * (size_t)in->n_exclude, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(fe.g_ctl.p, 0, sizeof(lh_gftt_ctl), s));
    a.img = fe.g_img.p;
    a.n_exclude = in->n_exclude; a.exclude_pt = fe.g_excl.p; a.exclude_half = in->exclude_half;
    a.kp = fe.g_kp.p;
    STAGE(call.start());
    STAGE(gftt_select(call, a));
    STAGE(call.stop());
    const lh_gftt_ctl& ctl = *fe.s_gctl.p;
    HIPCHK(hipMemcpyAsync(fe.s_gctl.p, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    if (out->eig) HIPCHK(hipMemcpyAsync(out->eig, a.eig, sizeof(double) * px, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const int64_t n_written = std::min<int64_t>(ctl.n_acc, limit);
    if (n_written > 0) {
        HIPCHK(hipMemcpyAsync(out->kp, a.kp, 2 * sizeof(float) * (size_t)n_written, hipMemcpyDeviceToHost, s));
        if (out->response)
            HIPCHK(hipMemcpyAsync(out->response, a.response, sizeof(double) * (size_t)n_written, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    STAGE(call.time(&out->time_ms));
    out->n_corners = in->max_corners > 0 ? (int32_t)n_written : (int32_t)ctl.n_acc;
    out->n_candidates = (int32_t)ctl.n_cand;
    out->lambda_max = ctl.max_key ? lh_gftt_unkey(ctl.max_key) : 0.0;
    return LH_OK;
}

}  // namespace

extern "C" {

int lh_estimate_pose(lh_handle* h, const lh_frames* in, lh_frames_result* out) {
    return no_throw(estimate_pose_impl, h, in, out);
}
int lh_lk_track(lh_handle* h, const lh_lk_input* in, lh_lk_result* out) { return no_throw(lk_track_impl, h, in, out); }
int lh_triangulate(lh_handle* h, const lh_tri_input* in, lh_tri_result* out) {
    return no_throw(triangulate_impl, h, in, out);
}
int lh_stereo_landmarks(lh_handle* h, const lh_stereo_input* in, lh_stereo_result* out) {
    return no_throw(stereo_landmarks_impl, h, in, out);
}
int lh_detect_features(lh_handle* h, const lh_detect_input* in, lh_detect_result* out) {
    return no_throw(detect_features_impl, h, in, out);
}
int lh_klt_track(lh_handle* h, const lh_klt_input* in, lh_lk_result* out) { return no_throw(klt_track_impl, h, in, out); }
int lh_klt_stereo_landmarks(lh_handle* h, const lh_klt_stereo_input* in, lh_stereo_result* out) {
    return no_throw(klt_stereo_landmarks_impl, h, in, out);
}

}  // extern "C"
