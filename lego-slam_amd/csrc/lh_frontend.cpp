// lh_frontend.cpp — the frontend entry points of the C ABI (include/lego_ba.h) on the solver's handle and stream:
// lh_estimate_pose, lh_lk_track, lh_klt_track, lh_triangulate, lh_stereo_landmarks, lh_klt_stereo_landmarks,
// lh_detect_features, lh_track_frame, lh_insert_keyframe.  Each checks its arguments,
// grows its buffers (lh_handle.h FrontendState), enqueues copies and kernels, synchronises and copies out.
#include <cmath>

#include "lh_handle.h"
#include "lh_launch.h"

using namespace lh;

namespace {

// One frontend call on the handle's stream: the device selection, the two events around its kernels (start() in front
// of the first, stop() behind the last), time_ms once the stream has drained, and on every way out (the error returns
// included) the handle's event pool put back.
struct FrontendCall {
    lh_handle* h;
    hipStream_t s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit FrontendCall(lh_handle* hh) : h(hh), s(hh->stream) {}
    ~FrontendCall() { h->event_next = 0; }
    int select() { return hipSetDevice(h->device) == hipSuccess ? LH_OK : LH_E_HIP; }
    int record(hipEvent_t* e) {
        if (!(*e = next_event(h))) return LH_E_HIP;
        HIPCHK(hipEventRecord(*e, s));
        return LH_OK;
    }
    int start() { return record(&e0); }
    int stop() { return record(&e1); }
    int time(double* time_ms) {   // after the call's last synchronise
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *time_ms = ms;
        return LH_OK;
    }
};

// the staging copies build std::vectors (par_copy): no exception crosses the ABI
template <typename In, typename Out>
int no_throw(int (*impl)(lh_handle*, const In*, Out*), lh_handle* h, const In* in, Out* out) {
    try {
        return impl(h, in, out);
    } catch (...) {
        return LH_E_HIP;
    }
}

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
    // arena layouts (16-byte aligned segments)
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const bool has_flag = in->is_outlier && O > 0;
    const size_t i_ptr = 0, i_pose = al(sizeof(int64_t) * (F + 1)), i_pts = i_pose + al(sizeof(double) * 12 * (size_t)F),
                 i_uv = i_pts + al(sizeof(double) * 3 * (size_t)O), i_flag = i_uv + al(sizeof(double) * 2 * (size_t)O),
                 i_end = i_flag + (has_flag ? al((size_t)O) : 0);
    const size_t o_pose = 0, o_rchi2 = al(sizeof(double) * 12 * (size_t)F), o_iters = o_rchi2 + al(sizeof(double) * (size_t)O),
                 o_inl = o_iters + al(sizeof(int32_t) * (size_t)F), o_flag = o_inl + al(sizeof(int32_t) * (size_t)F),
                 o_end = o_flag + al((size_t)O);
    HIPCHK(fe.f_in.ensure(i_end));
    HIPCHK(fe.f_out.ensure(o_end));
    HIPCHK(fe.f_res.ensure(2 * (size_t)O));
    HIPCHK(fe.s_fin.ensure(i_end));
    HIPCHK(fe.s_fout.ensure(o_end));
    {
        uint8_t* st = fe.s_fin.p;
        const ByteSeg seg[5] = {{st + i_ptr, in->obs_ptr, sizeof(int64_t) * (F + 1)},
                                {st + i_pose, in->pose_Tcw, sizeof(double) * 12 * (size_t)F},
                                {st + i_pts, in->pts_w, sizeof(double) * 3 * (size_t)O},
                                {st + i_uv, in->obs_uv, sizeof(double) * 2 * (size_t)O},
                                {st + i_flag, in->is_outlier, has_flag ? (size_t)O : 0}};
        par_copy(h, seg, 5);
    }
    HIPCHK(hipMemcpyAsync(fe.f_in.p, fe.s_fin.p, i_end, hipMemcpyHostToDevice, s));
    uint8_t *fi = fe.f_in.p, *fo = fe.f_out.p;
    const lh_params prm = frames_params(h, in->K);
    STAGE(call.start());
    HIPCHK(lh_launch_frames(s, F, (const int64_t*)(fi + i_ptr), (const double*)(fi + i_pose),
                            (const double*)(fi + i_pts), (const double*)(fi + i_uv), has_flag ? fi + i_flag : nullptr,
                            prm, fe.f_res.p, (double*)(fo + o_pose), fo + o_flag, (double*)(fo + o_rchi2),
                            (int32_t*)(fo + o_iters), (int32_t*)(fo + o_inl)));
    STAGE(call.stop());
    // one download of what the caller asked for: the pose block always, the rest up to the last wanted
    const size_t want = out->is_outlier && O > 0 ? o_end
                        : out->n_inliers         ? o_flag
                        : out->iterations        ? o_inl
                        : out->edge_chi2 && O > 0 ? o_iters
                                                 : o_rchi2;
    HIPCHK(hipMemcpyAsync(fe.s_fout.p, fo, want, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    {
        const uint8_t* st = fe.s_fout.p;
        const ByteSeg seg[5] = {{out->pose_Tcw, st + o_pose, sizeof(double) * 12 * (size_t)F},
                                {out->edge_chi2, st + o_rchi2, out->edge_chi2 ? sizeof(double) * (size_t)O : 0},
                                {out->iterations, st + o_iters, out->iterations ? sizeof(int32_t) * (size_t)F : 0},
                                {out->n_inliers, st + o_inl, out->n_inliers ? sizeof(int32_t) * (size_t)F : 0},
                                {out->is_outlier, st + o_flag, out->is_outlier ? (size_t)O : 0}};
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

// legoslam::triangulation (algorithm.h:11-34) for a batch of points (k_triangulate, lh_tri.hip).
// The fields lh_triangulate and lh_stereo_landmarks share: threshold, gate, T_out, and the output arena
// (pt [n][3], sing_ratio [n], flags [n]).
struct TriOut { size_t o_ratio, o_flag, o_end; };
void tri_tests(lh_tri_args* a, double thr, int gate, double y_max, double z_min, double z_max, const double* T_out) {
    a->thr = thr;
    a->gate = gate ? 1 : 0;
    a->y_max = y_max; a->z_min = z_min; a->z_max = z_max;
    a->has_T = T_out ? 1 : 0;
    for (int i = 0; i < 12; ++i) a->T[i] = T_out ? T_out[i] : 0.0;
}
int tri_outputs(lh_handle* h, lh_tri_args* a, int n, double thr, int gate, double y_max, double z_min,
                double z_max, const double* T_out, TriOut* o) {
    o->o_ratio = sizeof(double) * 3 * (size_t)n;
    o->o_flag = o->o_ratio + sizeof(double) * (size_t)n;
    o->o_end = o->o_flag + (size_t)n;
    HIPCHK(h->fe.t_out.ensure(o->o_end));
    tri_tests(a, thr, gate, y_max, z_min, z_max, T_out);
    a->pt = (double*)h->fe.t_out.p;
    a->ratio = (double*)(h->fe.t_out.p + o->o_ratio);
    a->flags = h->fe.t_out.p + o->o_flag;
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
    TriOut o;
    STAGE(tri_outputs(h, &a, n, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out, &o));
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
    TriOut o;
    STAGE(tri_outputs(h, &a, n, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out, &o));
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

// cv::calcOpticalFlowPyrLK as lh_klt.h defines it (include/lego_ba.h).  klt_check: the argument
// errors.  klt_enqueue (n_points > 0): upload both images and the keypoints into the tracker's buffers (lh_lk_track's:
// a handle runs one tracker at a time), build the pyramids (k_klt_pyr per level and image, levels 1.. packed), track
// (k_klt_track); it starts the call's timing in front of the first kernel.  kp2 (host): the guess when in->has_initial.
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

int klt_enqueue(FrontendCall& call, const lh_klt_input* in, const float* kp2) {
    const int n = in->n_points;
    STAGE(call.select());
    lh_klt_args a{};
    a.n_levels = lh_klt_level_sizes(in->cols, in->rows, in->max_level, a.I.cols, a.I.rows);
    const int64_t total = klt_pyramid_layout(&a.I, a.n_levels, nullptr, in->step);
    hipStream_t s = call.s;
    FrontendState& fe = call.h->fe;
    HIPCHK(fe.k_img[0].ensure((size_t)total));
    HIPCHK(fe.k_img[1].ensure((size_t)total));
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
    a.J = a.I;
    klt_pyramid_layout(&a.I, a.n_levels, fe.k_img[0].p, in->step);
    klt_pyramid_layout(&a.J, a.n_levels, fe.k_img[1].p, in->step);
    a.n_points = n;
    a.kp1 = fe.k_kp1.p;
    a.kp2 = fe.k_kp2.p;
    a.success = fe.k_succ.p;
    a.has_initial = in->has_initial ? 1 : 0;
    a.max_iters = in->max_iters;
    a.eps2 = in->epsilon * in->epsilon;
    a.min_eig = in->min_eig_threshold;
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

// Frontend::Track (frontend_lego.cpp:48-75) in one call (include/lego_ba.h): upload img2 (and img1,
// unless the resident image stands in for it) and one arena; k_track_guess, the tracker's kernels, k_track_pack and
// k_frames behind one another on the device buffers; one download; one synchronise.  The edge count stays on the
// device until then: k_frames reads it from the obs_ptr k_track_pack wrote.
int track_frame_impl(lh_handle* h, const lh_track_input* in, lh_track_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const lh_klt_input& k = in->klt;
    const int n = k.n_points, cols = k.cols, rows = k.rows;
    {
        lh_klt_input chk = k;   // lh_klt_track's argument checks; a null img1 is the resident image
        if (!chk.img1) chk.img1 = chk.img2;
        STAGE(klt_check(&chk, out->kp2, out->success));
    }
    if (n > 0 && !in->pts_w) {
        if (!in->has_point) return LH_E_BADARG;
        for (int i = 0; i < n; ++i)
            if (in->has_point[i]) return LH_E_BADARG;
    }
    FrontendState& fe = h->fe;
    if (n > 0 && !k.img1 && !(fe.r_valid && fe.r_cols == cols && fe.r_rows == rows)) return LH_E_STATE;
    for (int i = 0; i < 12; ++i) out->pose_Tcw[i] = in->pose_Tcw[i];
    out->n_tracked = out->n_edges = out->n_inliers = out->iterations = 0;
    out->time_ms = 0.0;
    if (n == 0 && !k.img2) return LH_OK;
    FrontendCall call(h);
    STAGE(call.select());
    hipStream_t s = call.s;
    // from here on the resident image is in the making: valid again once the call has succeeded
    const int slot_I = fe.r_cur, slot_J = 1 - fe.r_cur;
    const int have_I = n == 0 ? LH_KLT_MAX_LEVELS : k.img1 ? 1 : fe.r_levels;   // I's first level to build (n == 0: no I)
    fe.r_valid = false;
    lh_klt_args a{};
    {
        lh_klt_levels full{};   // the buffers hold every level, whatever max_level a call asks for
        const int n_full = lh_klt_level_sizes(cols, rows, LH_KLT_MAX_LEVELS - 1, full.cols, full.rows);
        const size_t bytes = (size_t)klt_pyramid_layout(&full, n_full, nullptr, cols);
        HIPCHK(fe.r_img[slot_J].ensure(bytes));
        if (n > 0) HIPCHK(fe.r_img[slot_I].ensure(bytes));   // no change of a resident image: its size is this one
    }
    a.n_levels = lh_klt_level_sizes(cols, rows, k.max_level, a.I.cols, a.I.rows);
    a.J = a.I;
    klt_pyramid_layout(&a.I, a.n_levels, fe.r_img[slot_I].p, cols);
    klt_pyramid_layout(&a.J, a.n_levels, fe.r_img[slot_J].p, cols);
    // arena layouts (16-byte aligned segments)
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t N = (size_t)n;
    const size_t i_pose = 0, i_pts = al(sizeof(double) * 12), i_kp1 = i_pts + al(sizeof(double) * 3 * N),
                 i_hp = i_kp1 + al(sizeof(float) * 2 * N), i_end = i_hp + (in->has_point ? al(N) : 0);
    const size_t o_pose = 0, o_cnt = al(sizeof(double) * 12), o_kp2 = o_cnt + al(sizeof(int32_t) * 4),
                 o_succ = o_kp2 + al(sizeof(float) * 2 * N), o_idx = o_succ + al(N), o_flag = o_idx + al(sizeof(int32_t) * N),
                 o_chi = o_flag + al(N), o_end = o_chi + al(sizeof(double) * N);
    const size_t w_ptr = 0, w_pts = al(sizeof(int64_t) * 2), w_uv = w_pts + al(sizeof(double) * 3 * N),
                 w_end = w_uv + al(sizeof(double) * 2 * N);
    if (n > 0) {
        HIPCHK(fe.tk_in.ensure(i_end));
        HIPCHK(fe.tk_out.ensure(o_end));
        HIPCHK(fe.tk_work.ensure(w_end));
        HIPCHK(fe.f_res.ensure(2 * N));
        HIPCHK(fe.s_tkin.ensure(i_end));
        HIPCHK(fe.s_tkout.ensure(o_end));
    }
    HIPCHK(upload_rows(s, fe.r_img[slot_J].p, k.img2, cols, rows, k.step));
    if (n > 0 && k.img1) HIPCHK(upload_rows(s, fe.r_img[slot_I].p, k.img1, cols, rows, k.step));
    lh_track_args t{};
    uint8_t *ti = fe.tk_in.p, *to = fe.tk_out.p, *tw = fe.tk_work.p;
    if (n > 0) {
        uint8_t* st = fe.s_tkin.p;
        const ByteSeg seg[4] = {{st + i_pose, in->pose_Tcw, sizeof(double) * 12},
                                {st + i_pts, in->pts_w, in->pts_w ? sizeof(double) * 3 * N : 0},
                                {st + i_kp1, k.kp1, sizeof(float) * 2 * N},
                                {st + i_hp, in->has_point, in->has_point ? N : 0}};
        par_copy(h, seg, 4);
        HIPCHK(hipMemcpyAsync(ti, st, i_end, hipMemcpyHostToDevice, s));
        t.n_points = n;
        t.kp1 = (const float*)(ti + i_kp1);
        t.pts_w = (const double*)(ti + i_pts);
        t.has_point = in->has_point ? ti + i_hp : nullptr;
        for (int i = 0; i < 12; ++i) { t.pose[i] = in->pose_Tcw[i]; t.ext[i] = in->cam_ext[i]; }
        for (int i = 0; i < 4; ++i) t.K[i] = in->K[i];
        t.kp2 = (float*)(to + o_kp2);
        t.success = to + o_succ;
        t.obs_ptr = (int64_t*)(tw + w_ptr);
        t.pts = (double*)(tw + w_pts);
        t.uv = (double*)(tw + w_uv);
        t.edge_feature = (int32_t*)(to + o_idx);
        t.counts = (int32_t*)(to + o_cnt);
        a.n_points = n;
        a.kp1 = t.kp1;
        a.kp2 = t.kp2;
        a.success = to + o_succ;
        a.has_initial = 1;
        a.max_iters = k.max_iters;
        a.eps2 = k.epsilon * k.epsilon;
        a.min_eig = k.min_eig_threshold;
    }
    STAGE(call.start());
    HIPCHK(lh_launch_track_guess(s, &t));
    STAGE(klt_pyr_track(s, a, have_I));
    if (n > 0) {
        HIPCHK(lh_launch_track_pack(s, &t));
        HIPCHK(lh_launch_frames(s, 1, t.obs_ptr, (const double*)(ti + i_pose), t.pts, t.uv, nullptr, frames_params(h, in->K),
                                fe.f_res.p, (double*)(to + o_pose), to + o_flag, (double*)(to + o_chi), t.counts + 2,
                                t.counts + 3));
    }
    STAGE(call.stop());
    if (n > 0) {   // one download, up to the last output the caller asked for
        const size_t want = out->edge_chi2 ? o_end : out->is_outlier ? o_chi : o_idx;
        HIPCHK(hipMemcpyAsync(fe.s_tkout.p, to, want, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (n > 0) {
        const uint8_t* st = fe.s_tkout.p;
        const int32_t* cnt = (const int32_t*)(st + o_cnt);
        const int32_t m = cnt[1];
        if (m < 0 || m > n) return LH_E_HIP;
        const ByteSeg seg[3] = {{out->pose_Tcw, st + o_pose, sizeof(double) * 12},
                                {out->kp2, st + o_kp2, sizeof(float) * 2 * N},
                                {out->success, st + o_succ, N}};
        par_copy(h, seg, 3);
        out->n_tracked = cnt[0];
        out->n_edges = m;
        out->iterations = cnt[2];
        out->n_inliers = cnt[3];
        // the edges' outputs back to their features
        const int32_t* idx = (const int32_t*)(st + o_idx);
        if (out->is_outlier) {
            std::fill(out->is_outlier, out->is_outlier + n, (uint8_t)0);
            for (int32_t e = 0; e < m; ++e) out->is_outlier[idx[e]] = st[o_flag + e];
        }
        if (out->edge_chi2) {
            std::fill(out->edge_chi2, out->edge_chi2 + n, 0.0);
            const double* chi = (const double*)(st + o_chi);
            for (int32_t e = 0; e < m; ++e) out->edge_chi2[idx[e]] = chi[e];
        }
    }
    STAGE(call.time(&out->time_ms));
    fe.r_cur = slot_J;
    fe.r_cols = cols;
    fe.r_rows = rows;
    fe.r_levels = a.n_levels;
    fe.r_valid = true;
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

int detect_features_impl(lh_handle* h, const lh_detect_input* in, lh_detect_result* out) {
    if (!h || !in || !out || !in->img) return LH_E_BADARG;
    const int cols = in->cols, rows = in->rows;
    if (cols < 3 || rows < 3 || in->step < cols || (int64_t)rows * cols > INT32_MAX) return LH_E_BADARG;
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

// Frontend::InsertKeyframe's and StereoInit's chain (frontend_lego.cpp:77-102, :323-362) in one call (include/lego_ba.h,
// DESIGN.md 2.5e): upload img_right (and img_left, unless the resident image stands in for it) and one arena; the
// detector on level 0 of the resident pyramid, k_kf_assemble, the tracker's kernels, k_triangulate and k_kf_finish behind
// one another on the device buffers; one download.  The corner count stays on the device until then: every launch
// behind the detector is sized for n_have + max_corners slots (lh_keyframe.h).  The host waits where the detector
// always has, between batches of selection rounds, and once at the end.
int insert_keyframe_impl(lh_handle* h, const lh_keyframe_input* in, lh_keyframe_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    const int cols = in->cols, rows = in->rows, nh = in->n_have, mc = in->max_corners;
    // lh_detect_features' argument errors (mask == NULL), then lh_klt_track's
    if (cols < 3 || rows < 3 || in->step < cols || (int64_t)rows * cols > INT32_MAX) return LH_E_BADARG;
    if (nh < 0 || (nh > 0 && !in->have_kp) || mc <= 0 || (int64_t)nh + mc > LH_KF_MAX_FEATURES) return LH_E_BADARG;
    if (!(in->quality_level >= 0.0) || !(in->min_distance >= 0.0)) return LH_E_BADARG;
    if (!in->img_right || !out->kp_new || !out->kp_right || !out->success || !out->pt || !out->flags) return LH_E_BADARG;
    const int cap = nh + mc;
    lh_klt_input k{};
    k.cols = cols; k.rows = rows; k.step = in->step;
    k.img1 = k.img2 = in->img_right;   // a null img_left is the resident image
    k.n_points = cap;
    k.kp1 = out->kp_right;             // (the list is made on the device: any non-null pointer passes the check)
    k.max_level = in->max_level; k.max_iters = in->max_iters;
    k.epsilon = in->epsilon; k.min_eig_threshold = in->min_eig_threshold;
    STAGE(klt_check(&k, out->kp_right, out->success));
    if (nh > 0 && !in->have_pts_w) {
        if (!in->have_point) return LH_E_BADARG;
        for (int i = 0; i < nh; ++i)
            if (in->have_point[i]) return LH_E_BADARG;
    }
    FrontendState& fe = h->fe;
    if (!in->img_left && !(fe.r_valid && fe.r_cols == cols && fe.r_rows == rows)) return LH_E_STATE;
    out->n_new = out->n_candidates = out->n_right = out->n_accepted = 0;
    out->lambda_max = 0.0;
    out->time_ms = 0.0;
    FrontendCall call(h);
    STAGE(call.select());
    hipStream_t s = call.s;
    const int slot = fe.r_cur;
    const int have_I = in->img_left ? 1 : fe.r_levels;   // the left pyramid's first level to build
    lh_klt_levels full{};   // as lh_track_frame: the pyramid buffers hold every level, whatever max_level a call asks for
    const int n_full = lh_klt_level_sizes(cols, rows, LH_KLT_MAX_LEVELS - 1, full.cols, full.rows);
    const size_t pyr_bytes = (size_t)klt_pyramid_layout(&full, n_full, nullptr, cols);
    HIPCHK(fe.kf_right.ensure(pyr_bytes));
    // arena layouts (16-byte aligned segments).  The upload ends with have_kp, the head of the feature list, and the
    // device arena goes on for the corners behind it
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t NH = (size_t)nh, CAP = (size_t)cap;
    const size_t i_cam = 0, i_K = sizeof(double) * 24, i_pts = i_K + sizeof(double) * 8,
                 i_hp = i_pts + al(sizeof(double) * 3 * NH), i_kl = i_hp + (in->have_point ? al(NH) : 0),
                 i_up = i_kl + sizeof(float) * 2 * NH, i_end = i_kl + sizeof(float) * 2 * CAP;
    const size_t o_cnt = 0, o_lam = sizeof(int32_t) * 4, o_pt = 32, o_kpr = o_pt + al(sizeof(double) * 3 * CAP),
                 o_new = o_kpr + al(sizeof(float) * 2 * CAP), o_succ = o_new + al(sizeof(float) * 2 * (size_t)mc),
                 o_flag = o_succ + al(CAP), o_end = o_flag + al(CAP);
    HIPCHK(fe.kf_in.ensure(i_end));
    HIPCHK(fe.kf_out.ensure(o_end));
    HIPCHK(fe.kf_state.ensure(CAP));
    HIPCHK(fe.s_kfin.ensure(i_up));
    HIPCHK(fe.s_kfout.ensure(o_end));
    lh_gftt_args g{};
    STAGE(gftt_prepare(fe, cols, rows, in->quality_level, in->min_distance, mc, &g));
    // Every buffer of the call's own is there.  From here on the resident image is in the making (a given img_left
    // replaces it, its buffer first if that has to grow; then the enqueueing begins): valid again once the call has
    // succeeded.  A resident image that stays has this call's size, and its buffer every level's room.
    fe.r_valid = false;
    if (in->img_left) HIPCHK(fe.r_img[slot].ensure(pyr_bytes));
    lh_klt_args a{};
    a.n_levels = lh_klt_level_sizes(cols, rows, in->max_level, a.I.cols, a.I.rows);
    a.J = a.I;
    klt_pyramid_layout(&a.I, a.n_levels, fe.r_img[slot].p, cols);
    klt_pyramid_layout(&a.J, a.n_levels, fe.kf_right.p, cols);
    HIPCHK(upload_rows(s, fe.kf_right.p, in->img_right, cols, rows, in->step));
    if (in->img_left) HIPCHK(upload_rows(s, fe.r_img[slot].p, in->img_left, cols, rows, in->step));
    uint8_t *ki = fe.kf_in.p, *ko = fe.kf_out.p;
    {
        uint8_t* st = fe.s_kfin.p;
        const ByteSeg seg[5] = {{st + i_cam, in->cam_pose, sizeof(double) * 24},
                                {st + i_K, in->cam_K, sizeof(double) * 8},
                                {st + i_pts, in->have_pts_w, in->have_pts_w ? sizeof(double) * 3 * NH : 0},
                                {st + i_hp, in->have_point, in->have_point ? NH : 0},
                                {st + i_kl, in->have_kp, sizeof(float) * 2 * NH}};
        par_copy(h, seg, 5);
        HIPCHK(hipMemcpyAsync(ki, st, i_up, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemsetAsync(fe.g_allow.p, 1, (size_t)rows * (size_t)cols, s));
    HIPCHK(hipMemsetAsync(fe.g_ctl.p, 0, sizeof(lh_gftt_ctl), s));
    float* kl = (float*)(ki + i_kl);
    g.img = fe.r_img[slot].p;   // level 0 of the resident pyramid: rows packed to cols, the layout g_img has
    g.n_exclude = nh; g.exclude_pt = kl; g.exclude_half = in->exclude_half;
    g.kp = kl + 2 * NH;         // the corners straight into the feature list, behind have_kp
    lh_kf_args f{};
    f.n_have = nh; f.max_corners = mc;
    f.ctl = g.ctl;
    f.pts_w = (const double*)(ki + i_pts);
    f.has_point = in->have_point ? ki + i_hp : nullptr;
    for (int i = 0; i < 12; ++i) { f.pose[i] = in->pose_Tcw[i]; f.ext[i] = in->cam_pose[1][i]; }
    for (int i = 0; i < 4; ++i) f.K[i] = in->cam_K[1][i];
    f.kl = kl;
    f.kp_right = (float*)(ko + o_kpr);
    f.state = fe.kf_state.p;
    f.kp_new = (float*)(ko + o_new);
    f.success = ko + o_succ;
    f.pt = (double*)(ko + o_pt);
    f.flags = ko + o_flag;
    f.counts = (int32_t*)(ko + o_cnt);
    f.lambda_max = (double*)(ko + o_lam);
    a.n_points = cap;
    a.kp1 = kl;
    a.kp2 = f.kp_right;
    a.success = ko + o_succ;
    a.has_initial = 1;
    a.max_iters = in->max_iters;
    a.eps2 = in->epsilon * in->epsilon;
    a.min_eig = in->min_eig_threshold;
    lh_tri_args t{};
    tri_tests(&t, in->sing_ratio_thr, in->gate, in->y_max, in->z_min, in->z_max, in->T_out);
    t.n_points = cap; t.n_poses = 2;
    t.pose = (const double*)(ki + i_cam);
    t.cam_K = (const double*)(ki + i_K);
    t.kp1 = kl; t.kp2 = f.kp_right; t.success = f.success;
    t.pt = f.pt; t.flags = f.flags;
    STAGE(call.start());
    STAGE(gftt_select(call, g));
    HIPCHK(lh_launch_kf_assemble(s, &f));
    STAGE(klt_pyr_track(s, a, have_I));
    HIPCHK(lh_launch_triangulate(s, &t));
    HIPCHK(lh_launch_kf_finish(s, &f));
    STAGE(call.stop());
    HIPCHK(hipMemcpyAsync(fe.s_kfout.p, ko, o_end, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint8_t* st = fe.s_kfout.p;
    const int32_t* cnt = (const int32_t*)(st + o_cnt);
    const int32_t m = cnt[0];
    if (m < 0 || m > mc) return LH_E_HIP;
    const size_t N = NH + (size_t)m;
    const ByteSeg seg[5] = {{out->kp_new, st + o_new, sizeof(float) * 2 * (size_t)m},
                            {out->kp_right, st + o_kpr, sizeof(float) * 2 * N},
                            {out->success, st + o_succ, N},
                            {out->pt, st + o_pt, sizeof(double) * 3 * N},
                            {out->flags, st + o_flag, N}};
    par_copy(h, seg, 5);
    out->n_new = m;
    out->n_candidates = cnt[1];
    out->n_right = cnt[2];
    out->n_accepted = cnt[3];
    out->lambda_max = *(const double*)(st + o_lam);
    STAGE(call.time(&out->time_ms));
    fe.r_cols = cols;
    fe.r_rows = rows;
    fe.r_levels = in->img_left ? a.n_levels : std::max(fe.r_levels, a.n_levels);
    fe.r_valid = true;
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
int lh_track_frame(lh_handle* h, const lh_track_input* in, lh_track_result* out) {
    return no_throw(track_frame_impl, h, in, out);
}
int lh_insert_keyframe(lh_handle* h, const lh_keyframe_input* in, lh_keyframe_result* out) {
    return no_throw(insert_keyframe_impl, h, in, out);
}

}  // extern "C"
