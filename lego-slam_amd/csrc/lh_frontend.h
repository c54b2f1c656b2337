// lh_frontend.h — what the frontend's two host files share (internal): lh_frontend.cpp defines these, the fused
// calls of lh_frame.cpp (lh_track_frame, lh_insert_keyframe) are made of them.  Each is described at its definition.
#pragma once
#include "lh_frontend_layout.h"
#include "lh_handle.h"
#include "lh_launch.h"

namespace lh {

hipError_t upload_rows(hipStream_t s, uint8_t* dst, const uint8_t* src, int cols, int rows, int64_t step);
lh_params frames_params(const lh_handle* h, const double* K);
bool points_optional_ok(int n, const double* pts_w, const uint8_t* has_point);
bool image_ok(int cols, int rows, int64_t step);

int klt_check(const lh_klt_input* in, const float* kp2, const uint8_t* success);
int64_t klt_pyramid_layout(lh_klt_levels* v, int n_levels, uint8_t* buf, int64_t step);
size_t pyramid_bytes(int cols, int rows);
lh_klt_args klt_args(const lh_klt_input& k, uint8_t* I, uint8_t* J, int64_t step, int has_initial);
int klt_pyr_track(hipStream_t s, const lh_klt_args& a, int first_I);

int gftt_prepare(FrontendState& fe, int cols, int rows, double quality_level, double min_distance, int limit, lh_gftt_args* a);
int gftt_select(FrontendCall& call, const lh_gftt_args& a);

void tri_tests(lh_tri_args* a, double thr, int gate, double y_max, double z_min, double z_max, const double* T_out);

}  // namespace lh
