// lh_launch.h — the one declaration of every kernel launcher.  The definitions (lh_lin.hip, lh_kernels.hip and its lh_probe.hip, lh_frames.hip,
// lh_aux.hip, lh_lk.hip, lh_klt.hip, lh_tri.hip, lh_gftt.hip, lh_track.hip, lh_keyframe.hip, lh_cov.hip, lh_marg.hip) and the callers (lh_host.cpp, lh_frontend.cpp, lh_cov_host.cpp, lh_marg_host.cpp) all include it: the symbols are extern "C", so only
// the compiler, seeing a definition beside this declaration, can tell that the two sides disagree.
// (lh_tri.h, lh_gftt.h, lh_klt.h, lh_track.h, lh_cov.h and lh_marg.h are also compiled by plain g++ for the CPU probes and hold no HIP type: hence this header.
// lh_keyframe.h holds its kernels' arguments alone, and no HIP type either.)
#pragma once
#include <hip/hip_runtime.h>

#include "lh_common.h"
#include "lh_cov.h"
#include "lh_gftt.h"
#include "lh_keyframe.h"
#include "lh_klt.h"
#include "lh_lk.h"
#include "lh_marg.h"
#include "lh_track.h"
#include "lh_tri.h"

extern "C" {
hipError_t lh_prepare_lin(int lds_limit);
size_t lh_lin_smem(int T, int ncam, int nw);
hipError_t lh_launch_nop(hipStream_t st);
hipError_t lh_launch_outliers(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                              double th0, unsigned* part, uint8_t* flags);
hipError_t lh_launch_p2p(hipStream_t st, double* rs, double* maxd, int n, lh_peers peers, int rank, int world,
                         int parity, unsigned long long tag, long slot, int mode, int* err);
hipError_t lh_launch_outlier_counts(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                                    double th0, unsigned* part, double* tot);
hipError_t lh_launch_outlier_flags(hipStream_t st, const double* rho, const int32_t* obs_perm, long nslots, long n_obs,
                                   double th0, const double* gtot, uint8_t* flags);
hipError_t lh_launch_lin(int T, int nw, int trial, int nchunks, int chunk_base, hipStream_t st, const lh_chunk* chunks,
                         const lh_subbatch* sbs, const float* obs_uv, const uint32_t* obs_meta, double* rec,
                         double* ptab, const double* ext, const lh_ctrl* ctrl, const double* dxp,
                         double* edge_rho, double* rows, double* csc, const uint32_t* crow, uint8_t* wflag,
                         long nslots, lh_params prm, int nrec, const uint64_t* fixed_bits, double* pose_mat,
                         int writer, lh_reset_args rst);
hipError_t lh_launch_reduce(hipStream_t st, const double* rows, const double* csc, const uint32_t* red_tab, int nred,
                            lh_ctrl* ctrl, double* rs_stage, double* rs_commit, double* maxd,
                            lh_params prm, int n_chunks, int mode, int* host_done, int seq, double* img);
hipError_t lh_launch_img_init(hipStream_t st, double* img, int n);
hipError_t lh_launch_ldlt_g_probe(const double* S, const double* b, int n, double* x, double* gA);
hipError_t lh_launch_ctrl(hipStream_t st, lh_ctrl* ctrl, double* rs_commit, const double* rs_stage, const double* maxd,
                          const uint32_t* rsmap, const uint16_t* pair_pq, double* dxp, lh_params prm, int mode,
                          int* host_done, int seq, double* gA, const double* gS,
                          const int32_t* brow_ptr, const uint32_t* brow_ent, const uint16_t* units, lh_band_args band,
                          double* img, int kind);
hipError_t lh_launch_dense(hipStream_t st, const double* rs_stage, const uint16_t* pair_pq, const lh_ctrl* ctrl,
                           double* gS, int P);
hipError_t lh_launch_gather(hipStream_t st, const lh_ctrl* ctrl, const double* rec, const int32_t* lm_perm, int nrec,
                            const double* rho, const int32_t* obs_perm, long nslots, double* out_xyz, double* out_rho);
hipError_t lh_launch_ldlt_probe(const double* S, const double* b, int n, double* x, int solver, double tol, int max_it,
                                int* iters);
hipError_t lh_launch_mfma_probe(const double* A, const double* B, double* D);
hipError_t lh_read_stamps(unsigned long long* out, int n, int reset);
hipError_t lh_read_lin_stamps(unsigned long long* out, int n);
hipError_t lh_launch_frames(hipStream_t st, int n_frames, const int64_t* obs_ptr, const double* pose_in,
                            const double* pts, const double* uv, const uint8_t* flag_in, lh_params prm, double* res,
                            double* pose_out, uint8_t* flag_out, double* rchi2_out, int32_t* iters_out,
                            int32_t* inliers_out);
hipError_t lh_launch_lk_pyr(hipStream_t st, const uint8_t* src, int sw, int sh, int64_t sstep, uint8_t* dst, int dw,
                            int dh);
hipError_t lh_launch_lk_track(hipStream_t st, const lh_lk_levels* L1, const lh_lk_levels* L2, int levels, int n,
                              const float* kp1, const float* kp2_in, float* kp2_out, uint8_t* success, int inverse,
                              int has_initial);
hipError_t lh_launch_klt_pyr(hipStream_t st, const uint8_t* src, int sw, int sh, int64_t sstep, uint8_t* dst, int dw,
                             int dh);
hipError_t lh_launch_klt_track(hipStream_t st, const lh_klt_args* a);
hipError_t lh_launch_triangulate(hipStream_t st, const lh_tri_args* a);
hipError_t lh_launch_gftt_front(hipStream_t st, const lh_gftt_args* a);
hipError_t lh_launch_gftt_rounds(hipStream_t st, const lh_gftt_args* a, int first, int count);
hipError_t lh_launch_gftt_order(hipStream_t st, const lh_gftt_args* a);
hipError_t lh_launch_track_guess(hipStream_t st, const lh_track_args* a);
hipError_t lh_launch_track_pack(hipStream_t st, const lh_track_args* a);
hipError_t lh_launch_kf_assemble(hipStream_t st, const lh_kf_args* a);
hipError_t lh_launch_kf_finish(hipStream_t st, const lh_kf_args* a);
hipError_t lh_launch_cov_snapshot(hipStream_t st, const lh_cov_snap_args* a);
hipError_t lh_launch_cov_pose(hipStream_t st, const lh_cov_args* a);
hipError_t lh_launch_cov_lm(hipStream_t st, const lh_cov_lm_args* a, lh_params prm);
hipError_t lh_launch_marg_mask(hipStream_t st, const lh_marg_mask_args* a);
hipError_t lh_launch_marg_prior(hipStream_t st, const lh_marg_args* a);
}
