// lh_cov_host.cpp — lh_covariance (include/lego_ba.h): the marginal covariances of the window the
// handle last solved.  One stream of launches and one download:
//   k_cov_snapshot                     the returned state (committed poses, tables, landmarks) as lh_reset_args;
//   k_lin<T, false>, k_reduce mode 0   the solver's own kernels, unchanged, linearise there into buffers of this
//                                      file's (lh::CovState): the lambda-free packed S and the records with chol(H_ll);
//   k_cov_factor, _linv, _gram         Sigma_pp;  k_cov_lm  Sigma_l (only when asked for).
// The committed system of the solve is not used: an accepted evaluate-only trial of the final iteration commits the
// state and writes no system, so the system is always formed again.  The solver's state is only read.
// The first two steps are lh::relin_enqueue, which lh_marginalize (lh_marg_host.cpp) runs too.
#include <cstring>

#include "lh_handle.h"
#include "lh_launch.h"

using namespace lh;

namespace {

bool pose_held(const lh_handle* h, int p, int anchor) {
    return ((h->plan.fixed_bits[p >> 6] >> (p & 63)) & 1ull) != 0ull || p == anchor;
}

int covariance_impl(lh_handle* h, const lh_cov_input* in, lh_cov_result* out) {
    if (!h || !in || !out) return LH_E_BADARG;
    FrontendCall call(h);
    STAGE(call.select());
    if (!h->uploaded || !h->solved) return LH_E_STATE;
    if (h->opt.world_size > 1 || h->P > LH_PMAX_WIN) return LH_E_UNSUPPORTED;
    const int P = h->P, anchor = in->anchor, n6 = 6 * P;
    if (anchor < -1 || anchor >= P) return LH_E_BADARG;
    out->n_free = 0; out->bad_row = -1; out->min_pivot = 0.0; out->max_pivot = 0.0; out->time_ms = 0.0;
    int nfree = 0;
    for (int p = 0; p < P; ++p) nfree += pose_held(h, p, anchor) ? 0 : 6;
    out->n_free = nfree;
    if (nfree == 0) { out->bad_row = 0; return LH_E_SINGULAR; }

    hipStream_t s = h->stream;
    CovState& cv = h->cov;
    const int ns = (nfree + LH_COV_NB - 1) & ~(LH_COV_NB - 1);
    const size_t nrec = (size_t)h->n_rec, L = (size_t)h->L;
    // the download: the result block, then the arrays asked for (Sigma_pp stays on the device when it is not)
    const size_t o_blk = LH_COV_R_N, o_full = o_blk + (out->pose_cov ? 36 * (size_t)P : 0);
    const size_t o_lm = o_full + (out->pose_cov_full ? (size_t)n6 * n6 : 0), n_out = o_lm + (out->lm_cov ? 9 * L : 0);
    STAGE(relin_ensure(h, cv.lin));
    HIPCHK(cv.rowmap.ensure(n6));
    HIPCHK(cv.A.ensure((size_t)ns * ns)); HIPCHK(cv.W.ensure((size_t)ns * ns));
    HIPCHK(cv.full.ensure((size_t)n6 * n6 + 36 * (size_t)P));
    HIPCHK(cv.out.ensure(n_out));
    HIPCHK(h->s_out.ensure(n_out));
    double* d_blk = out->pose_cov ? cv.out.p + o_blk : cv.full.p + (size_t)n6 * n6;
    double* d_full = out->pose_cov_full ? cv.out.p + o_full : cv.full.p;

    STAGE(call.start());
    STAGE(relin_enqueue(h, cv.lin, h->d_meta.p, h->d_rho.p, h->d_wflag.p, h->prm));
    // ---- Sigma_pp ----
    HIPCHK(hipMemsetAsync(d_full, 0, (size_t)n6 * n6 * sizeof(double), s));
    HIPCHK(hipMemsetAsync(d_blk, 0, 36 * (size_t)P * sizeof(double), s));
    const lh_cov_args ca{cv.lin.rs.p, h->d_pair_pq.p, h->d_fixed.p, P, h->LY.npairs, anchor, ns, cv.rowmap.p,
                         cv.A.p, cv.W.p, d_full, d_blk, cv.out.p};
    HIPCHK(lh_launch_cov_pose(s, &ca));
    // ---- Sigma_l ----
    if (out->lm_cov) {
        HIPCHK(hipMemsetAsync(cv.out.p + o_lm, 0xFF, 9 * L * sizeof(double), s));   // NaN: a landmark without a record
        const lh_cov_lm_args la{h->d_sbs.p, h->d_uv.p, h->d_meta.p, cv.lin.rec.p + nrec * LH_REC, cv.lin.ptab_init.p, h->d_ext.p,
                                h->d_lm_perm.p, cv.rowmap.p, d_full, cv.out.p, cv.out.p + o_lm, h->plan.n_sb, P};
        HIPCHK(lh_launch_cov_lm(s, &la, h->prm));
    }
    STAGE(call.stop());
    HIPCHK(hipMemcpyAsync(h->s_out.p, cv.out.p, n_out * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    STAGE(call.time(&out->time_ms));
    const double* r = h->s_out.p;
    out->min_pivot = r[LH_COV_R_MINP];
    out->max_pivot = r[LH_COV_R_MAXP];
    if (r[LH_COV_R_BAD] >= 0.0) { out->bad_row = (int32_t)r[LH_COV_R_BAD]; return LH_E_SINGULAR; }
    // rank-deficient landmarks that the solver does not hold fixed poison S (their factor's NaN marker)
    if (!h->opt.degenerate_guard && r[LH_COV_R_NDEG] != 0.0) { out->bad_row = 0; return LH_E_SINGULAR; }
    const ByteSeg seg[3] = {{out->pose_cov, r + o_blk, 36 * (size_t)P * sizeof(double)},
                            {out->pose_cov_full, r + o_full, (size_t)n6 * n6 * sizeof(double)},
                            {out->lm_cov, r + o_lm, 9 * L * sizeof(double)}};
    par_copy(h, seg, 3);
    return LH_OK;
}

}  // namespace

int lh::relin_ensure(lh_handle* h, ReLin& rl) {
    const int P = h->P, npt = P * h->ncam * LH_PT;
    HIPCHK(rl.qt_init.ensure(24 * (size_t)P)); HIPCHK(rl.ptab_init.ensure(2 * (size_t)npt));
    HIPCHK(rl.lm.ensure(3 * std::max<size_t>((size_t)h->L, 1)));
    HIPCHK(rl.qt.ensure(24 * (size_t)P)); HIPCHK(rl.ptab.ensure(2 * (size_t)npt));
    HIPCHK(rl.rec.ensure(2 * (size_t)h->n_rec * LH_REC)); HIPCHK(rl.dxp.ensure(6 * (size_t)P));
    HIPCHK(rl.rs.ensure(h->LY.total)); HIPCHK(rl.maxd.ensure(1)); HIPCHK(rl.ctrl.ensure(1));
    return LH_OK;
}

int lh::relin_enqueue(lh_handle* h, ReLin& rl, const uint32_t* meta, double* rho, uint8_t* wflag, const lh_params& lprm) {
    hipStream_t s = h->stream;
    const int P = h->P, npt = P * h->ncam * LH_PT;
    const lh_cov_snap_args sn{h->d_ctrl.p, h->d_qt.p, h->d_ptab.p, h->d_rec.p, h->d_lm_perm.p, P, npt, (int32_t)h->n_rec,
                              rl.qt_init.p, rl.ptab_init.p, rl.lm.p};
    HIPCHK(lh_launch_cov_snapshot(s, &sn));
    // (the pair blocks no chunk reaches are not written by k_reduce: zero)
    HIPCHK(hipMemsetAsync(rl.rs.p, 0, (size_t)h->LY.total * sizeof(double), s));
    const lh_reset_args rst{h->d_lm_perm.p, rl.lm.p, rl.qt_init.p, rl.ptab_init.p, 24 * P, 2 * npt, 6 * std::max(P, 1)};
    int writer = 1;
    for (int T = 1; T <= LH_TMAX; ++T) {   // as the solver's initial linearisation (lh_host.cpp launch_lin)
        const int c0 = h->plan.tgroup_begin[T], c1 = h->plan.tgroup_begin[T + 1];
        if (c1 == c0 && !(writer && T == LH_TMAX)) continue;
        HIPCHK(lh_launch_lin(T, h->plan.lin_waves, 0, c1 - c0, c0, s, h->d_chunks.p, h->d_sbs.p, h->d_uv.p, meta, rl.rec.p, rl.ptab.p,
                             h->d_ext.p, rl.ctrl.p, rl.dxp.p, rho, h->d_rows.p, h->d_csc.p, h->d_items.p,
                             wflag, (long)h->n_slots, lprm, h->n_rec, h->d_fixed.p, rl.qt.p, writer, rst));
        writer = 0;
    }
    lh_params prm = lprm;   // k_reduce writes the packed blocks: no controller image, no decision, nothing committed
    prm.img = 0; prm.bimg = 0; prm.dec_in_reduce = 0; prm.commit_in_reduce = 0;
    HIPCHK(lh_launch_reduce(s, h->d_rows.p, h->d_csc.p, h->d_red.p, h->n_red, rl.ctrl.p, rl.rs.p, rl.rs.p, rl.maxd.p, prm,
                            h->plan.n_chunks, 0, nullptr, 0, nullptr));
    return LH_OK;
}

extern "C" int lh_covariance(lh_handle* h, const lh_cov_input* in, lh_cov_result* out) {
    return no_throw(covariance_impl, h, in, out);
}
